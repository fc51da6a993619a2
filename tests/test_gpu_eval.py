"""AP evaluation on the device (heal_eval_match): the reference's recorded TP / FP lists, the numpy restatement of its loop on the
same IoU bits, device-side counts, the append form and a captured replay.  The kernel is driven through the C ABI with every
operand inside a NaN-filled buffer and every output inside a sentinel-filled one, so a read or write past the live counts shows."""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden import eval_margins as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64                      # guard elements on either side of every buffer
SENT_I, SENT_B = -7, 0xEE
THR3 = (0.3, 0.5, 0.7)
THR8 = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def g(golden):
    return golden("eval_match")


def _guarded(arr, cap, fill=np.nan):
    """`arr` ([k, ...] f32) at the front of a capacity-`cap` region inside a `fill`ed device buffer with guard pads."""
    arr = np.ascontiguousarray(arr, np.float32)
    per = int(np.prod(arr.shape[1:])) if arr.ndim > 1 else 1
    host = np.full(2 * PAD + max(cap, 1) * per, fill, np.float32)
    host[PAD:PAD + arr.size] = arr.reshape(-1)
    return dev(host), per


def _ptr(t, offset_elems=0):
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


class Abi:
    """One heal_eval_match call through ctypes.  n_cap / m_cap: capacities (default: the operand sizes); dev_counts: pass the
    live counts in device words; append: (stride, cursor, gt_total) to use the append form."""

    def __init__(self, det, score, gt, thr, n_cap=None, m_cap=None, dev_counts=False, append=None, want_gi=True):
        from heal_amd import _capi
        n, m, T = len(det), len(gt), len(thr)
        n_cap = n if n_cap is None else n_cap
        m_cap = m if m_cap is None else m_cap
        self.n, self.T = n, T
        det_b, det_f = _guarded(det, n_cap)
        gt_b, gt_f = _guarded(gt, m_cap)
        sc_b, _ = _guarded(score, n_cap)
        if n == 0:
            det_f = 24
        if m == 0:
            gt_f = 24
        stride = n_cap if append is None else append[0]
        self.stride = stride
        self.order = torch.full((2 * PAD + stride,), SENT_I, dtype=torch.int32, device=DEV)
        self.tp = torch.full((2 * PAD + T * stride,), SENT_B, dtype=torch.uint8, device=DEV)
        self.gi = torch.full((2 * PAD + T * stride,), SENT_I, dtype=torch.int32, device=DEV)
        self.sorted = torch.full((2 * PAD + stride,), float("nan"), dtype=torch.float32, device=DEV)
        counts = torch.tensor([n, m], dtype=torch.int32, device=DEV)
        self.words = torch.tensor([0, 0, 0] if append is None else [append[1], append[2], 0], dtype=torch.int32, device=DEV)
        null = ctypes.c_void_p(0)
        ws_bytes = _capi.query("heal_eval_match_workspace", n_cap, m_cap)
        ws = torch.full((ws_bytes // 4 + 2 * PAD,), float("nan"), dtype=torch.float32, device=DEV)
        thr_host = (ctypes.c_float * T)(*[float(v) for v in thr])
        self.keep = (det_b, gt_b, sc_b, counts, ws)
        _capi.call("heal_eval_match", _ptr(det_b, PAD), det_f, n_cap, _ptr(counts, 0) if dev_counts else null,
                   _ptr(sc_b, PAD), _ptr(gt_b, PAD), gt_f, m_cap, _ptr(counts, 1) if dev_counts else null, thr_host, T,
                   _ptr(self.order, PAD), _ptr(self.tp, PAD), _ptr(self.gi, PAD) if want_gi else null, _ptr(self.sorted, PAD),
                   stride, *(([null] * 3) if append is None else [_ptr(self.words, k) for k in range(3)]),
                   _ptr(ws, PAD), ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[:PAD]).all()) and bool(torch.isnan(ws[PAD + ws_bytes // 4:]).all())

    def rows(self, base=0, n=None):
        """-> (order [n], tp [T,n], gt_index [T,n], score_sorted [n]) as numpy, the rows at offset `base`."""
        n = self.n if n is None else n
        s, T = self.stride, self.T
        o = self.order.cpu().numpy()[PAD:PAD + s]
        tp = self.tp.cpu().numpy()[PAD:PAD + T * s].reshape(T, s)
        gi = self.gi.cpu().numpy()[PAD:PAD + T * s].reshape(T, s)
        sc = self.sorted.cpu().numpy()[PAD:PAD + s]
        return o[base:base + n], tp[:, base:base + n], gi[:, base:base + n], sc[base:base + n]

    def assert_untouched_outside(self, base, n):
        """Guard pads and every row outside [base, base + n) still hold their sentinels."""
        s, T = self.stride, self.T
        o, sc = self.order.cpu().numpy(), self.sorted.cpu().numpy()
        tp, gi = self.tp.cpu().numpy(), self.gi.cpu().numpy()
        live = np.zeros(s, bool)
        live[base:base + n] = True
        for buf, sent, reps in ((o, SENT_I, 1), (tp, SENT_B, T), (gi, SENT_I, T)):
            assert (buf[:PAD] == sent).all() and (buf[PAD + reps * s:] == sent).all()
            assert (buf[PAD:PAD + reps * s].reshape(reps, s)[:, ~live] == sent).all()
        assert np.isnan(sc[:PAD]).all() and np.isnan(sc[PAD + s:]).all() and np.isnan(sc[PAD:PAD + s][~live]).all()


def device_iou(det, gt):
    """The IoU matrix of the fallback path: heal_quad_iou on the footprints (the bits the fused kernel must reproduce)."""
    from heal_amd import ops
    if len(det) == 0 or len(gt) == 0:
        return np.zeros((len(det), len(gt)), np.float32)
    return ops.quad_iou(dev(M.footprints(det)), dev(M.footprints(gt))).cpu().numpy()


def expected(det, score, gt, thr):
    from heal_amd.opencood.utils.eval_utils import _greedy_match
    order, tp, gi = _greedy_match(device_iou(det, gt), thr, score)
    return order, tp, gi, np.asarray(score, np.float32)[order]


def assert_rows(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape
        if a.dtype == np.float32:
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            np.testing.assert_array_equal(a.astype(np.int64), b.astype(np.int64))


def corners(boxes):
    """[k,7] (x, y, z, h, w, l, yaw) -> [k,8,3] f32 (footprint corners first)."""
    x, y, z, h, w, l, yaw = (boxes[:, i] for i in range(7))
    c, s = np.cos(yaw), np.sin(yaw)
    sx, sy = np.array([1, 1, -1, -1]), np.array([1, -1, -1, 1])
    px = x[:, None] + 0.5 * (l[:, None] * sx * c[:, None] - w[:, None] * sy * s[:, None])
    py = y[:, None] + 0.5 * (l[:, None] * sx * s[:, None] + w[:, None] * sy * c[:, None])
    lo = np.stack([px, py, np.repeat((z - h / 2)[:, None], 4, 1)], -1)
    hi = np.stack([px, py, np.repeat((z + h / 2)[:, None], 4, 1)], -1)
    return np.concatenate([lo, hi], 1).astype(np.float32)


def random_frame(seed, n, m, tie_scores=False):
    """A crowded frame: m cars in a small lot (many overlap), detections jittered off random cars plus clutter."""
    rng = np.random.default_rng(seed)
    side = 6.0 * max(1.0, np.sqrt(m))
    cars = np.stack([rng.uniform(-side, side, m), rng.uniform(-side, side, m), np.full(m, -1.0), rng.uniform(1.4, 1.8, m),
                     rng.uniform(1.7, 2.2, m), rng.uniform(3.8, 5.0, m), rng.uniform(-np.pi, np.pi, m)], 1)
    src = cars[rng.integers(0, m, n)] if m else np.zeros((n, 7))
    det = src.copy()
    det[:, :2] += rng.normal(0, 1, (n, 1)) * rng.choice([0.05, 0.3, 0.8, 6.0], (n, 1))
    det[:, 6] += rng.normal(0, 0.05, n)
    if m == 0:
        det[:, 3:6] = [1.5, 2.0, 4.5]
    score = rng.random(n).astype(np.float32)
    if tie_scores:
        score = np.round(score, 1).astype(np.float32)
    return corners(det), score, corners(cars)


# ---- the reference's recorded lists --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_frames_exact_in_one_launch(g, tag):
    det, score, gt = g[f"{tag}_det"], g[f"{tag}_det_score"], g[f"{tag}_gt_boxes"]
    run = Abi(det, score, gt, THR3)
    order, tp, gi, sc = run.rows()
    np.testing.assert_array_equal(order, g[f"{tag}_order"])
    np.testing.assert_array_equal(gi, g[f"{tag}_gt_index"])
    for t in range(3):
        np.testing.assert_array_equal(tp[t], g[f"{tag}_tp"][t])
        np.testing.assert_array_equal(1 - tp[t].astype(int), g[f"{tag}_fp"][t])
        assert sc.tolist() == g[f"{tag}_score"][t].tolist()
    run.assert_untouched_outside(0, len(det))


def test_golden_run_through_three_single_threshold_calls(g):
    """tools/inference.py's loop: caluclate_tp_fp per frame and threshold, then the reference's AP for the run."""
    from heal_amd.opencood.utils import eval_utils as E
    stat = E.new_result_stat()
    for tag in ("a", "b"):
        det, score, gt = (dev(g[f"{tag}_{k}"]) for k in ("det", "det_score", "gt_boxes"))
        for thr in THR3:
            E.caluclate_tp_fp(det, score, gt if thr != 0.5 else gt.cpu(), stat, thr)      # a host tensor is copied over
    for t, thr in enumerate(THR3):
        for k in ("tp", "fp", "score"):
            assert stat[thr][k] == g[f"run_{k}"][t].tolist(), (thr, k)
        assert stat[thr]["gt"] == int(g["run_gt"][t])
        ap, mrec, mpre = E.calculate_ap(stat, thr)
        assert ap == float(g["run_ap"][t]) and mrec == g["run_mrec"][t].tolist() and mpre == g["run_mpre"][t].tolist()


# ---- kernel path == fallback path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,thr", [(1, 1, (0.5,)), (1, 65, (0.5,)), (63, 64, THR3), (64, 64, THR3), (65, 64, THR3),
                                     (200, 129, THR8), (1024, 256, THR3)])
def test_kernel_equals_fallback_bit_for_bit(n, m, thr, monkeypatch):
    from heal_amd.opencood.utils import eval_utils as E
    det, score, gt = random_frame(100 * n + m, n, m, tie_scores=(n == 200))
    want = expected(det, score, gt, thr)
    assert 0 < want[1].sum() < want[1].size or n == 1
    run = Abi(det, score, gt, thr)
    assert_rows(run.rows(), want)
    run.assert_untouched_outside(0, n)
    for t, one in enumerate(thr):                                   # every threshold of the launch against a launch of its own
        o1, tp1, gi1, sc1 = Abi(det, score, gt, (one,)).rows()
        assert_rows((o1, tp1[0], gi1[0], sc1), (want[0], want[1][t], want[2][t], want[3]))
    fused, fallback = E.new_result_stat(thr), E.new_result_stat(thr)
    E.caluclate_tp_fp_multi(dev(det), dev(score), dev(gt), fused, thr)
    monkeypatch.setenv("HEAL_EVAL_FUSED", "0")
    E.caluclate_tp_fp_multi(dev(det), dev(score), dev(gt), fallback, thr)
    assert fused == fallback
    for t, one in enumerate(thr):
        assert fused[one]["tp"] == want[1][t].tolist() and fused[one]["score"] == want[3].tolist() and fused[one]["gt"] == m


def test_empty_cases():
    from heal_amd.opencood.utils import eval_utils as E
    det, score, gt = random_frame(3, 20, 9)
    none = Abi(det[:0], score[:0], gt, THR3, n_cap=8, dev_counts=True)            # n = 0: nothing is written
    none.assert_untouched_outside(0, 0)
    order, tp, gi, sc = Abi(det, score, gt[:0], THR3).rows()                       # m = 0: all FP
    assert tp.sum() == 0 and (gi == -1).all()
    assert_rows((order, sc), (np.argsort(-score, kind="stable"), score[np.argsort(-score, kind="stable")]))
    stat = E.new_result_stat()
    E.caluclate_tp_fp_multi(dev(det[:0]), dev(score[:0]), dev(gt), stat)            # n = 0 through the module: gt is still added
    E.caluclate_tp_fp(None, None, dev(gt), stat, 0.5)                               # det_boxes None
    E.caluclate_tp_fp(dev(det), dev(score), dev(gt[:0]), stat, 0.7)
    assert [stat[t]["gt"] for t in THR3] == [9, 18, 9] and stat[0.3]["tp"] == [] and stat[0.5]["score"] == []
    assert stat[0.7]["tp"] == [0] * 20 and stat[0.7]["fp"] == [1] * 20 and stat[0.7]["gt"] == 9
    app = Abi(det[:0], score[:0], gt, THR3, n_cap=0, append=(16, 5, 100))           # append form: only gt_total moves
    assert app.words.tolist() == [5, 109, 0]
    app.assert_untouched_outside(0, 0)


def test_device_counts_with_slack_capacity():
    det, score, gt = random_frame(11, 37, 11)
    want = expected(det, score, gt, THR3)
    by_value = Abi(det, score, gt, THR3)
    run = Abi(det, score, gt, THR3, n_cap=1024, m_cap=256, dev_counts=True)        # the tails are NaN
    assert_rows(run.rows(), want)
    assert_rows(run.rows(), by_value.rows())
    run.assert_untouched_outside(0, 37)


def test_quad_form_equals_corner_form():
    det, score, gt = random_frame(12, 90, 40)
    full = Abi(det, score, gt, THR3).rows()
    assert_rows(Abi(M.footprints(det), score, M.footprints(gt), THR3).rows(), full)
    assert_rows(Abi(det, score, M.footprints(gt), THR3).rows(), full)


def test_equal_scores_follow_index_order():
    det, _, gt = random_frame(13, 70, 20)
    score = np.full(70, 0.5, np.float32)
    score[[5, 40]] = 0.75
    score[[9, 66]] = [0.0, -0.0]
    order, tp, gi, sc = Abi(det, score, gt, (0.5,)).rows()
    rest = [i for i in range(70) if i not in (5, 40, 9, 66)]
    assert order.tolist() == [5, 40] + rest + [9, 66]
    assert_rows((order, tp, gi, sc), expected(det, score, gt, (0.5,)))


def test_duplicate_detections_give_one_tp():
    _, _, gt = random_frame(14, 1, 6)
    det = np.repeat(gt[2:3], 50, axis=0)
    score = np.linspace(0.9, 0.1, 50).astype(np.float32)
    far = gt[:, :, :2].max() + 50.0
    gt_far = gt.copy()
    gt_far[np.arange(6) != 2, :, 0] += far                        # the other boxes are out of reach
    order, tp, gi, _ = Abi(det, score, gt_far, THR3).rows()
    assert tp.sum(axis=1).tolist() == [1, 1, 1] and (tp[:, 0] == 1).all() and (gi[:, 0] == 2).all() and (gi[:, 1:] == -1).all()


def test_later_detection_falls_to_another_box():
    """Two overlapping boxes and three detections: the second detection's best box is taken, it must take the OTHER one (the
    VOC variant calls it FP); the third finds both gone."""
    box = lambda y: corners(np.array([[0.0, y, -1.0, 1.5, 2.0, 4.5, 0.0]]))[0]
    gt = np.stack([box(0.0), box(1.2)])
    det = np.stack([box(0.05), box(0.5), box(0.9)])
    score = np.array([0.9, 0.8, 0.7], np.float32)
    iou = device_iou(det, gt)
    assert iou[1, 0] > iou[1, 1] > 0.3 and iou[2, 1] > 0.3
    order, tp, gi, _ = Abi(det, score, gt, (0.3,)).rows()
    assert tp[0].tolist() == [1, 1, 0] and gi[0].tolist() == [0, 1, -1]


def test_beyond_the_limits_error_and_fallback():
    from heal_amd import _capi
    from heal_amd.opencood.utils import eval_utils as E
    from oracle import cref
    det, score, gt = random_frame(15, 1030, 20)
    for args in ((det[:1025], score[:1025], gt, THR3), (det[:4], score[:4], np.repeat(gt, 13, 0)[:257], THR3),
                 (det[:4], score[:4], gt, THR8 + (0.9,))):
        with pytest.raises(_capi.HealAmdError, match="heal_eval_match"):
            Abi(*args)
    for d, s, b in ((det, score, gt), (det[:10], score[:10], np.repeat(gt, 13, 0)[:257])):
        stat = E.new_result_stat()
        E.caluclate_tp_fp_multi(dev(d), dev(s), dev(b), stat)
        order, tp, _ = E._greedy_match(cref.quad_iou(M.footprints(d), M.footprints(b)), THR3, s)
        for t, thr in enumerate(THR3):
            assert stat[thr]["tp"] == tp[t].tolist() and stat[thr]["score"] == s[order].tolist() and stat[thr]["gt"] == len(b)


# ---- DeviceResultStat ----------------------------------------------------------------------------------------------------------
def test_device_result_stat_equals_per_frame_calls(g):
    from heal_amd.opencood.utils import eval_utils as E
    frames = [(g["a_det"], g["a_det_score"], g["a_gt_boxes"]), random_frame(21, 50, 70), (g["b_det"], g["b_det_score"], g["b_gt_boxes"])]
    acc = E.DeviceResultStat(capacity=512)
    stat = E.new_result_stat()
    for det, score, gt in frames:
        acc.add(dev(det), dev(score), dev(gt))
        E.caluclate_tp_fp_multi(dev(det), dev(score), dev(gt), stat)
    got = acc.result_stat()
    assert got == stat
    assert [E.calculate_ap(got, t)[0] for t in THR3] == [E.calculate_ap(stat, t)[0] for t in THR3]
    assert acc.result_stat() == stat                                # reading does not disturb the buffers


def test_append_overflow_sets_flag_and_writes_nothing():
    from heal_amd.opencood.utils import eval_utils as E
    det, score, gt = random_frame(22, 30, 8)
    fits = Abi(det, score, gt, THR3, append=(40, 10, 3))
    assert fits.words.tolist() == [40, 11, 0]
    assert_rows(fits.rows(base=10), expected(det, score, gt, THR3))
    fits.assert_untouched_outside(10, 30)
    over = Abi(det, score, gt, THR3, append=(40, 11, 3))
    assert over.words.tolist() == [11, 3, 1]
    over.assert_untouched_outside(0, 0)
    acc = E.DeviceResultStat(capacity=50)
    acc.add(dev(det), dev(score), dev(gt))
    acc.add(dev(det), dev(score), dev(gt))
    with pytest.raises(RuntimeError, match="did not fit"):
        acc.result_stat()
    assert acc.buffers["cursor"].item() == 30 and acc.buffers["overflow"].item() == 1


def test_captured_add_on_decode_nms_buffers_follows_the_loaded_frame(golden):
    """decode_nms(sync=False) -> DeviceResultStat.add captured once on a side stream and replayed on two frames: the live counts
    are read on the device, so every replay appends what the eager path gives for the frame that is loaded."""
    from heal_amd import ops
    from heal_amd.opencood.utils import eval_utils as E
    d = golden("decode")
    anchors = dev(d["anchors"].astype(np.float32))
    gt_range = d["gt_range"].tolist()
    tfm = np.eye(4, dtype=np.float32)
    decode = lambda c, r, p, sync: ops.decode_nms(c, r, p, anchors, 0.2, 0.7853, 2, 0.15, tfm, gt_range, sync=sync)
    rng = np.random.default_rng(5)
    frames, want = [], E.new_result_stat()
    for tag, m in (("id", 60), ("tf", 23)):
        cls, reg, dirp = (dev(d[f"{tag}_{k}"]) for k in ("cls", "reg", "dir"))
        pred, score = decode(cls, reg, dirp, True)
        gt = pred[torch.from_numpy(rng.permutation(len(pred))[:m]).to(DEV)].clone()
        gt[:, :, :2] += torch.from_numpy(rng.normal(0, 0.3, (m, 1, 2)).astype(np.float32)).to(DEV)
        E.caluclate_tp_fp_multi(pred, score, gt, want)
        frames.append((cls, reg, dirp, gt))
    assert 0 < sum(want[0.7]["tp"]) < sum(want[0.3]["tp"])
    s_cls, s_reg, s_dir = (torch.empty_like(t) for t in frames[0][:3])
    s_gt = torch.full((256, 8, 3), float("nan"), device=DEV)
    s_m = torch.zeros(1, dtype=torch.int32, device=DEV)
    acc = E.DeviceResultStat(capacity=1024)
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            corners_buf, score_buf, count = decode(s_cls, s_reg, s_dir, False)
            acc.add(corners_buf, score_buf, s_gt, n_dev=count, m_dev=s_m)
        for cls, reg, dirp, gt in frames:
            s_cls.copy_(cls), s_reg.copy_(reg), s_dir.copy_(dirp)
            s_gt.fill_(float("nan"))
            s_gt[:len(gt)] = gt
            s_m.fill_(len(gt))
            graph.replay()
        st.synchronize()
    assert acc.result_stat() == want
