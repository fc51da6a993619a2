"""Late-fusion decode + pooled NMS (heal_decode_nms_agents), the parts that need no GPU: the C ABI, the golden fixture's own
margins, the wrapper's refusals and the post-processor's dispatch."""
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests.golden import late_margins as M

NEW_SYMBOLS = ("heal_decode_nms_agents", "heal_decode_nms_agents_workspace")


def test_abi_12_declares_and_exports_the_agents_entry_points():
    declared = _capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/heal_amd.h"
        assert name in _capi.signatures(), f"{name} has no ctypes signature"
    assert _capi.abi_version_of_header() == 13
    from heal_amd import build
    build.build()
    lib = _capi.lib()
    assert int(lib.heal_abi_version()) == 13
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libheal_amd.so does not export {name}"
    header = open(_capi.HEADER).read()
    assert "voxel_postprocessor.py:277-405" in header
    # the workspace query is host arithmetic: the single-cav carve over the pooled anchor count plus the agent table
    need = _capi.query("heal_decode_nms_agents_workspace", 5 * 131072, 1000)
    assert 5 * 131072 * 8 < _capi.query("heal_decode_nms_workspace", 5 * 131072, 1000) < need


def _params(g):
    return (float(g["score_thr"]), float(g["dir_offset"]), int(g["num_bins"]), float(g["nms_thr"]), g["gt_range"].tolist())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_keeps_every_margin(golden, tag):
    """Recomputed in numpy (IoU from oracle.cref): distinct scores 1e-5 apart and away from the threshold, no filter quantity or
    corner within 1e-3 of its limit, no top-1000 pair within 1e-3 of nms_thresh."""
    g = golden("late_decode")
    cavs = M.case_cavs(g, tag)
    bad, info = M.offenders(cavs, *_params(g))
    assert bad == [], f"{len(bad)} candidates sit on an edge: {bad[:8]}"
    assert info["near_threshold"] == 0
    assert info["min_score_gap"] >= M.SCORE_MARGIN
    assert g[f"{tag}_pred"].shape[1:] == (8, 3) and g[f"{tag}_pred"].shape[0] == g[f"{tag}_score"].shape[0] > 0
    assert g[f"{tag}_pred"].dtype == np.float32 and g[f"{tag}_score"].dtype == np.float32
    # the reference's kept scores are scores of passing pooled candidates, in descending order
    assert bool((np.diff(g[f"{tag}_score"]) < 0).all())


def test_fixture_reaches_its_edges(golden):
    g = golden("late_decode")
    thr, off, bins, nms, rng = _params(g)
    a = M.case_cavs(g, "a")
    assert len(a) == 5
    _, info = M.offenders(a, thr, off, bins, nms, rng)
    above, passing = info["per_agent_above"], info["per_agent_passing"]
    assert above.count(0) == 1, "one cav has no score above the threshold"
    filtered = [k for k in range(5) if above[k] > 0 and passing[k] == 0]
    assert len(filtered) == 1 and above[filtered[0]] >= 50, "one cav's candidates all fail the size / z filters"
    grids = [c["cls"].shape[2:] for c in a]
    assert grids.count((32, 32)) >= 3 and any(s != (32, 32) and s[0] != s[1] for s in grids), grids
    other = [c for c in a if c["cls"].shape[2:] != (32, 32)][0]
    assert not np.array_equal(other["anchors"].reshape(-1, 7)[:64], a[0]["anchors"].reshape(-1, 7)[:64])
    tfms = [c["tfm"] for c in a]
    assert all(not np.allclose(tfms[i], tfms[j]) for i in range(5) for j in range(i))
    assert sum(not np.allclose(t, np.eye(4)) for t in tfms) >= 4
    # kept boxes come from more than one cav
    agents = M.expected_agents(a, g["a_score"], thr, off, bins)
    assert len(set(agents.tolist())) >= 3
    b = M.case_cavs(g, "b")
    _, info_b = M.offenders(b, thr, off, bins, nms, rng)
    assert info_b["passing"] > M.TOP, "the second case pools more than 1000 filter-passing candidates"
    for name in g.files:
        assert g[name].dtype.kind in "fiu", f"{name}: the fixture holds numeric data only"
    path = os.path.join(os.path.dirname(__file__), "golden", "late_decode.npz")
    assert os.path.getsize(path) < 1 << 20


# ---- wrapper refusals: nothing here may touch a device -------------------------------------------------------------------
def _maps(n, H=4, W=6, A=2):
    return ([torch.zeros(1, A, H, W) for _ in range(n)], [torch.zeros(1, 7 * A, H, W) for _ in range(n)],
            [torch.zeros(1, 2 * A, H, W) for _ in range(n)], [torch.zeros(H, W, A, 7) for _ in range(n)])


def _call(cls, reg, dirs, anchors, tfms):
    return ops.decode_nms_agents(cls, reg, dirs, anchors, tfms, 0.2, 0.7853, 2, 0.15, [-1, -1, -3, 1, 1, 1])


@pytest.fixture
def no_device(monkeypatch):
    """Any native call or workspace allocation fails the test; _need lets CPU tensors through so the shape checks are reached."""
    def boom(*a, **k):
        raise AssertionError("the wrapper reached the device")
    monkeypatch.setattr(_capi, "call", boom)
    monkeypatch.setattr(_capi, "query", boom)
    monkeypatch.setattr(ops, "_workspace", boom)

    def shapes_only():
        monkeypatch.setattr(ops, "_need", lambda t, dtype, name: t)
    return shapes_only


def test_wrapper_refuses_cpu_tensors(no_device):
    cls, reg, dirs, anchors = _maps(2)
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP tensor"):
        _call(cls, reg, dirs, anchors, np.stack([np.eye(4)] * 2))


def test_wrapper_refuses_bad_agent_lists(no_device):
    cls, reg, dirs, anchors = _maps(3)
    eye = np.stack([np.eye(4)] * 3)
    with pytest.raises(_capi.HealAmdError, match="3 score maps, 2 regression maps"):
        _call(cls, reg[:2], dirs, anchors, eye)
    with pytest.raises(_capi.HealAmdError, match="2 anchor tables"):
        _call(cls, reg, dirs, anchors[:2], eye)
    with pytest.raises(_capi.HealAmdError, match="1 direction maps"):
        _call(cls, reg, dirs[:1], anchors, eye)
    cls9, reg9, dirs9, anchors9 = _maps(9)
    with pytest.raises(_capi.HealAmdError, match=r"1\.\.8 agents"):
        _call(cls9, reg9, dirs9, anchors9, np.stack([np.eye(4)] * 9))
    with pytest.raises(_capi.HealAmdError, match=r"1\.\.8 agents"):
        _call([], [], [], [], np.zeros((0, 4, 4)))


def test_wrapper_refuses_mismatched_anchors_and_poses(no_device):
    no_device()                       # shape checks on stand-in (CPU) tensors
    cls, reg, dirs, anchors = _maps(2)
    eye = np.stack([np.eye(4)] * 2)
    wrong = [anchors[0], torch.zeros(4, 5, 2, 7)]
    with pytest.raises(_capi.HealAmdError, match="anchors .* of agent 1 do not match"):
        _call(cls, reg, dirs, wrong, eye)
    with pytest.raises(_capi.HealAmdError, match="regression / direction maps do not match"):
        _call(cls, [reg[0], torch.zeros(1, 14, 4, 5)], dirs, anchors, eye)
    with pytest.raises(_capi.HealAmdError, match="batch size must be 1"):
        _call([torch.zeros(2, 2, 4, 6), cls[1]], reg, dirs, anchors, eye)
    with pytest.raises(_capi.HealAmdError, match="tfms is required"):
        _call(cls, reg, dirs, anchors, None)
    with pytest.raises(_capi.HealAmdError, match="tfms must be 2 4x4 matrices"):
        _call(cls, reg, dirs, anchors, np.stack([np.eye(4)] * 3))
    with pytest.raises(_capi.HealAmdError, match="tfms must be 2 4x4 matrices"):
        _call(cls, reg, dirs, anchors, np.zeros((2, 3, 4)))


def test_c_entry_refuses_both_or_neither_pose_argument():
    """heal_decode_nms_agents validates its operands on the host before any launch: the pose arguments, the agent count and
    null pointers are refused with an error message, without a device."""
    import ctypes
    from heal_amd import build
    build.build()
    one = (ctypes.c_void_p * 1)(0x1000)
    hw = (ctypes.c_int32 * 1)(4)
    g = (ctypes.c_float * 6)(-1, -1, -3, 1, 1, 1)
    t = (ctypes.c_float * 16)(*np.eye(4).reshape(-1).tolist())
    p = ctypes.c_void_p
    fake = p(0x1000)

    def call(n, tfm_host, tfm_dev, ws=p(0x10000), cls=one):
        _capi.call("heal_decode_nms_agents", n, cls, one, one, one, hw, hw, 2, 2, 0.2, 0.7853, 0.15, 1000, tfm_host, tfm_dev, g,
                   fake, fake, p(0), fake, 1000, ws, 1 << 30, p(0))

    with pytest.raises(_capi.HealAmdError, match="exactly one of tfm_host / tfm_dev"):
        call(1, t, fake)
    with pytest.raises(_capi.HealAmdError, match="exactly one of tfm_host / tfm_dev"):
        call(1, p(0), p(0))
    with pytest.raises(_capi.HealAmdError, match=r"n_agents must be in \[1,8\]"):
        call(9, t, p(0))
    with pytest.raises(_capi.HealAmdError, match="256-B aligned"):
        call(1, t, p(0), ws=p(0x10010))
    with pytest.raises(_capi.HealAmdError, match="null"):
        call(1, t, p(0), cls=(ctypes.c_void_p * 1)(0))
    big = (ctypes.c_int32 * 1)(40000)
    with pytest.raises(_capi.HealAmdError, match="below 2\\^31"):
        _capi.call("heal_decode_nms_agents", 1, one, one, one, one, big, big, 2, 2, 0.2, 0.7853, 0.15, 1000, t, p(0), g,
                   fake, fake, p(0), fake, 1000, p(0x10000), 1 << 30, p(0))


# ---- post-processor dispatch ---------------------------------------------------------------------------------------------
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the device: enough for the dispatch predicate, which only looks."""
    @property
    def is_cuda(self):
        return True


def _post():
    from heal_amd import configs
    from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    return VoxelPostprocessor(configs.m1_late([-12.8, -12.8, -3, 12.8, 12.8, 1])["postprocess"], train=False)


def _dicts(n, wrap=lambda t: t, **extra):
    shared = torch.zeros(4, 6, 2, 7)          # the cavs of one YAML share the anchor table
    data = {f"cav{k}": {"transformation_matrix": np.eye(4, dtype=np.float32), "anchor_box": shared} for k in range(n)}
    out = {f"cav{k}": dict({"cls_preds": wrap(torch.zeros(1, 2, 4, 6)), "reg_preds": wrap(torch.zeros(1, 14, 4, 6)),
                            "dir_preds": wrap(torch.zeros(1, 4, 4, 6))}, **extra) for k in range(n)}
    return data, out


def test_post_process_dispatch(monkeypatch):
    post = _post()
    seen = []
    monkeypatch.setattr(post, "_post_process_multi", lambda d, o: seen.append("multi") or ("multi", len(o)))
    monkeypatch.setattr(post, "_post_process_agents", lambda d, o: seen.append("agents") or ("agents", len(o)))
    as_cuda = lambda t: t.as_subclass(_Cuda)
    monkeypatch.delenv("HEAL_LATE_FUSED", raising=False)
    assert post.post_process(*_dicts(3)) == ("multi", 3)                       # CPU maps
    assert post.post_process(*_dicts(3, as_cuda)) == ("agents", 3)
    assert post.post_process(*_dicts(8, as_cuda)) == ("agents", 8)
    assert post.post_process(*_dicts(9, as_cuda)) == ("multi", 9)              # more cavs than the kernel takes
    assert post.post_process(*_dicts(2, as_cuda, iou_preds=torch.zeros(1))) == ("multi", 2)
    assert post.post_process(*_dicts(2, lambda t: as_cuda(t.double()))) == ("multi", 2)
    assert post.post_process(*_dicts(2, lambda t: as_cuda(torch.cat([t, t])))) == ("multi", 2)    # batch size 2
    monkeypatch.setenv("HEAL_LATE_FUSED", "0")
    assert post.post_process(*_dicts(3, as_cuda)) == ("multi", 3)
    assert seen == ["multi", "agents", "agents", "multi", "multi", "multi", "multi", "multi"]


def test_post_process_agents_hands_the_cavs_over_in_order(monkeypatch):
    """_post_process_agents: one decode_nms_agents call with the cavs of output_dict in order, each with its own anchors and
    matrix (tensor or numpy), and the YAML's thresholds."""
    post = _post()
    got = {}

    def fake(cls, reg, dirs, anchors, tfms, thr, dir_offset, num_bins, nms_thr, gt_range, **kw):
        got.update(cls=cls, reg=reg, dirs=dirs, anchors=anchors, tfms=tfms, args=(thr, dir_offset, num_bins, nms_thr, gt_range), kw=kw)
        return "boxes", "scores"
    monkeypatch.setattr(ops, "decode_nms_agents", fake)
    data, out = _dicts(3)
    for k in range(3):
        out[f"cav{k}"]["cls_preds"] += k
        data[f"cav{k}"]["transformation_matrix"] = (np.eye(4) * (k + 1)).astype(np.float32)
    data["cav1"]["transformation_matrix"] = torch.from_numpy(data["cav1"]["transformation_matrix"])
    data["cav2"]["anchor_box"] = np.ones((4, 6, 2, 7))
    assert post._post_process_agents(data, out) == ("boxes", "scores")
    assert [float(c.mean()) for c in got["cls"]] == [0.0, 1.0, 2.0]
    assert [float(np.asarray(t)[0, 0]) for t in got["tfms"]] == [1.0, 2.0, 3.0]
    assert got["anchors"][0] is got["anchors"][1] and got["anchors"][2].dtype == torch.float32 and float(got["anchors"][2].mean()) == 1.0
    assert got["args"] == (0.2, 0.7853, 2, 0.15, post.params["gt_range"]) and got["kw"] == {}
