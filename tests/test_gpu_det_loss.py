"""The fused criterion terms on the MI355X: heal_det_loss, heal_occ_loss and heal_depth_focal_loss through the loss classes and
through ops, against the reference's recorded values (tests/golden/loss.npz) and against the torch composition evaluated on
the CPU in float64 (that code is pinned to the reference by tests/test_host_cpu.py and is not under test here).

Bounds (the project's bar for backward kernels, tests/test_gpu_kd.py): loss within 1e-5 relative, every gradient tensor within
1e-5 x the largest magnitude of the expected tensor.  The float64 composition reproduces the recorded reference values to 9e-8
(loss) and 3e-7 of the largest element (gradients), i.e. the reference alone sits 30 x inside these bounds."""
import contextlib
import os

import numpy as np
import pytest
import torch

from heal_amd import configs, ops
from heal_amd.opencood.loss.point_pillar_depth_loss import FocalLoss
from heal_amd.opencood.tools.train_utils import create_loss
from tests.test_reference_live import _loss_inputs

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5
KERNELS = ("det_loss", "occ_loss", "depth_focal_loss")
CASES = ((0, "collab", ""), (1, "collab", "_single"), (2, "single", ""))
YAW = np.deg2rad(np.array([0, 90], dtype=np.float64))
DET = dict(pos_cls_weight=2.0, alpha=0.25, sigma=3.0, weights=(1.0, 2.0, 0.2), anchor_yaw=YAW, dir_offset=0.7853)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def criterion(fg=False, without_dir=False):
    hy = configs.lidar_pyramid()
    hy["loss"]["args"]["depth"]["use_fg_mask"] = bool(fg)
    if without_dir:
        del hy["loss"]["args"]["dir"]
    return create_loss(hy)


def run_module(crit, out, tgt, mode, suffix, dev, map_dtype, label_dtype, fused, scale=None):
    """One criterion call + backward on copies of the inputs -> (loss, [gradient | None per leaf], loss_dict, kernels timed)."""
    o = {"pyramid": mode}
    leafs = []

    def leaf(t):
        t = t.detach().to(device=dev, dtype=map_dtype).requires_grad_(True)
        leafs.append(t)
        return t
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        if k in out:
            o[k] = leaf(out[k])
    o["occ_single_list"] = [leaf(t) for t in out["occ_single_list"]]
    for k in out:
        if k.startswith("depth_items"):
            o[k] = (leaf(out[k][0]),) + tuple(t.to(dev) for t in out[k][1:])
    t = {k: v.to(device=dev, dtype=label_dtype) for k, v in tgt.items()}
    calls = {}
    with env("HEAL_LOSS_FUSED", fused):
        ops.TIMING = calls if dev != "cpu" else None
        try:
            loss = crit(o, t, suffix)
            (loss if scale is None else scale * loss).backward()
            if dev != "cpu":
                torch.cuda.synchronize()
        finally:
            ops.TIMING = None
    return loss.detach().cpu(), [None if x.grad is None else x.grad.detach().cpu() for x in leafs], dict(crit.loss_dict), sorted(calls)


def fp64(crit, out, tgt, mode, suffix):
    return run_module(crit, out, tgt, mode, suffix, "cpu", torch.float64, torch.float64, "0")[:3]


def check(tag, got, want):
    """got, want = (loss, gradients): the issue's bounds, every figure printed before it is asserted."""
    (la, ga), (lb, gb) = got, want
    la, lb = float(la), float(lb)
    e_loss = abs(la - lb) / abs(lb) if lb != 0 else abs(la)
    print(f"{tag}: loss {la:.9e} (expected {lb:.9e}), relative error {e_loss:.3e}")
    errs = []
    assert len(ga) == len(gb)
    for k, (x, y) in enumerate(zip(ga, gb)):
        assert (x is None) == (y is None), (tag, k)
        if x is None:
            continue
        y = torch.as_tensor(y).double()
        assert x.shape == y.shape and bool(torch.isfinite(x).all()), (tag, k)
        top = float(y.abs().max())
        e = float((x.double() - y).abs().max()) / top if top > 0 else float(x.abs().max())
        print(f"{tag}: gradient {k} {tuple(x.shape)}: error {e:.3e} of the largest magnitude {top:.3e}")
        errs.append((k, e))
    assert np.isfinite(la) and e_loss <= TOL, (tag, e_loss)
    for k, e in errs:
        assert e <= TOL, (tag, k, e)


def check_dict(tag, got, want):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in got:
        a, b = float(got[k]), float(want[k])
        assert isinstance(got[k], float) or k == "depth_loss", (tag, k, type(got[k]))
        assert abs(a - b) <= TOL * abs(b), (tag, k, a, b)


def timed(calls, prefix):
    return any(c.startswith(prefix) for c in calls)


# ---------------------------------------------------------------------------------------------------- 1. the reference's golden
@pytest.mark.parametrize("fg", [0, 1])
def test_loss_classes_match_reference_golden_on_the_kernels(fg):
    g = np.load(os.path.join(GOLD, "loss.npz"))
    crit = criterion(fg)
    for seed, mode, suffix in CASES:
        out, tgt = _loss_inputs(seed)
        tag = f"fg{fg}_s{seed}"
        loss, grads, ldict, calls = run_module(crit, out, tgt, mode, suffix, DEV, torch.float32, torch.float32, "1")
        want_grads = [g[f"{tag}_grad{k}"] if f"{tag}_grad{k}" in g.files else None for k in range(len(grads))]
        check(f"golden {tag} {mode}{suffix}", (loss, grads), (g[f"{tag}_loss"], want_grads))
        ref_loss, ref_grads, ref_dict = fp64(crit, out, tgt, mode, suffix)
        check(f"fp64 {tag}", (loss, grads), (ref_loss, ref_grads))
        check_dict(tag, ldict, ref_dict)
        want_kernels = {"det_loss": suffix == "", "depth_focal_loss": suffix == "", "occ_loss": not (mode == "collab" and suffix == "")}
        for name, want in want_kernels.items():
            assert timed(calls, name) == want, (tag, name, calls)
        _, off_grads, off_dict, off_calls = run_module(crit, out, tgt, mode, suffix, DEV, torch.float32, torch.float32, "0")
        assert not any(timed(off_calls, k) for k in KERNELS), off_calls
        check_dict(tag + " off", off_dict, ref_dict)


# ---------------------------------------------------------------------------------------------------- 2. tile edges, label types
def edge_inputs(n, H, W):
    """_loss_inputs at an odd size; sample 1 (if any) without a positive anchor, sample 2 (if any) with pos = neg = 0."""
    out, tgt = _loss_inputs(100 + n * H * W, n=n, H=H, W=W, with_depth=False)
    if n > 1:
        tgt["pos_equal_one"][1] = 0
    if n > 2:
        tgt["pos_equal_one"][2] = 0
        tgt["neg_equal_one"][2] = 0
    assert float(tgt["pos_equal_one"][0].sum()) > 0
    return out, tgt


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 8, 8), (2, 9, 15)], ids=lambda s: "x".join(map(str, s)))
def test_tile_edges_and_label_types_against_fp64(shape, label_dtype):
    crit = criterion()
    out, tgt = edge_inputs(*shape)
    loss, grads, ldict, calls = run_module(crit, out, tgt, "single", "", DEV, torch.float32, label_dtype, "1")
    assert timed(calls, "det_loss") and timed(calls, "occ_loss")
    ref_loss, ref_grads, ref_dict = fp64(crit, out, tgt, "single", "")
    check(f"edges {shape} {label_dtype}", (loss, grads), (ref_loss, ref_grads))
    check_dict(str(shape), ldict, ref_dict)
    assert float(ref_grads[1].abs().max()) > 0 and float(ref_grads[2].abs().max()) > 0


def depth_case(D, with_mask, seed=0):
    g = torch.Generator().manual_seed(1000 + D + seed)
    logit = torch.randn((4, D, 6, 8), generator=g) * 2.0
    idx = torch.randint(0, D, (4, 6, 8), generator=g)
    idx[1, 2, 3] = D                                         # one target index out of range
    idx[3, 5, 7] = -1
    mask = (torch.rand((4, 6, 8), generator=g) > 0.6).float() if with_mask else None
    return logit, idx, mask


def depth_fp64(logit, idx, mask, weight):
    """The composition (FocalLoss, the mask weights, mean, depth weight) in float64 with out-of-range pixels taken out."""
    D = logit.shape[1]
    x = logit.detach().double().cpu().requires_grad_(True)
    idx, valid = idx.cpu(), ((idx >= 0) & (idx < D)).cpu()
    per_pixel = FocalLoss(alpha=0.25, gamma=2.0, reduction="none")(x, idx.clamp(0, D - 1)) * valid
    if mask is not None:
        m = mask.cpu()
        per_pixel = per_pixel * ((m > 0) * 3.25 + (m == 0) * 0.25)
    loss = per_pixel.mean() * weight
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("D", [12, 48, 5])
def test_depth_focal_loss_against_fp64(D, with_mask):
    logit, idx, mask = depth_case(D, with_mask)
    dev = [t.to(DEV) if t is not None else None for t in (logit, idx, mask)]
    assert ops.depth_focal_loss_supported(*dev)
    loss, grad = ops.depth_focal_loss(*dev, alpha=0.25, weight=1.5)
    want_loss, want_grad = depth_fp64(logit, idx, mask, 1.5)
    check(f"depth D={D} mask={with_mask}", (loss.cpu(), [grad.cpu()]), (want_loss, [want_grad]))
    assert float(want_loss) > 1e-3
    # 3. exact zeros at the out-of-range pixels
    bits = grad.view(torch.int32)
    assert int(bits[1, :, 2, 3].abs().max()) == 0 and int(bits[3, :, 5, 7].abs().max()) == 0
    leaf = dev[0].clone().requires_grad_(True)
    term = ops.depth_focal_loss_term(leaf, dev[1], dev[2], alpha=0.25, weight=1.5)
    (3.0 * term).backward()
    assert torch.equal(term.detach().reshape(1), loss) and torch.equal(leaf.grad, 3.0 * grad)


# ---------------------------------------------------------------------------------------------------- ops-level inputs
@pytest.fixture(scope="module")
def dev_case():
    """(maps, labels f32, labels f64, occupancy maps) of a (3, 9, 15) problem on the device; read-only."""
    out, tgt = edge_inputs(3, 9, 15)
    maps = tuple(out[k].to(DEV) for k in ("cls_preds", "reg_preds", "dir_preds"))
    lab32 = tuple(tgt[k].to(DEV) for k in ("pos_equal_one", "neg_equal_one", "targets"))
    lab64 = tuple(t.double() for t in lab32)
    occ = [t.to(DEV) for t in out["occ_single_list"]]
    return maps, lab32, lab64, occ


OCC = dict(relative_downsample=[1, 2, 4], level_weight=[0.4, 0.2, 0.1], pos_cls_weight=2.0, alpha=0.25)


def zero_bits(t):
    return t.view(torch.int32) == 0


# ---------------------------------------------------------------------------------------------------- 3. exact zeros
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_exact_zeros_where_nothing_is_supervised(dev_case, f64):
    maps, lab32, lab64, _ = dev_case
    pos, neg, _ = lab32
    terms, (gc, gr, gd) = ops.det_loss(*maps, *(lab64 if f64 else lab32), **DET)
    N, A, H, W = maps[0].shape
    pos_m = pos.permute(0, 3, 1, 2) > 0                                         # [N, A, H, W]
    idle = (pos.permute(0, 3, 1, 2) == 0) & (neg.permute(0, 3, 1, 2) == 0)
    assert int(idle.sum()) > H * W * A and int(pos_m.sum()) > 0
    assert bool(zero_bits(gc)[idle].all())
    assert bool((gc != 0)[~idle].all())
    not_pos7 = ~pos_m.repeat_interleave(7, dim=1)
    not_pos2 = ~pos_m.repeat_interleave(2, dim=1)
    assert bool(zero_bits(gr)[not_pos7].all()) and bool(zero_bits(gd)[not_pos2].all())
    assert bool((gr != 0)[~not_pos7].all()) and bool((gd != 0)[~not_pos2].all())
    assert bool(torch.isfinite(terms).all()) and float(terms.min()) > 0


# ---------------------------------------------------------------------------------------------------- 4. bit-equal results
def shifted(x, words):
    """The same values `words` elements into a fresh allocation (4-B aligned only for fp32)."""
    buf = torch.empty(x.numel() + 64, dtype=x.dtype, device=DEV)
    view = buf[words:words + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + x.element_size() * words
    return view


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_bit_equal_across_launches_and_addresses(dev_case, f64):
    maps, lab32, lab64, occ = dev_case
    labels = lab64 if f64 else lab32
    a_terms, a_grads = ops.det_loss(*maps, *labels, **DET)
    b_terms, b_grads = ops.det_loss(*maps, *labels, **DET)
    assert torch.equal(a_terms, b_terms) and all(torch.equal(x, y) for x, y in zip(a_grads, b_grads))
    a_occ, a_og = ops.occ_loss(occ, labels[0], labels[1], **OCC)
    b_occ, b_og = ops.occ_loss(occ, labels[0], labels[1], **OCC)
    assert torch.equal(a_occ, b_occ) and all(torch.equal(x, y) for x, y in zip(a_og, b_og))
    logit, idx, mask = (t.to(DEV) for t in depth_case(48, True))
    a_d, a_dg = ops.depth_focal_loss(logit, idx, mask)
    b_d, b_dg = ops.depth_focal_loss(logit, idx, mask)
    assert torch.equal(a_d, b_d) and torch.equal(a_dg, b_dg)
    for wm, wl, wg in ((1, 3, 2), (2, 1, 3), (3, 2, 1)):
        sm = [shifted(m, wm + i) for i, m in enumerate(maps)]
        sl = [shifted(t, wl) for t in labels]
        bufs = [shifted(torch.zeros_like(m), wg) for m in maps]
        c_terms, c_grads = ops.det_loss(*sm, *sl, grad_out=bufs, **DET)
        assert torch.equal(a_terms, c_terms) and all(torch.equal(x, y) for x, y in zip(a_grads, c_grads))
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(bufs, c_grads))
        c_occ, c_og = ops.occ_loss([shifted(o, wm) for o in occ], sl[0], sl[1],
                                   grad_out=[shifted(torch.zeros_like(o), wg) for o in occ], **OCC)
        assert torch.equal(a_occ, c_occ) and all(torch.equal(x, y) for x, y in zip(a_og, c_og))
        c_d, c_dg = ops.depth_focal_loss(shifted(logit, wm), shifted(idx, wl), shifted(mask, wg),
                                         grad_out=shifted(torch.zeros_like(logit), wg))
        assert torch.equal(a_d, c_d) and torch.equal(a_dg, c_dg)


# ---------------------------------------------------------------------------------------------------- 5. saturation
@pytest.mark.parametrize("big", [80.0, 1.0e4])
def test_saturated_logits_stay_finite_and_within_the_bounds(big):
    crit = criterion(True)
    out, tgt = _loss_inputs(7, n=2, H=9, W=15)
    g = torch.Generator().manual_seed(int(big))
    sign = lambda t: (torch.randint(0, 2, t.shape, generator=g).float() * 2 - 1) * big      # noqa: E731
    out["cls_preds"] = sign(out["cls_preds"])
    out["occ_single_list"] = [sign(t) for t in out["occ_single_list"]]
    logit, idx, mask = out["depth_items_m2"]
    out["depth_items_m2"] = (torch.randint(0, 2, logit.shape, generator=g).float() * 1.0e4, idx, mask)
    loss, grads, ldict, calls = run_module(crit, out, tgt, "single", "", DEV, torch.float32, torch.float64, "1")
    assert all(timed(calls, k) for k in KERNELS)
    assert all(bool(torch.isfinite(x).all()) for x in grads) and bool(torch.isfinite(loss))
    ref_loss, ref_grads, ref_dict = fp64(crit, out, tgt, "single", "")
    check(f"saturation {big}", (loss, grads), (ref_loss, ref_grads))
    check_dict(f"saturation {big}", ldict, ref_dict)


# ---------------------------------------------------------------------------------------------------- 6. read-only mode
def test_without_gradient_the_kernels_only_read(dev_case):
    maps, lab32, _, occ = dev_case
    terms, _ = ops.det_loss(*maps, *lab32, **DET)
    poison = [torch.full_like(m, float("nan")) for m in maps]
    keep = [p.clone() for p in poison]
    ro_terms, ro_grads = ops.det_loss(*maps, *lab32, need_grad=False, grad_out=poison, **DET)
    assert ro_grads is None and torch.equal(ro_terms, terms)
    occ_loss, _ = ops.occ_loss(occ, lab32[0], lab32[1], **OCC)
    opoison = [torch.full_like(o, float("nan")) for o in occ]
    okeep = [p.clone() for p in opoison]
    ro_occ, ro_og = ops.occ_loss(occ, lab32[0], lab32[1], need_grad=False, grad_out=opoison, **OCC)
    assert ro_og is None and torch.equal(ro_occ, occ_loss)
    logit, idx, mask = (t.to(DEV) for t in depth_case(12, True))
    d_loss, _ = ops.depth_focal_loss(logit, idx, mask)
    dpoison = torch.full_like(logit, float("nan"))
    dkeep = dpoison.clone()
    ro_d, ro_dg = ops.depth_focal_loss(logit, idx, mask, need_grad=False, grad_out=dpoison)
    torch.cuda.synchronize()
    assert ro_dg is None and torch.equal(ro_d, d_loss)
    for p, k in zip(poison + opoison + [dpoison], keep + okeep + [dkeep]):
        assert torch.equal(p.view(torch.int32), k.view(torch.int32))
    leafs = [m.clone().requires_grad_(True) for m in maps]
    with torch.no_grad():
        assert torch.equal(ops.det_loss_terms(*leafs, *lab32, **DET), terms)
        assert torch.equal(ops.occ_loss_term([o.clone().requires_grad_(True) for o in occ], lab32[0], lab32[1], **OCC).reshape(1),
                           occ_loss)
        assert torch.equal(ops.depth_focal_loss_term(logit.clone().requires_grad_(True), idx, mask).reshape(1), d_loss)
    # a gradient for one map only
    only_reg = ops.det_loss(*maps, *lab32, need_grad=(False, True, False), **DET)[1]
    assert only_reg[0] is None and only_reg[2] is None and only_reg[1] is not None


# ---------------------------------------------------------------------------------------------------- 7. strided head maps
def test_non_contiguous_head_maps_give_the_same_bits(dev_case):
    maps, _, lab64, occ = dev_case
    want_terms, want_grads = ops.det_loss(*maps, *lab64, **DET)

    def channel_slice(m):
        wide = torch.zeros((m.shape[0], m.shape[1] + 3) + tuple(m.shape[2:]), device=DEV)
        wide[:, 2:2 + m.shape[1]] = m
        view = wide[:, 2:2 + m.shape[1]]
        assert not view.is_contiguous()
        return view
    sliced = [channel_slice(m) for m in maps]
    assert ops.det_loss_supported(*sliced, *lab64)
    terms, grads = ops.det_loss(*sliced, *lab64, **DET)
    assert torch.equal(terms, want_terms) and all(torch.equal(x, y) for x, y in zip(grads, want_grads))
    leafs = [s.clone(memory_format=torch.preserve_format).requires_grad_(True) for s in sliced]
    ops.det_loss_terms(*leafs, *lab64, **DET).sum().backward()
    assert all(torch.equal(x.grad, y) for x, y in zip(leafs, want_grads))
    want_occ, want_og = ops.occ_loss(occ, lab64[0], lab64[1], **OCC)
    occ_cl = [torch.zeros((o.shape[0], 2) + tuple(o.shape[2:]), device=DEV) for o in occ]
    for wide, o in zip(occ_cl, occ):
        wide[:, 1:2] = o
    got_occ, got_og = ops.occ_loss([w[:, 1:2] for w in occ_cl], lab64[0], lab64[1], **OCC)
    assert torch.equal(got_occ, want_occ) and all(torch.equal(x, y) for x, y in zip(got_og, want_og))


# ---------------------------------------------------------------------------------------------------- 8. scaled backward
def test_backward_scales_the_saved_gradients_and_dir_is_optional():
    out, tgt = _loss_inputs(3, n=2, H=9, W=15)
    crit = criterion(True)
    _, grads, _, _ = run_module(crit, out, tgt, "single", "", DEV, torch.float32, torch.float64, "1")
    _, grads3, _, calls = run_module(crit, out, tgt, "single", "", DEV, torch.float32, torch.float64, "1", scale=3.0)
    assert all(timed(calls, k) for k in KERNELS)
    for x, y in zip(grads, grads3):
        assert torch.equal(3.0 * x, y) and float(x.abs().max()) > 0
    plain = criterion(True, without_dir=True)
    loss, g_nodir, ldict, calls = run_module(plain, out, tgt, "single", "", DEV, torch.float32, torch.float64, "1")
    assert timed(calls, "det_loss") and "dir_loss" not in ldict
    assert g_nodir[2] is None and g_nodir[0] is not None and g_nodir[1] is not None
    ref_loss, ref_grads, ref_dict = fp64(plain, out, tgt, "single", "")
    check("no dir block", (loss, g_nodir), (ref_loss, ref_grads))
    check_dict("no dir block", ldict, ref_dict)


# ---------------------------------------------------------------------------------------------------- 9. through a model
class _SmallHeads(torch.nn.Module):
    """1x1 convolutions from a fixed 8-channel input to the three heads, three occupancy levels and a depth head."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(11)
        self.cls_head, self.reg_head, self.dir_head = torch.nn.Conv2d(8, 2, 1), torch.nn.Conv2d(8, 14, 1), torch.nn.Conv2d(8, 4, 1)
        self.occ_head, self.depth_head = torch.nn.Conv2d(8, 1, 1), torch.nn.Conv2d(8, 12, 1)

    def forward(self, x, cam, depth_gt):
        occ = self.occ_head(x)
        return {"cls_preds": self.cls_head(x), "reg_preds": self.reg_head(x) * 0.3, "dir_preds": self.dir_head(x),
                "occ_single_list": [occ, torch.nn.functional.avg_pool2d(occ, 2), torch.nn.functional.avg_pool2d(occ, 4)],
                "depth_items_m2": (self.depth_head(cam),) + depth_gt, "pyramid": "collab"}


def test_fused_and_unfused_agree_through_a_model_with_single_supervision():
    gen = torch.Generator().manual_seed(21)
    x = torch.randn((2, 8, 9, 15), generator=gen).to(DEV)
    cam = torch.randn((8, 8, 6, 8), generator=gen).to(DEV)
    _, tgt = _loss_inputs(5, n=2, H=9, W=15)
    depth_gt = tuple(t.to(DEV) for t in depth_case(12, True)[1:])
    depth_gt = (depth_gt[0].clamp(0, 11).repeat(2, 1, 1), depth_gt[1].repeat(2, 1, 1))
    results = {}
    for fused in ("1", "0"):
        model, crit = _SmallHeads().to(DEV), criterion(True)
        labels = {k: v.double().to(DEV) for k, v in tgt.items()}
        with env("HEAL_LOSS_FUSED", fused):
            calls = {}
            ops.TIMING = calls
            try:
                out = model(x, cam, depth_gt)
                total = crit(out, labels)
                first = dict(crit.loss_dict)
                total = total + crit(out, labels, suffix="_single")
                total.backward()
                torch.cuda.synchronize()
            finally:
                ops.TIMING = None
        assert all(timed(calls, k) == (fused == "1") for k in KERNELS), calls
        results[fused] = (float(total.detach()), first, dict(crit.loss_dict), {n: p.grad.clone() for n, p in model.named_parameters()})
    (ta, fa, sa, ga), (tb, fb, sb, gb) = results["1"], results["0"]
    print(f"model: fused total {ta!r}, composition {tb!r}")
    assert abs(ta - tb) <= TOL * abs(tb)
    check_dict("fused heads", fa, fb)
    check_dict("single pass", sa, sb)
    for name, want in gb.items():
        e = float((ga[name] - want).abs().max()) / float(want.abs().max())
        print(f"model: {name} gradient error {e:.3e}")
        assert e <= TOL, (name, e)
    assert all(float(v.abs().max()) > 0 for v in gb.values())
