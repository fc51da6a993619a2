"""heal_unc_loss on the MI355X: PointPillarUncertaintyLoss's four terms and the gradients of the four head maps in one pass,
through the loss class and through ops, against the torch composition evaluated on the CPU in float64 (pinned to the
reference by tests/test_unc_cpu.py, not under test here) and against the reference's recorded values (tests/golden/unc_loss.npz).

Bounds, the project's for loss kernels (tests/test_gpu_det_loss.py, tests/test_gpu_kd.py): loss and every term within 1e-5
relative, every gradient tensor within 1e-5 x the largest magnitude of the expected tensor.  The composition in float32 sits at
<= 1.7e-7 (loss) and <= 6.5e-7 (gradients) from its float64 form on inputs like these (s in [-4, 4], ~520 anchors, 8 %
positives, all five configurations), so the reference's own arithmetic is about 15 x inside the bar."""
import contextlib
import os

import numpy as np
import pytest
import torch

from heal_amd import configs, ops
from heal_amd.opencood.loss import point_pillar_uncertainty_loss as ul
from heal_amd.opencood.tools import train_utils
from oracle import cref
from tests.golden import unc_cases as U
from tests.golden.detfill import fill_module

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5
MAPS = ("cls_preds", "reg_preds", "unc_preds", "dir_preds")
LABELS = ("pos_equal_one", "neg_equal_one", "targets")
YAW = np.deg2rad(np.array([0, 90], dtype=np.float64))


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


def criterion(tag, with_dir=None, weight=None):
    args = U.loss_args(tag, weight)
    if with_dir is False:
        args.pop("dir", None)
    return ul.PointPillarUncertaintyLoss(args)


def run_module(crit, out, tgt, dev, map_dtype, label_dtype, fused, scale=None):
    """One criterion call + backward on copies of the inputs -> (loss, [gradient per map present], loss_dict, kernels timed)."""
    leafs = {k: out[k].detach().to(device=dev, dtype=map_dtype).requires_grad_(True) for k in MAPS
             if k in out and (k != "dir_preds" or crit.dir)}
    t = {k: v.to(device=dev, dtype=label_dtype) for k, v in tgt.items()}
    calls = {}
    with env("HEAL_LOSS_FUSED", fused):
        ops.TIMING = calls if dev != "cpu" else None
        try:
            loss = crit(dict(leafs), t)
            (loss if scale is None else scale * loss).backward()
            if dev != "cpu":
                torch.cuda.synchronize()
        finally:
            ops.TIMING = None
    return loss.detach().cpu(), [x.grad.detach().cpu() for x in leafs.values()], dict(crit.loss_dict), sorted(calls)


def fp64(crit, out, tgt):
    return run_module(crit, out, tgt, "cpu", torch.float64, torch.float64, "0")[:3]


def check(tag, got, want):
    """got, want = (loss, gradients): the bounds above, every figure printed before it is asserted."""
    (la, ga), (lb, gb) = got, want
    la, lb = float(la), float(lb)
    e_loss = abs(la - lb) / abs(lb) if lb != 0 else abs(la)
    print(f"{tag}: loss {la:.9e} (expected {lb:.9e}), relative error {e_loss:.3e}")
    errs = []
    assert len(ga) == len(gb)
    for k, (x, y) in enumerate(zip(ga, gb)):
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
        assert isinstance(got[k], float), (tag, k, type(got[k]))
        print(f"{tag}: {k} {a:.9e} (expected {b:.9e})")
        assert abs(a - b) <= TOL * abs(b), (tag, k, a, b)


def timed(calls, prefix):
    return any(c.startswith(prefix) for c in calls)


def edge_inputs(n, H, W, dim, A=2):
    """Seeded inputs at an odd size with 15 % positives; the second sample (if any) without a positive anchor."""
    out, tgt = U.loss_inputs(700 + n * H * W + dim + A, n, H, W, dim, A=A, positives=0.15)
    if n > 1:
        tgt["pos_equal_one"][1] = 0
    assert float(tgt["pos_equal_one"][0].sum()) > 0
    return out, tgt


def unc_part_of_grad_reg(tag, with_dir, out, tgt, ref_grads):
    """The float64 composition's grad_reg minus the one of the same criterion with uncertainty.weight = 0."""
    _, g0, _ = fp64(criterion(tag, with_dir, weight=0.0), out, tgt)
    return ref_grads[1] - g0[1]


# ---------------------------------------------------------------------------------------------------- 1. tile edges, label types
# (3, 5, 7): one ragged tile; (1, 8, 8): exactly one tile; (2, 9, 15): two full tiles + a 7-pixel tail; (1, 17, 16): five tiles,
# so the second block has one tile
SHAPES = [(3, 5, 7), (1, 8, 8), (2, 9, 15), (1, 17, 16)]


def edge_case(tag, shape, label_dtype, A):
    dim, with_dir = U.CONFIGS[tag][0], U.CONFIGS[tag][4] and A == 2
    crit = criterion(tag, with_dir)
    out, tgt = edge_inputs(*shape, dim, A=A)
    loss, grads, ldict, calls = run_module(crit, out, tgt, DEV, torch.float32, label_dtype, "1")
    assert timed(calls, f"unc_loss_a{A}_d{dim}"), calls
    ref_loss, ref_grads, ref_dict = fp64(crit, out, tgt)
    name = f"{tag} {shape} A={A} {label_dtype}"
    check(name, (loss, grads), (ref_loss, ref_grads))
    check_dict(name, ldict, ref_dict)
    assert float(ref_grads[2].abs().max()) > 0                                  # a kernel that skips the term fails
    assert float(unc_part_of_grad_reg(tag, with_dir, out, tgt, ref_grads).abs().max()) > 0
    if shape[0] > 1:                                                            # the sample without positives: exact zeros
        for k in (1, 2) + ((3,) if with_dir else ()):
            assert int(grads[k][1].view(torch.int32).abs().max()) == 0, (name, k)
        assert float(grads[0][1].abs().max()) > 0                               # its negatives still count (normaliser 1)


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("tag", list(U.CONFIGS))
def test_tile_edges_and_label_types_against_fp64(tag, shape, label_dtype):
    edge_case(tag, shape, label_dtype, 2)


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 9, 15)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("tag", list(U.CONFIGS))
def test_one_and_four_anchors_without_a_direction_map(tag, shape, A):
    edge_case(tag, shape, torch.float64, A)


# ---------------------------------------------------------------------------------------------------- 2. the reference's golden
@pytest.mark.parametrize("tag", list(U.CONFIGS))
def test_loss_class_matches_the_reference_recording_on_the_kernel(tag):
    g = np.load(os.path.join(GOLD, "unc_loss.npz"))
    crit = criterion(tag)
    out = {k: torch.from_numpy(g[f"{tag}_{k}"]) for k in MAPS if f"{tag}_{k}" in g.files}
    tgt = {k: torch.from_numpy(g[f"{tag}_{k}"]) for k in LABELS}
    loss, grads, ldict, calls = run_module(crit, out, tgt, DEV, torch.float32, torch.float32, "1")
    assert timed(calls, "unc_loss"), calls
    check(f"golden {tag}", (loss, grads), (g[f"{tag}_total_loss"], [g[f"{tag}_grad_{k}"] for k in out]))
    check_dict(f"golden {tag}", ldict, {k: g[f"{tag}_{k}"] for k in ldict})
    # 4. ... and the switch: no kernel, the same values
    off_loss, off_grads, off_dict, off_calls = run_module(crit, out, tgt, DEV, torch.float32, torch.float32, "0")
    assert not timed(off_calls, "unc_loss") and not timed(off_calls, "det_loss"), off_calls
    check_dict(f"golden {tag} off", off_dict, {k: g[f"{tag}_{k}"] for k in off_dict})
    check(f"golden {tag} off", (off_loss, off_grads), (g[f"{tag}_total_loss"], [g[f"{tag}_grad_{k}"] for k in out]))


# ---------------------------------------------------------------------------------------------------- ops-level inputs
def cfg_for(tag, with_dir, unc_weight=0.25):
    dim, xy, angle, limit, _ = U.CONFIGS[tag]
    return dict(pos_cls_weight=2.0, alpha=0.25, sigma=3.0, weights=(1.0, 2.0, unc_weight, 0.2 if with_dir else 0.0), dim=dim,
                xy_loss_type=xy, angle_loss_type=angle, angle_weight=0.5, lambda_V=0.001, s0=1.0, limit_period=limit,
                anchor_yaw=YAW if with_dir else None, dir_offset=0.7853)


def dev_inputs(tag, shape=(3, 9, 15), A=2, f64=False, with_dir=True):
    out, tgt = edge_inputs(*shape, U.CONFIGS[tag][0], A=A)
    maps = [out[k].to(DEV) for k in MAPS]
    if not with_dir:
        maps[3] = None
    labels = [tgt[k].to(DEV).double() if f64 else tgt[k].to(DEV) for k in LABELS]
    return maps, labels


# ---------------------------------------------------------------------------------------------------- 3. bit-equal to det_loss
@pytest.mark.parametrize("A,with_dir", [(2, True), (4, False), (1, False)])
@pytest.mark.parametrize("tag", ["d3_vm_lp", "d7", "d3_l1_l2"])
def test_cls_reg_dir_are_bit_equal_to_det_loss(tag, A, with_dir):
    maps, labels = dev_inputs(tag, A=A, f64=True, with_dir=with_dir)
    cls, reg, unc, dirp = maps
    det = dict(pos_cls_weight=2.0, alpha=0.25, sigma=3.0, weights=(1.0, 2.0, 0.2 if with_dir else 0.0),
               anchor_yaw=YAW if with_dir else None, dir_offset=0.7853)
    d_terms, d_grads = ops.det_loss(cls, reg, dirp, *labels, **det)
    terms, grads = ops.unc_loss(cls, reg, unc, dirp, *labels, **cfg_for(tag, with_dir))
    assert torch.equal(terms[0], d_terms[0]) and torch.equal(terms[1], d_terms[1]) and torch.equal(terms[3], d_terms[2])
    assert torch.equal(grads[0], d_grads[0]) and float(terms[2]) != 0
    assert not torch.equal(grads[1], d_grads[1])                                 # the unc term's share is in grad_reg
    if with_dir:
        assert torch.equal(grads[3], d_grads[2])
    z_terms, z_grads = ops.unc_loss(cls, reg, unc, dirp, *labels, **cfg_for(tag, with_dir, unc_weight=0.0))
    assert torch.equal(z_grads[1], d_grads[1]) and torch.equal(z_grads[0], d_grads[0]) and float(z_terms[2]) == 0
    assert float(z_grads[2].abs().max()) == 0


# ---------------------------------------------------------------------------------------------------- 5. bit-equal results
def shifted(x, words):
    """The same values `words` elements into a fresh allocation (4-B aligned only for fp32)."""
    buf = torch.empty(x.numel() + 64, dtype=x.dtype, device=DEV)
    view = buf[words:words + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + x.element_size() * words
    return view


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_bit_equal_across_launches_and_addresses(f64):
    maps, labels = dev_inputs("d3_vm_lp", f64=f64)
    cfg = cfg_for("d3_vm_lp", True)
    a_terms, a_grads = ops.unc_loss(*maps, *labels, **cfg)
    b_terms, b_grads = ops.unc_loss(*maps, *labels, **cfg)
    assert torch.equal(a_terms, b_terms) and all(torch.equal(x, y) for x, y in zip(a_grads, b_grads))
    for wm, wl, wg in ((1, 3, 2), (2, 1, 3), (3, 2, 1)):
        sm = [shifted(m, wm + i) for i, m in enumerate(maps)]
        sl = [shifted(t, wl) for t in labels]
        bufs = [shifted(torch.zeros_like(m), wg) for m in maps]
        c_terms, c_grads = ops.unc_loss(*sm, *sl, grad_out=bufs, **cfg)
        assert torch.equal(a_terms, c_terms) and all(torch.equal(x, y) for x, y in zip(a_grads, c_grads))
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(bufs, c_grads))


# ---------------------------------------------------------------------------------------------------- 6. read-only mode
def test_without_gradient_the_kernels_only_read():
    maps, labels = dev_inputs("d7")
    cfg = cfg_for("d7", True)
    terms, _ = ops.unc_loss(*maps, *labels, **cfg)
    poison = [torch.full_like(m, float("nan")) for m in maps]
    keep = [p.clone() for p in poison]
    ro_terms, ro_grads = ops.unc_loss(*maps, *labels, need_grad=False, grad_out=poison, **cfg)
    torch.cuda.synchronize()
    assert ro_grads is None and torch.equal(ro_terms, terms)
    for p, k in zip(poison, keep):
        assert torch.equal(p.view(torch.int32), k.view(torch.int32))
    leafs = [m.clone().requires_grad_(True) for m in maps]
    with torch.no_grad():
        total, t2 = ops.unc_loss_terms(*leafs, *labels, **cfg)
    assert torch.equal(t2, terms) and not total.requires_grad
    only_unc = ops.unc_loss(*maps, *labels, need_grad=(False, False, True, False), **cfg)[1]
    assert only_unc[0] is None and only_unc[1] is None and only_unc[3] is None and only_unc[2] is not None


# ---------------------------------------------------------------------------------------------------- 7. strided head maps
def test_non_contiguous_head_maps_give_the_same_bits():
    maps, labels = dev_inputs("d3_vm", f64=True)
    cfg = cfg_for("d3_vm", True)
    want_terms, want_grads = ops.unc_loss(*maps, *labels, **cfg)

    def channel_slice(m):
        wide = torch.zeros((m.shape[0], m.shape[1] + 3) + tuple(m.shape[2:]), device=DEV)
        wide[:, 2:2 + m.shape[1]] = m
        view = wide[:, 2:2 + m.shape[1]]
        assert not view.is_contiguous()
        return view
    sliced = [channel_slice(m) for m in maps]
    assert ops.unc_loss_supported(*sliced, *labels, 3, xy_loss_type="l2", angle_loss_type="von-mise")
    terms, grads = ops.unc_loss(*sliced, *labels, **cfg)
    assert torch.equal(terms, want_terms) and all(torch.equal(x, y) for x, y in zip(grads, want_grads))
    leafs = [s.clone(memory_format=torch.preserve_format).requires_grad_(True) for s in sliced]
    total, _ = ops.unc_loss_terms(*leafs, *labels, **cfg)
    (3.0 * total).backward()
    assert all(torch.equal(x.grad, 3.0 * y) for x, y in zip(leafs, want_grads))


# ---------------------------------------------------------------------------------------------------- 8. extreme values
@pytest.mark.parametrize("tag", ["d3_vm_lp", "d3_vm", "d7"])
def test_extreme_s_stays_finite_where_the_reference_overflows(tag, monkeypatch):
    """s = +-30 at the positives: kappa = exp(30) overflows the reference's log(i0e(kappa) exp(kappa)) in float32 AND float64;
    the expected values are the float64 composition with log I0 written as log(i0e(kappa)) + kappa.  s = +-1e4 at the other
    anchors: they carry no weight, so exact zeros (the composition itself gives inf * 0 there and is evaluated without them)."""
    dim, with_dir = U.CONFIGS[tag][0], U.CONFIGS[tag][4]
    out, tgt = edge_inputs(2, 9, 15, dim)
    pos = tgt["pos_equal_one"].permute(0, 3, 1, 2).repeat_interleave(dim, dim=1) > 0          # [N, dim * A, H, W]
    g = torch.Generator().manual_seed(3)
    sign = torch.randint(0, 2, out["unc_preds"].shape, generator=g).float() * 2 - 1
    out["unc_preds"] = torch.where(pos, 30.0 * sign, 1.0e4 * sign)
    crit = criterion(tag)
    loss, grads, ldict, calls = run_module(crit, out, tgt, DEV, torch.float32, torch.float64, "1")
    assert timed(calls, "unc_loss") and bool(torch.isfinite(loss)) and all(bool(torch.isfinite(x).all()) for x in grads)
    assert int(grads[2][~pos].view(torch.int32).abs().max()) == 0
    monkeypatch.setattr(ul, "log_i0", lambda k: torch.log(torch.special.i0e(k)) + k)
    ref_out = dict(out, unc_preds=torch.where(pos, out["unc_preds"], torch.zeros(())))
    ref_loss, ref_grads, ref_dict = fp64(crit, ref_out, tgt)
    assert bool(torch.isfinite(ref_loss)) and float(ref_grads[2][~pos].abs().max()) == 0
    check(f"extreme {tag}", (loss, grads), (ref_loss, ref_grads))
    check_dict(f"extreme {tag}", ldict, ref_dict)


# ---------------------------------------------------------------------------------------------------- 9. through the model
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]


def test_one_training_step_fused_and_unfused_agree():
    """Loss and loss_dict at the bar; every parameter gradient within 1e-5 of its largest magnitude, the bound of
    test_fused_and_unfused_agree_through_a_model_with_single_supervision (tests/test_gpu_det_loss.py).  Measured on an MI355X:
    heads <= 3.4e-7, trunk <= 6.1e-6 -- and two backward passes of the SAME criterion through this trunk differ by 4.8e-6
    (kernel path) and 5.4e-6 (composition): the trunk figures are the gradient path's own run-to-run spread, not the criterion's."""
    from heal_amd import synth
    hypes = configs.lidar_uncertainty(M_RANGE)
    parts = []
    for b, seed in enumerate((191, 192)):
        pts = synth.lidar_frame(seed)
        near = (np.abs(pts[:, 0]) < M_RANGE[3] + 2) & (np.abs(pts[:, 1]) < M_RANGE[4] + 2)
        parts.append(cref.voxelize(pts[near][:1000], M_RANGE, (0.4, 0.4, 4), 32, 70000, batch_idx=b))
    lidar = {"voxel_features": torch.from_numpy(np.concatenate([p[0] for p in parts])).to(DEV),
             "voxel_coords": torch.from_numpy(np.concatenate([p[1] for p in parts])).to(torch.int32).to(DEV),
             "voxel_num_points": torch.from_numpy(np.concatenate([p[2] for p in parts])).to(torch.int32).to(DEV)}
    _, tgt = U.loss_inputs(77, 2, 32, 32, 3, positives=0.03)
    labels = {k: v.double().to(DEV) for k, v in tgt.items()}
    model = fill_module(train_utils.create_model(hypes)).to(DEV).train()
    with torch.no_grad():                          # s stays where the composition's own log(i0e(k) exp(k)) is finite in float32
        model.unc_head.weight.mul_(0.05)
        model.unc_head.bias.zero_()
    crit = train_utils.create_loss(hypes)
    # ONE forward, both criteria on its head maps: two training-mode forwards of the trunk are not bit-equal to each other,
    # which is not what is compared here
    out = model({"processed_lidar": lidar})
    assert tuple(out["unc_preds"].shape) == (2, 6, 32, 32) and tuple(out["cls_preds"].shape) == (2, 2, 32, 32)
    results = {}
    for fused in ("1", "0"):
        model.zero_grad()
        with env("HEAL_LOSS_FUSED", fused):
            calls = {}
            ops.TIMING = calls
            try:
                total = crit(dict(out), labels)
                total.backward(retain_graph=True)
                torch.cuda.synchronize()
            finally:
                ops.TIMING = None
        assert timed(calls, "unc_loss") == (fused == "1"), calls
        results[fused] = (float(total.detach()), dict(crit.loss_dict),
                          {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    (ta, da, ga), (tb, db, gb) = results["1"], results["0"]
    print(f"model: fused total {ta!r}, composition {tb!r}")
    assert abs(ta - tb) <= TOL * abs(tb)
    check_dict("model", da, db)
    assert set(ga) == set(gb) and "unc_head.weight" in gb
    for name, want in gb.items():
        e = float((ga[name] - want).abs().max()) / float(want.abs().max())
        print(f"model: {name} gradient error {e:.3e}")
        assert e <= TOL, (name, e)
    assert all(float(v.abs().max()) > 0 for v in gb.values())
