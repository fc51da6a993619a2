"""The restatement of tests/warp_refs.py proved on the CPU, and the host side of the differentiable warp
(include/heal_amd_train_warp.h): float64 autograd of F.grid_sample, the candidate box of heal_warp_affine_window against the
brute-force contributor sets, the accept / refuse table of heal_warp_affine_backward_supported, the header's signatures, ops.warp_grad
and the routing of the gradient-path warps on CPU tensors.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, ops
from heal_amd.opencood.models.fuse_modules import fusion_in_one as fio
from tests import warp_refs as R

MAX_AGENTS = _capi.header_define("HEAL_WARP_MAX_AGENTS")


def _window(row, H, W):
    out = (ctypes.c_double * 8)()
    row = np.ascontiguousarray(row, dtype=np.float64)
    _capi.call("heal_warp_affine_window", row.ctypes.data_as(ctypes.c_void_p), H, W, ctypes.cast(out, ctypes.c_void_p))
    return list(out)


def _supported(rows, n, H, W):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    return int(_capi.lib().heal_warp_affine_backward_supported(rows.ctypes.data_as(ctypes.c_void_p), n, H, W))


def _cpu_fixtures():
    """(name, H, W, rows): the fixed rows on a 12 x 20 map and 200 seeded random rigid rows on 13 x 21 and 32 x 48."""
    rows = R.named_rows(12, 20)
    out = [(k, 12, 20, rows[k][None]) for k in ("identity", "rot90", "rot180", "rot37", "shift", "scale075", "scale150")]
    out.append(("random13x21", 13, 21, R.random_rigid(200, 13, 21, 1, 0.5)))
    out.append(("random32x48", 32, 48, R.random_rigid(200, 32, 48, 2, 0.5)))
    return out


@pytest.mark.grad
@pytest.mark.parametrize("f64", [True, False])
def test_restated_adjoint_equals_float64_autograd(f64):
    for name, (H, W, C, rows) in R.gpu_fixtures().items():
        Rs = R.Restated(rows, H, W, f64)
        G = R.fixture_grad(name, len(rows), min(C, 3), H, W)
        assert R.check_against_autograd(Rs, G) <= 1e-12, name
        # and the forward of the same taps against float64 grid_sample: the restatement is the adjoint of THAT map
        x = torch.randn(len(rows), 2, H, W, dtype=torch.float64)
        grid = torch.stack([(2.0 * Rs.ix + 1.0) / W - 1.0, (2.0 * Rs.iy + 1.0) / H - 1.0], dim=-1).reshape(len(rows), H, W, 2)
        assert (Rs.forward(x) - F.grid_sample(x, grid, align_corners=False)).abs().max() <= 1e-12, name


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("fixture", _cpu_fixtures(), ids=lambda f: f[0])
def test_window_contains_every_contributor(fixture, f64):
    name, H, W, rows = fixture
    Rs = R.Restated(rows, H, W, f64)
    most = 0
    for a in range(len(rows)):
        win = _window(rows[a], H, W)
        assert R.window_violations(Rs, a, win) == 0, (name, a, rows[a])
        most = max(most, Rs.max_contributors(a))
        rigid_row = not name.startswith("scale")
        if rigid_row:       # a rigid row reaches at most sqrt(2) (+ the margin) per axis: at most 4 x 4 candidates
            margin = 0.01 + 2.0 ** -20 * max(H, W)
            assert win[6] <= 2 ** 0.5 + margin + 1e-12 and win[7] <= 2 ** 0.5 + margin + 1e-12
            assert Rs.max_contributors(a) <= 16      # (5 with non-zero weight; fp32 positions add taps of weight ~1e-7)
    assert most >= 1


def test_window_is_the_inverse_pixel_map():
    """Ainv and b of heal_warp_affine_window invert the positions the restatement samples at (to fp32 rounding)."""
    H, W = 13, 21
    row = R.named_rows(H, W)["rot37"]
    win = _window(row, H, W)
    ix, iy = (t.double() for t in R.positions(row[None], H, W, True))
    h, w = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ex, ey = ix[0] - win[4], iy[0] - win[5]
    assert (win[0] * ex + win[1] * ey - w).abs().max() < 1e-4 and (win[2] * ex + win[3] * ey - h).abs().max() < 1e-4


def test_supported_accepts_and_refuses():
    H, W = 12, 20
    rows = R.named_rows(H, W)
    for k in ("identity", "rot90", "rot180", "rot37", "shift", "scale075", "scale150", "outside"):
        assert _supported(rows[k], 1, H, W) == 1, k
    assert _supported(np.stack([rows["identity"]] * MAX_AGENTS), MAX_AGENTS, H, W) == 1
    assert _supported(R.rigid(10, 0, 0, H, W, 0.2), 1, H, W) == 0                 # reach sqrt(2) / 0.2 > 4
    assert _supported(R.rigid(0, 0, 0, H, W, 0.26), 1, H, W) == 1                 # reach 1 / 0.26 < 4
    assert _supported(np.zeros(6), 1, H, W) == 0                                  # a padded agent's all-zero row: singular
    for bad in (np.nan, np.inf):
        r = rows["rot37"].copy()
        r[2] = bad
        assert _supported(r, 1, H, W) == 0
    assert _supported(np.stack([rows["identity"], np.zeros(6)]), 2, H, W) == 0    # one bad row refuses the launch
    assert _supported(rows["identity"], 0, H, W) == 0
    assert _supported(np.stack([rows["identity"]] * (MAX_AGENTS + 1)), MAX_AGENTS + 1, H, W) == 0
    assert _supported(rows["identity"], 1, 0, W) == 0 and _supported(rows["identity"], 1, H, 0) == 0
    assert _supported(rows["identity"], 1, 1 << 16, 1 << 15) == 0                 # H * W beyond the index range
    with pytest.raises(_capi.HealAmdError, match="singular"):
        _window(np.zeros(6), H, W)
    with pytest.raises(_capi.HealAmdError, match="REACH"):
        _window(R.rigid(10, 0, 0, H, W, 0.2), H, W)


def test_header_signatures_load():
    sig = _capi.signatures_train_warp()
    assert sorted(sig) == ["heal_warp_affine_backward", "heal_warp_affine_backward_supported", "heal_warp_affine_forward",
                           "heal_warp_affine_window"]
    assert len(sig["heal_warp_affine_forward"][1]) == 10 and len(sig["heal_warp_affine_backward"][1]) == 9
    assert all(res is ctypes.c_int for res, _ in sig.values())
    assert not set(sig) & set(_capi.declared_symbols())          # outside the versioned inference ABI
    L = _capi.lib()
    for name, (res, args) in sig.items():
        assert hasattr(L, name) and getattr(L, name).argtypes == args, name
    from heal_amd import build
    assert any(p.endswith("heal_amd_train_warp.h") for p in build._deps())


def test_warp_grad_setter_and_context():
    assert not ops.warp_grad_enabled()                            # the default is "torch"
    with pytest.raises(ValueError):
        ops.warp_grad("hip")
    assert not ops.warp_grad_enabled()
    with ops.warp_grad("kernel"):
        assert ops.warp_grad_enabled()
        with ops.warp_grad("torch"):
            assert not ops.warp_grad_enabled()
        assert ops.warp_grad_enabled()
    assert not ops.warp_grad_enabled()
    s = ops.warp_grad("kernel")                                   # a plain setter
    assert ops.warp_grad_enabled()
    s.__exit__()
    assert not ops.warp_grad_enabled()
    assert set(ops.WARP_GRAD_CALLS) == {"forward", "backward", "torch"}


def _cpu_warps(x, rows):
    """The three gradient-path warps on CPU tensors -> their results."""
    aff = torch.from_numpy(rows.reshape(1, 1, -1, 2, 3))
    return [fio.warp_to_ego(x, rows.reshape(-1, 2, 3), True), fio._warp_affine_simple(x, aff[0, 0], tuple(x.shape[2:]))]


@pytest.mark.grad
@pytest.mark.parametrize("mode", ["torch", "kernel"])
def test_cpu_tensors_run_the_torch_lines(mode, monkeypatch):
    """The default mode, and CPU tensors in "kernel" mode, never reach the library."""
    def boom(*a, **k):
        raise AssertionError("the C ABI was called")
    monkeypatch.setattr(_capi, "call", boom)
    H, W = 13, 21
    named = R.named_rows(H, W)
    rows = np.stack([named["rot37"], named["shift"]])
    x = torch.randn(2, 3, H, W, requires_grad=True)
    before = dict(ops.WARP_GRAD_CALLS)
    with ops.warp_grad(mode):
        outs = _cpu_warps(x, rows)
        model = fio.MaxFusion()
        fused = model(x, torch.tensor([2]), torch.from_numpy(rows.reshape(1, 1, 2, 2, 3)).expand(1, 2, 2, 2, 3))
    want = F.grid_sample(x, F.affine_grid(torch.from_numpy(rows.reshape(2, 2, 3)).float(), [2, 3, H, W], align_corners=False),
                         align_corners=False)
    assert torch.equal(outs[0], want)
    assert (outs[1] - want).abs().max() < 1e-5          # its grid is built in float64, then cast
    assert torch.equal(fused[0], want.max(dim=0)[0])
    fused.sum().backward()
    assert x.grad is not None and x.grad.abs().sum() > 0
    assert ops.WARP_GRAD_CALLS["forward"] == before["forward"] and ops.WARP_GRAD_CALLS["backward"] == before["backward"]
    assert ops.WARP_GRAD_CALLS["torch"] == before["torch"] + 3


def test_gpu_fixtures_are_not_vacuous():
    """Every agent of every GPU fixture but the all-outside one reaches at least half of its source pixels; the outside one none."""
    seen_outside = False
    for name, (H, W, C, rows) in R.gpu_fixtures().items():
        assert 1 <= len(rows) <= MAX_AGENTS and _supported(rows, len(rows), H, W) == 1, name
        for f64 in (True, False):
            Rs = R.Restated(rows, H, W, f64)
            for a, row in enumerate(rows):
                if R.is_outside(row, H, W):
                    assert Rs.coverage(a) == 0.0
                    seen_outside = True
                else:
                    assert Rs.coverage(a) >= 0.5, (name, a, Rs.coverage(a))
    assert seen_outside
    shapes = {(H, W) for H, W, _, _ in R.gpu_fixtures().values()}
    assert shapes == {(1, 1), (1, 7), (13, 21), (32, 48)}
    assert {C for _, _, C, _ in R.gpu_fixtures().values()} == {1, 33, 70}
    assert {len(r) for _, _, _, r in R.gpu_fixtures().values()} == {1, 3, MAX_AGENTS}
    with open(_capi.HEADER_TRAIN_WARP) as f:
        assert "#define HEAL_WARP_BWD_CHANNELS 32" in f.read()           # 33 = one channel more than a chunk
