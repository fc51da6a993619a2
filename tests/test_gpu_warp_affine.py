"""heal_warp_affine_forward / heal_warp_affine_backward (include/heal_amd_train_warp.h) through the C ABI, per element.

Every operand lies inside a NaN-filled buffer (a read outside the operand poisons the result, a write outside it is seen in the
guard words), once with every base pointer moved by one float.  The backward is held to the float64 restatement of
tests/warp_refs.py at  |got - want| <= 1e-5 * sum_d |w| |G| + 1e-30  per element; the forward must be bit-equal to ops.warp_agent
agent by agent; a second backward launch must be bit-equal to the first; a refused call must launch nothing."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, ops
from tests import warp_refs as R

pytestmark = pytest.mark.gpu

FIXTURES = R.gpu_fixtures()
GUARD = 64      # NaN words before and after every operand


def _dev():
    return torch.device("cuda:0")


def _embed(t, offset):
    """A copy of t (or an uninitialised operand of t's shape when t is a shape) inside a NaN-filled buffer, `offset` floats off the
    buffer's alignment -> (view, buffer)."""
    shape = tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD + offset,), float("nan"), dtype=torch.float32, device=_dev())
    view = buf[GUARD + offset:GUARD + offset + numel].view(shape)
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    return view, buf


def _guards_intact(view, buf, offset):
    numel = view.numel()
    return bool(torch.isnan(buf[:GUARD + offset]).all() and torch.isnan(buf[GUARD + offset + numel:]).all())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _host_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 6)
    return rows, rows.ctypes.data_as(ctypes.c_void_p)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _backward(G, rows, f64, offset=0):
    """heal_warp_affine_backward on G [n, C, H, W] (a CPU tensor) -> (grad_src on the CPU, guards intact)."""
    n, C, H, W = G.shape
    g, gbuf = _embed(G, offset)
    out, obuf = _embed(G.shape, offset)
    keep, rp = _host_rows(rows)
    _capi.call("heal_warp_affine_backward", _ptr(g), n, C, H, W, rp, int(f64), _ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu(), _guards_intact(out, obuf, offset) and _guards_intact(g, gbuf, offset)


def _forward(x, rows, f64, offset=0, device_rows=False):
    n, C, H, W = x.shape
    xs, xbuf = _embed(x, offset)
    out, obuf = _embed(x.shape, offset)
    keep, rp = _host_rows(rows)
    dev = torch.from_numpy(keep).to(_dev()) if device_rows else None
    _capi.call("heal_warp_affine_forward", _ptr(xs), n, C, H, W, ctypes.c_void_p(0) if device_rows else rp,
               _ptr(dev) if device_rows else ctypes.c_void_p(0), int(f64), _ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu(), _guards_intact(out, obuf, offset)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(G, float64 adjoint, per-element scale) of a fixture with float64 rows: computed once, shared, never written."""
    H, W, C, rows = FIXTURES[name]
    Rs = R.Restated(rows, H, W, True)
    G = R.fixture_grad(name, len(rows), C, H, W)
    return G, Rs.adjoint(G), Rs.scale(G)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_backward_per_element(name, offset):
    H, W, C, rows = FIXTURES[name]
    G, want, scale = _reference(name)
    got, intact = _backward(G, rows, True, offset)
    assert intact
    assert not torch.isnan(got).any()                      # every element written, none from outside the operand
    err = (got.double() - want).abs()
    bound = R.BOUND * scale + R.TINY
    print(f"{name} offset {offset}: max err / bound = {float((err / bound).max()):.3f}, max err = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())
    for a, row in enumerate(rows):
        if R.is_outside(row, H, W):
            assert torch.equal(got[a], torch.zeros_like(got[a]))     # written as exact zeros
        else:
            assert float((got[a] != 0).float().mean()) >= 0.5        # not a vacuous comparison of zeros


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("name", ["13x21_n8_c1", "32x48_n3_c33_outside"])
def test_backward_twice_bit_equal(name, f64):
    H, W, C, rows = FIXTURES[name]
    G = _reference(name)[0]
    first, _ = _backward(G, rows, f64)
    second, _ = _backward(G, rows, f64, offset=1)
    assert torch.equal(first, second)


@pytest.mark.parametrize("f64", [True, False])
def test_backward_is_the_adjoint_of_the_forward_kernel(f64):
    """Both grid dtypes, without a restatement of the positions: one-hot maps through the FORWARD kernel give its weights exactly
    (x = 1 at one source pixel: out[d] = 1 * w(d, s), every other tap adds 0 * w), so  sum_d w(d, s) G[d]  in float64 with the
    per-element bound 1e-5 * sum_d |w| |G| is the backward's reference."""
    H, W = 13, 21
    named = R.named_rows(H, W)
    rows = np.stack([named["rot37"], named["scale150"], R.random_rigid(1, H, W, 9, 0.1)[0]])
    n, P = len(rows), H * W
    onehot = torch.eye(P, dtype=torch.float32).view(1, P, H, W).expand(n, -1, -1, -1).contiguous()     # channel s = pixel s
    wk, intact = _forward(onehot, rows, f64)               # wk[a, s, d] = w(d, s)
    assert intact
    wk = wk.double().view(n, P, P)
    C = 5
    G = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(4), dtype=torch.float32)
    g = G.double().view(n, C, P)
    want = torch.einsum("asd,acd->acs", wk, g).view(n, C, H, W)
    scale = torch.einsum("asd,acd->acs", wk.abs(), g.abs()).view(n, C, H, W)
    got, intact = _backward(G, rows, f64)
    assert intact
    err = (got.double() - want).abs()
    bound = R.BOUND * scale + R.TINY
    print(f"f64 {f64}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((scale > 0).float().mean()) >= 0.5


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("device_rows", [False, True])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_forward_bit_equal_to_warp_agent(name, device_rows, f64):
    H, W, C, rows = FIXTURES[name]
    n = len(rows)
    x = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(7), dtype=torch.float32)
    got, intact = _forward(x, rows, f64, offset=1 if device_rows else 0, device_rows=device_rows)
    assert intact and not torch.isnan(got).any()
    xd = x.to(_dev())
    zeros = torch.zeros((1, H, W), dtype=torch.float32, device=_dev())
    for a in range(n):
        row = torch.from_numpy(rows[a].reshape(2, 3)).to(_dev()) if device_rows else rows[a].reshape(2, 3)
        want = ops.warp_agent(xd[a], zeros, row, f64)[0].cpu()
        assert torch.equal(got[a], want), (name, a)
    # and through the wrapper, the same bits
    assert torch.equal(ops.warp_affine(xd, rows.reshape(n, 2, 3), f64).cpu(), got)
    if not f64:
        return
    # the float64 restatement of the same warp (not bit-equal: fp32 products and sums)
    want = R.Restated(rows, H, W, True).forward(x)
    assert float((got.double() - want).abs().max()) <= 1e-5 * float(x.abs().max())


def test_wrapper_chunks_above_the_agent_limit():
    """ops.warp_affine / ops.warp_affine_backward with more agents than one launch takes: chunks of HEAL_WARP_MAX_AGENTS."""
    H, W, C = 13, 21, 3
    n = ops.WARP_MAX_AGENTS + 2
    rows = R.random_rigid(n, H, W, 11, 0.1)
    x = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(3), dtype=torch.float32).to(_dev())
    got = ops.warp_affine(x, rows.reshape(n, 2, 3), True)
    gb = ops.warp_affine_backward(x, rows.reshape(n, 2, 3), True)
    for lo, hi in ((0, 8), (8, n)):
        assert torch.equal(got[lo:hi], ops.warp_affine(x[lo:hi], rows[lo:hi].reshape(-1, 2, 3), True))
        assert torch.equal(gb[lo:hi], ops.warp_affine_backward(x[lo:hi], rows[lo:hi].reshape(-1, 2, 3), True))
    assert ops.warp_affine_train_supported(x, rows.reshape(n, 2, 3))


def test_refusals_launch_nothing():
    H, W, C = 13, 21, 3
    named = R.named_rows(H, W)
    good = named["rot37"]
    G = torch.randn(2, C, H, W, dtype=torch.float32)
    g, _ = _embed(G, 0)
    bad_rows = {"singular": np.stack([good, np.zeros(6)]), "nan": np.stack([good, np.where(np.arange(6) == 2, np.nan, good)]),
                "reach": np.stack([good, R.rigid(10, 0, 0, H, W, 0.2)])}
    for why, rows in bad_rows.items():
        out, obuf = _embed(G.shape, 0)
        keep, rp = _host_rows(rows)
        with pytest.raises(_capi.HealAmdError, match="not supported"):
            _capi.call("heal_warp_affine_backward", _ptr(g), 2, C, H, W, rp, 1, _ptr(out), _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(obuf).all()), why                # nothing was written
        assert not ops.warp_affine_train_supported(g, rows.reshape(2, 2, 3))
    out, obuf = _embed(G.shape, 0)
    keep, rp = _host_rows(np.stack([good] * 9))
    for n in (0, 9):
        with pytest.raises(_capi.HealAmdError, match="n must be in"):
            _capi.call("heal_warp_affine_backward", _ptr(g), n, C, H, W, rp, 1, _ptr(out), _stream())
        with pytest.raises(_capi.HealAmdError, match="n must be in"):
            _capi.call("heal_warp_affine_forward", _ptr(g), n, C, H, W, rp, ctypes.c_void_p(0), 1, _ptr(out), _stream())
    with pytest.raises(_capi.HealAmdError, match="host"):        # device-resident rows are not accepted by the backward
        _capi.call("heal_warp_affine_backward", _ptr(g), 2, C, H, W, ctypes.c_void_p(0), 1, _ptr(out), _stream())
    with pytest.raises(_capi.HealAmdError, match="NULL"):
        _capi.call("heal_warp_affine_forward", _ptr(g), 2, C, H, W, ctypes.c_void_p(0), ctypes.c_void_p(0), 1, _ptr(out), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf).all())
    # the wrapper's own checks
    with pytest.raises(_capi.HealAmdError):
        ops.warp_affine(G, good.reshape(1, 2, 3))                 # a CPU tensor
    assert not ops.warp_affine_train_supported(G, np.stack([good, good]).reshape(2, 2, 3))
    assert not ops.warp_affine_train_supported(g.double(), np.stack([good, good]).reshape(2, 2, 3))
    assert not ops.warp_affine_train_supported(g, torch.zeros(2, 2, 3, requires_grad=True))
    with pytest.raises(_capi.HealAmdError, match="does not take these rows"):
        ops.WarpAffine.apply(g, bad_rows["singular"].reshape(2, 2, 3), True)


@pytest.mark.grad
@pytest.mark.parametrize("device_rows", [False, True])
def test_warp_affine_function_against_float64_autograd(device_rows):
    """ops.WarpAffine on 2 x 3 x 13 x 21 against float64 autograd of affine_grid + grid_sample.  The float64 composition samples at
    float64 positions, the operator at the fp32-rounded ones: a position differs by at most ~5e-6 pixel per axis (gx rounded to
    fp32: 6e-8 * 1.5 * W / 2; three fp32 operations of the un-normalisation on values up to W = 21), a weight by twice that, and a
    source pixel has at most six contributors: |difference| <= 6e-5 max|G|, held to 1e-4 max|G| (value and gradient)."""
    H, W = 13, 21
    named = R.named_rows(H, W)
    rows = np.stack([named["rot37"], R.random_rigid(1, H, W, 13, 0.1)[0]]).reshape(2, 2, 3)
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float32)
    G = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float32)
    x64 = x.double().requires_grad_(True)
    y64 = F.grid_sample(x64, F.affine_grid(torch.from_numpy(rows), [2, 3, H, W], align_corners=False), align_corners=False)
    y64.backward(G.double())
    xd = x.to(_dev()).requires_grad_(True)
    before = dict(ops.WARP_GRAD_CALLS)
    y = ops.WarpAffine.apply(xd, torch.from_numpy(rows).to(_dev()) if device_rows else rows, True)
    y.backward(G.to(_dev()))
    assert ops.WARP_GRAD_CALLS["forward"] == before["forward"] + 1 and ops.WARP_GRAD_CALLS["backward"] == before["backward"] + 1
    assert float((y.detach().cpu().double() - y64.detach()).abs().max()) <= 1e-4 * float(x.abs().max())
    assert float((xd.grad.cpu().double() - x64.grad).abs().max()) <= 1e-4 * float(G.abs().max())
    assert float(xd.grad.abs().max()) > 0


def test_device_rows_refused_under_capture(monkeypatch):
    """The 48 n byte copy of device rows to the host cannot run under stream capture: ops.WarpAffine says so (a clear error, not a
    broken graph) and warp_affine_train_supported answers False, so the modules fall back to torch there."""
    H, W = 13, 21
    rd = torch.from_numpy(R.named_rows(H, W)["rot37"].reshape(1, 2, 3)).to(_dev())
    x = torch.zeros(1, 2, H, W, device=_dev())
    torch.cuda.synchronize()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert not ops.warp_affine_train_supported(x, rd)
    with pytest.raises(_capi.HealAmdError, match="capture"):
        ops.WarpAffine.apply(x, rd, True)


def test_forward_is_capture_safe_and_follows_device_rows():
    """ops.warp_affine with device-resident rows recorded into a graph: the replay reads the rows of the replay's time."""
    H, W, C = 13, 21, 5
    named = R.named_rows(H, W)
    first, second = np.stack([named["rot37"], named["shift"]]), np.stack([named["rot180"], named["scale150"]])
    x = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float32).to(_dev())
    want = ops.warp_affine(x, second.reshape(2, 2, 3), True)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        rows = torch.from_numpy(first.reshape(2, 2, 3)).to(_dev())
        ops.warp_affine(x, rows, True)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            y = ops.warp_affine(x, rows, True)
        rows.copy_(torch.from_numpy(second.reshape(2, 2, 3)))
        graph.replay()
        st.synchronize()
        assert torch.equal(y, want)
