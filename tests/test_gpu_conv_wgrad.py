"""heal_conv_wgrad (the dense convolutions' weight gradient) and the kernel-backed convolution backward built on it
(ops.ConvGrad, bev_blocks.grad_conv, HEAL_CONV_GRAD=kernel).

Part 1 follows tests/test_gpu_conformance.py: integer operands whose every partial sum stays far below 2^24, so fp32 is exact in ANY
summation order and any split of the pixel reduction, and the kernel must equal torch.nn.grad.conv2d_weight evaluated on the CPU in
float64 BIT FOR BIT.  Operands, result and workspace sit inside NaN-poisoned buffers whose guard words are checked.
The kernel's tiling (include/heal_amd_train.h): blocks of 64 output x 32 input channels (16-wide MFMA tiles), pixel tiles of R output
rows x 32 output columns (R = 4 at stride 1, 2 at stride 2), the list of n * ceil(Ho / R) * ceil(Wo / 32) tiles cut into
heal_conv_wgrad_splits contiguous runs of which the first tiles % splits hold one tile more.

Part 3 bounds the rounding error of random fp32 inputs per element by gamma_m * sum|g||x| with m the number of summands of that
element -- the standard bound of an m-term inner product, valid for every summation order, so nothing is tuned."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gpu_conformance import (PAD, POISON, _assert_equal, _assert_poison_outside, _chan_mag, _exact_bound, _ints,
                                         _pix_mag, _poisoned)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _tiles(n, H, W, stride):
    Ho, Wo, R = (H - 1) // stride + 1, (W - 1) // stride + 1, 4 if stride == 1 else 2
    return n * -(-Ho // R) * -(-Wo // 32)


def _splits(case):
    from heal_amd import _capi
    return int(_capi.lib().heal_conv_wgrad_splits(*case))


def _nonzero_border(t):
    """Zeros on the outermost rows and columns become 1: a padding read that lands on the border instead of outside changes the sum."""
    b = torch.zeros(t.shape[-2:], dtype=torch.bool)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
    return torch.where(b & (t == 0), torch.ones_like(t), t)


def _int_operands(seed, n, cin, cout, H, W, k, s):
    """x: integers in [-3, 3] times the 1 | 2 pixel magnitudes, g: integers in [-2, 2] times the 2 / 1 / 0 output-channel magnitudes;
    border pixels non-zero (before the channel magnitude: a magnitude-0 channel stays all zero)."""
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x = _nonzero_border(_ints(gen, (n, cin, H, W), -3, 3)) * _pix_mag(H, W)
    g = _nonzero_border(_ints(gen, (n, cout, Ho, Wo), -2, 2)) * _chan_mag(cout).view(1, -1, 1, 1)
    return x, g


def _ref64(x, g, cout, cin, k, s):
    """(dW, sum |g||x|, number of summands) per element, float64 on the CPU."""
    shape = (cout, cin, k, k)
    x, g = x.detach().double().cpu(), g.detach().double().cpu()
    ref = torch.nn.grad.conv2d_weight(x, shape, g, stride=s, padding=k // 2)
    mag = torch.nn.grad.conv2d_weight(x.abs(), shape, g.abs(), stride=s, padding=k // 2)
    cnt = torch.nn.grad.conv2d_weight(torch.ones_like(x), shape, torch.ones_like(g), stride=s, padding=k // 2)
    return ref, mag, cnt


def _launch_guarded(x, g, case):
    """heal_conv_wgrad through the C ABI on poisoned operands, a poisoned result and a poisoned workspace -> (dW, guard check)."""
    from heal_amd import _capi, ops
    n, cin, cout, H, W, k, s = case
    bx, xv = _poisoned(x)
    bg, gv = _poisoned(g)
    count = cout * cin * k * k
    bd, dw = _poisoned(torch.zeros(cout, cin, k, k))
    bd.view(torch.int32)[PAD:PAD + count] = POISON            # an element the kernel does not write stays NaN
    nbytes = _capi.query("heal_conv_wgrad_workspace", *case)
    assert nbytes == (0 if _splits(case) == 1 else _splits(case) * count * 4)
    bw, wv = _poisoned(torch.zeros(max(nbytes // 4, 4)))
    bw.view(torch.int32)[PAD:PAD + wv.numel()] = POISON

    def run():
        _capi.call("heal_conv_wgrad", ops._ptr(xv), ops._ptr(gv), n, cin, cout, H, W, k, s, ops._ptr(dw),
                   ops._ptr(wv) if nbytes else None, nbytes, ops._stream())
        torch.cuda.synchronize()
        return dw.clone()

    def guards():
        _assert_poison_outside(bx, PAD, PAD + x.numel(), "conv_wgrad x")
        _assert_poison_outside(bg, PAD, PAD + g.numel(), "conv_wgrad g")
        _assert_poison_outside(bd, PAD, PAD + count, "conv_wgrad dW")
        _assert_poison_outside(bw, PAD, PAD + nbytes // 4, "conv_wgrad workspace")
        assert torch.equal(xv.cpu(), x) and torch.equal(gv.cpu(), g), "conv_wgrad wrote into an operand"

    return run, guards


MULTI = (1, 8, 16, 26, 70, 3, 1)         # 7 x 3 = 21 pixel tiles in 11 splits: ten of two tiles and a last one of one
EXACT_CASES = [
    pytest.param((1, 8, 16, 8, 8, 3, 1), id="one_tile_one_split"),
    pytest.param((3, 10, 70, 19, 21, 3, 1), id="ragged_channels_and_tiles_images_inside_a_split"),
    pytest.param((2, 33, 65, 17, 18, 3, 2), id="odd_H_stride2_three_channel_blocks"),
    pytest.param((2, 40, 24, 12, 20, 1, 1), id="pointwise_stride1"),
    pytest.param((2, 40, 24, 13, 20, 1, 2), id="pointwise_stride2"),
    pytest.param(MULTI, id="eleven_splits_short_last"),
]


def test_case_shapes_aim_at_what_they_name():
    """The split counts the case ids rely on, from heal_conv_wgrad_splits (a pure function of the shape)."""
    assert _splits((1, 8, 16, 8, 8, 3, 1)) == 1 and _tiles(1, 8, 8, 1) == 2
    s = _splits((3, 10, 70, 19, 21, 3, 1))
    assert s >= 3 and _tiles(3, 19, 21, 1) == 15 and 15 % s and 15 // s < 5     # runs of < 5 tiles: some span two images
    s = _splits(MULTI)
    t = _tiles(*MULTI[:1], *MULTI[3:5], MULTI[6])
    assert s >= 3 and t % s != 0 and t // s >= 1, (s, t)                           # the last run is one tile shorter than the first


@pytest.mark.parametrize("case", EXACT_CASES)
def test_conv_wgrad_exact_on_integers(case):
    from heal_amd import ops
    n, cin, cout, H, W, k, s = case
    x, g = _int_operands(sum(case), *case)
    ref, mag, _ = _ref64(x, g, cout, cin, k, s)
    _exact_bound(mag)
    run, guards = _launch_guarded(x, g, case)
    got = run()
    _assert_equal(got, ref, f"heal_conv_wgrad {case} [co, ci, ky, kx]")
    guards()
    _assert_equal(ops.conv_wgrad(x.cuda(), g.cuda(), k, s), ref, f"ops.conv_wgrad {case}")


def test_conv_wgrad_is_deterministic_over_splits():
    """Two launches on the multi-split case are bit-equal, on random fp32 inputs where the order of the partial sums matters."""
    from heal_amd import ops
    n, cin, cout, H, W, k, s = MULTI
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, H, W, generator=gen)
    g = torch.randn(n, cout, H, W, generator=gen)
    run, guards = _launch_guarded(x, g, MULTI)
    a, b = run(), run()
    guards()
    assert not torch.isnan(a).any()
    assert torch.equal(a, b)
    assert torch.equal(ops.conv_wgrad(x.cuda(), g.cuda(), k, s), a)


def _assert_gamma(got, x, g, k, s, what):
    ref, mag, cnt = _ref64(x, g, int(g.shape[1]), int(x.shape[1]), k, s)
    m = cnt * U
    bound = m / (1.0 - m) * mag
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max error / bound = {worst:.3f}, max summands {int(cnt.max())}")
    assert bool((err <= bound).all()), f"{what}: error exceeds gamma_m sum|g||x| by a factor {worst}"


@pytest.mark.parametrize("case", [(2, 64, 64, 32, 32, 3, 1), (2, 128, 64, 31, 33, 3, 2)])
def test_conv_wgrad_random_fp32_within_the_inner_product_bound(case):
    from heal_amd import ops
    n, cin, cout, H, W, k, s = case
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(n, cin, H, W, generator=gen)
    g = torch.randn(n, cout, (H - 1) // s + 1, (W - 1) // s + 1, generator=gen)
    _assert_gamma(ops.conv_wgrad(x.cuda(), g.cuda(), k, s), x, g, k, s, f"conv_wgrad {case}")


def _close(got, ref, tol, what):
    ref = ref.detach().double().cpu()
    err = float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"{what}: {err:.2e} of scale")
    assert err < tol, (what, err)


@pytest.mark.grad
@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_conv_grad_function_vs_float64_autograd(k, s):
    """ops.ConvGrad against F.conv2d differentiated on the CPU in float64: the output, dx and db within 1e-4 of their scale, dW within
    the inner-product bound; the data gradient ran on the forward kernels at stride 1 and on the library at stride 2."""
    from heal_amd import ops
    n, cin, cout, H, W = 2, 16, 32, 16, 16
    gen = torch.Generator().manual_seed(100 + 10 * k + s)
    x = torch.randn(n, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.2
    b = torch.randn(cout, generator=gen)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv2d(x64, w64, b64, s, k // 2)
    ct = torch.randn(y64.shape, generator=gen)
    y64.backward(ct.double())
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    before = dict(ops.CONV_GRAD_CALLS)
    y = ops.ConvGrad.apply(xd, wd, bd, s)
    y.backward(ct.cuda())
    torch.cuda.synchronize()
    delta = {key: ops.CONV_GRAD_CALLS[key] - before[key] for key in before}
    assert delta == {"forward": 1, "wgrad": 1, "dx_kernel": 1 if s == 1 else 0, "dx_library": 0 if s == 1 else 1}, delta
    _close(y, y64, 1e-4, "y")
    _close(xd.grad, x64.grad, 1e-4, "dx")
    _close(bd.grad, b64.grad, 1e-4, "db")
    _assert_gamma(wd.grad, x, ct, k, s, f"ConvGrad dW k={k} s={s}")
    # only the gradients asked for: a frozen weight costs no weight-gradient launch
    before = dict(ops.CONV_GRAD_CALLS)
    xd2 = x.cuda().requires_grad_(True)
    ops.ConvGrad.apply(xd2, wd.detach(), None, s).backward(ct.cuda())
    assert ops.CONV_GRAD_CALLS["wgrad"] == before["wgrad"]
    _close(xd2.grad, x64.grad, 1e-4, "dx (frozen weight, no bias)")


def _module_cases():
    from heal_amd.opencood.models.sub_modules.base_bev_backbone import _PlainStage
    from heal_amd.opencood.models.sub_modules.bev_blocks import BasicBlock, DoubleConv, conv1x1
    torch.manual_seed(31)
    down = nn.Sequential(conv1x1(32, 32, 2), nn.BatchNorm2d(32))
    # a stage of BaseBEVBackbone: the opener is ZeroPad2d(1) + a padding-0 stride-2 convolution (the pad becomes the kernel's own)
    stage = _PlainStage([nn.ZeroPad2d(1), nn.Conv2d(32, 32, 3, stride=2, padding=0, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                         nn.Conv2d(32, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU()])
    # (module, ConvGrad calls of one forward + backward: forward, wgrad, dx_kernel, dx_library)
    return [("BasicBlock_s2", BasicBlock(32, 32, 2, down), (3, 3, 1, 2)), ("DoubleConv", DoubleConv(32, 32, 3, 1, 1), (2, 2, 2, 0)),
            ("PlainStage_s2", stage, (2, 2, 1, 1))]


@pytest.mark.grad
@pytest.mark.parametrize("which", [0, 1, 2], ids=["BasicBlock_s2", "DoubleConv", "PlainStage_s2"])
def test_modules_under_the_switch_vs_float64(which, monkeypatch):
    """Training mode, 32 channels, 16 x 16, batch 2, one backward: with HEAL_CONV_GRAD=kernel every convolution of the block goes
    through ConvGrad and the output and every gradient lie within 1e-4 of scale of the same module differentiated on the CPU in
    float64; with the switch unset the call takes the library path (counters untouched) and meets the same figures."""
    from heal_amd import ops
    name, mod, calls = _module_cases()[which]
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 32, 16, 16, generator=gen)
    ref = copy.deepcopy(mod).double().train()
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    ct = torch.randn(y64.shape, generator=gen)
    y64.backward(ct.double())
    for mode in ("kernel", None):
        if mode is None:
            monkeypatch.delenv("HEAL_CONV_GRAD", raising=False)
        else:
            monkeypatch.setenv("HEAL_CONV_GRAD", mode)
        dev = copy.deepcopy(mod).cuda().train()
        xd = x.cuda().requires_grad_(True)
        before = dict(ops.CONV_GRAD_CALLS)
        y = dev(xd)
        y.backward(ct.cuda())
        torch.cuda.synchronize()
        delta = tuple(ops.CONV_GRAD_CALLS[key] - before[key] for key in ("forward", "wgrad", "dx_kernel", "dx_library"))
        assert delta == (calls if mode else (0, 0, 0, 0)), (name, mode, delta)
        _close(y, y64, 1e-4, f"{name} [{mode}] y")
        _close(xd.grad, x64.grad, 1e-4, f"{name} [{mode}] dx")
        for (pn, p), (_, p64) in zip(dev.named_parameters(), ref.named_parameters()):
            assert p.grad is not None, pn
            _close(p.grad, p64.grad, 1e-4, f"{name} [{mode}] {pn}")


@pytest.mark.grad
def test_training_steps_under_the_switch(monkeypatch):
    """The small pyramid LiDAR model from raw point clouds, three Adam steps with HEAL_CONV_GRAD=kernel: the convolutions ran through
    ConvGrad, the loss is finite and decreases, every parameter has a finite gradient.
    The step size is 1e-5: the same scene is fed every step, so the loss is a deterministic function of the parameters and a step
    small enough for first-order descent must lower it if the gradients are right.  (At 1e-4 and 1e-3 the SECOND step overshoots on
    this loss with the library's gradients as well -- 0.429, 0.175, 1.226 at 1e-4 -- which says nothing about either backward.)"""
    from heal_amd import configs, ops
    from heal_amd.opencood.tools.train_utils import create_model
    from heal_amd.pipeline import Scene
    from tests.golden.detfill import fill_module
    monkeypatch.setenv("HEAL_CONV_GRAD", "kernel")
    hypes = configs.lidar_pyramid([-25.6, -25.6, -3, 25.6, 25.6, 1])
    model = fill_module(create_model(hypes)).cuda()
    data = Scene(2, seed=3, device="cuda:0", modalities=["m1", "m1"]).model_input()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    before = dict(ops.CONV_GRAD_CALLS)
    losses = []
    for _step in range(3):
        opt.zero_grad()
        out = model(data)
        loss = sum(out[key].square().mean() for key in ("cls_preds", "reg_preds", "dir_preds"))
        assert bool(torch.isfinite(loss))
        loss.backward()
        for pn, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pn
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses, "ConvGrad calls", {key: ops.CONV_GRAD_CALLS[key] - before[key] for key in before})
    assert ops.CONV_GRAD_CALLS["forward"] - before["forward"] >= 3 * 10
    assert ops.CONV_GRAD_CALLS["wgrad"] - before["wgrad"] == ops.CONV_GRAD_CALLS["forward"] - before["forward"]
    assert ops.CONV_GRAD_CALLS["dx_kernel"] > before["dx_kernel"]
    assert losses[-1] < losses[0], losses
