"""The streaming kernels of the camera branch at their edges: k_depthwise<K, STRIDE> (one wave per 32 x 8 output tile, four
tiles to a block, 16-B staging where the rows are aligned), k_se_gate's parallel squeeze over the per-tile sums, and the split
LayerNorm (C <= 128, C % 4 == 0: four waves share a pixel's channels) beside the general one.

The depthwise maps are OUTPUT maps (tiles are tiles of the output); the input is sized to produce them under the asymmetric
paddings of test_depthwise_conv_exact_with_channel_sums.  Those paddings give an input width W % 4 != 0 for every stride-1 case
but the 2 x 3 map, so `aligned` adds "same"-padded inputs with W % 4 == 0 (the model's case: the 16-B staging path)."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conformance import U, _assert_act, _assert_equal, _bias, _chan_mag, _conv_ref, _exact_bound, _input, _ints

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1, "silu": 2}
# (k, stride) -> (left, right, top, bottom), the asymmetric paddings of the conformance test
INSTANCES = {(3, 1): (0, 1, 1, 0), (3, 2): (0, 1, 0, 1), (5, 1): (2, 1, 0, 2), (5, 2): (1, 2, 2, 1), (7, 1): (3, 2, 1, 3)}
OUT_MAPS = [(1, 1), (2, 3), (8, 32), (9, 33), (7, 36), (12, 16), (5, 130)]
BATCHES = [(1, 3), (3, 7)]             # (n, C): 3 and 21 planes, so the item counts include values that are no multiple of 4


def _depthwise(x, w, b, k, stride, pad, act):
    """heal_depthwise_conv into NaN-filled y and channel_sums: (y, sums [n, C, T]) on the host."""
    from heal_amd import _capi, ops
    n, C, H, W = x.shape
    pl, pr, pt, pb = pad
    Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
    bd = None if b is None else b.cuda().contiguous()
    y = torch.full((n, C, Ho, Wo), float("nan"), device="cuda")
    sums = torch.full((n, C, ops.depthwise_tiles(Ho, Wo)), float("nan"), device="cuda")
    _capi.call("heal_depthwise_conv", ops._ptr(xd), ops._ptr(wd), ops._ptr(bd), n, C, H, W, k, stride, pt, pl, Ho, Wo, ACTS[act],
               ops._ptr(y), ops._ptr(sums), ops._stream())
    torch.cuda.synchronize()
    return y.cpu(), sums.cpu()


def _tile_view(y):
    n, C, Ho, Wo = y.shape
    ty, tx = -(-Ho // 8), -(-Wo // 32)
    return F.pad(y, (0, tx * 32 - Wo, 0, ty * 8 - Ho)).reshape(n, C, ty, 8, tx, 32), ty * tx


def _check_case(g, k, stride, pad, n, C, H, W, what):
    pl, pr, pt, pb = pad
    # integers: every partial sum is exact in fp32, so y and the tile sums are THE integers
    x = _input(g, n, C, H, W)
    w = _ints(g, (C, 1, k, k), -2, 2) * _chan_mag(C).view(-1, 1, 1, 1)
    b = _bias(g, C)
    pre, bound = _conv_ref(x, w, b, None, stride, pad, C)
    _exact_bound(bound)
    for act in ("none", "relu"):
        y, sums = _depthwise(x, w, b, k, stride, pad, act)
        _assert_act(y, pre, act, f"{what} {act}")
        tiles, T = _tile_view(torch.relu(pre) if act == "relu" else pre)
        assert sums.shape == (n, C, T)
        _assert_equal(sums, tiles.sum(dim=(3, 5)).reshape(n, C, T), f"{what} {act} tile sums")
    # SiLU on random inputs: the tolerance of test_depthwise_conv_vs_torch against fp64; each tile sum within the bound of a depth-8
    # tree, 8 u sum|y|, around the fp64 sum of the kernel's own outputs; every word of the NaN-filled buffers written
    xr = torch.randn((n, C, H, W), generator=g)
    wr = torch.randn((C, 1, k, k), generator=g) * 0.3
    br = torch.randn((C,), generator=g)
    ref = F.silu(F.conv2d(F.pad(xr, pad).double(), wr.double(), br.double(), stride, 0, 1, C))
    y, sums = _depthwise(xr, wr, br, k, stride, pad, "silu")
    assert y.shape == ref.shape and bool(torch.isfinite(y).all()), f"{what} silu: an output was not written"
    assert bool(torch.isfinite(sums).all()), f"{what} silu: a word of channel_sums was not written"
    torch.testing.assert_close(y, ref.float(), rtol=1e-4, atol=1e-5)
    tiles, T = _tile_view(y.double())
    want = tiles.sum(dim=(3, 5)).reshape(n, C, T)
    tol = 8 * U * tiles.abs().sum(dim=(3, 5)).reshape(n, C, T)
    worst = float(((sums.double() - want).abs() / tol.clamp_min(1e-300)).max())
    assert bool(((sums.double() - want).abs() <= tol).all()), f"{what} silu: a tile sum is {worst:.2f} x its bound 8 u sum|y|"


@pytest.mark.parametrize("k,stride", sorted(INSTANCES), ids=[f"k{k}_s{s}" for k, s in sorted(INSTANCES)])
def test_depthwise_edges(k, stride):
    pad = INSTANCES[(k, stride)]
    pl, pr, pt, pb = pad
    g = torch.Generator().manual_seed(100 * k + stride)
    for Ho, Wo in OUT_MAPS:
        H, W = (Ho - 1) * stride + k - pt - pb, (Wo - 1) * stride + k - pl - pr
        for n, C in BATCHES:
            _check_case(g, k, stride, pad, n, C, H, W, f"k{k} s{stride} out {Ho}x{Wo} in {H}x{W} n{n} C{C}")


@pytest.mark.parametrize("k,stride", sorted(INSTANCES), ids=[f"k{k}_s{s}" for k, s in sorted(INSTANCES)])
def test_depthwise_edges_aligned(k, stride):
    """Inputs with W % 4 == 0 (16-B staging) under TF-style "same" padding, the model's case: a 4-wide map (one chunk), the deep-stage
    12 x 16 map, one with a partial last tile column and one 5 tiles wide whose last chunk of a row ends at the map's edge."""
    g = torch.Generator().manual_seed(100 * k + stride + 7)
    for H, W in ((3, 4), (12, 16), (9, 72), (5, 132)):
        tw, th = max((-(-W // stride) - 1) * stride + k - W, 0), max((-(-H // stride) - 1) * stride + k - H, 0)
        pad = (tw // 2, tw - tw // 2, th // 2, th - th // 2)
        for n, C in BATCHES:
            _check_case(g, k, stride, pad, n, C, H, W, f"k{k} s{stride} same-padded in {H}x{W} n{n} C{C}")


@pytest.mark.parametrize("n,C,S,T", [(4, 32, 8, 192), (4, 96, 4, 48), (3, 33, 8, 65), (2, 240, 10, 12), (1, 1152, 48, 2),
                                     (2, 1100, 48, 64)])
def test_se_gate_with_tiles(n, C, S, T):
    """The gate from per-tile sums against the fp64 gate of the same sums, at the tolerance of test_se_gate_vs_torch; two calls agree
    bit for bit (fixed summation order)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(n * 1000 + C + T)
    scale = 1.0 / (T * 256)
    sums = (torch.randn((n, C, T), generator=g) * 256.0 ** 0.5 + 40.0).cuda()      # tile sums of 256 outputs each
    w1 = (torch.randn((S, C, 1, 1), generator=g) / C ** 0.5).cuda(); b1 = torch.randn((S,), generator=g).cuda()
    w2 = (torch.randn((C, S, 1, 1), generator=g) / S ** 0.5).cuda(); b2 = torch.randn((C,), generator=g).cuda()
    m = sums.double().sum(2).mul(scale).view(n, C, 1, 1)
    ref = torch.sigmoid(F.conv2d(F.silu(F.conv2d(m, w1.double(), b1.double())), w2.double(), b2.double())).reshape(n, C)
    got = ops.se_gate(sums, w1, b1, w2, b2, scale=scale, tiles=T)
    again = ops.se_gate(sums, w1, b1, w2, b2, scale=scale, tiles=T)
    torch.testing.assert_close(got.cpu(), ref.float().cpu(), rtol=1e-5, atol=1e-6)
    assert torch.equal(got, again)


@pytest.mark.parametrize("C", [1, 3, 4, 64, 128, 132])
def test_layernorm_split_per_element_bound(C):
    """Input recipe (|mean| ~ 1000 std, one pixel with a negative mean) and per-element bound of
    test_layernorm_nchw_per_element_bound, which is derived for sequential sums: the fixed tree of the split kernel is tighter.
    C = 4, 64, 128 take the split kernel (1, 16 and 32 channels per wave), the others the general one; the maps are one pixel, one
    block exactly, and two sizes that end inside a 64-pixel block."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(C)
    n, eps = 2, 1e-6
    for H, W in ((1, 1), (8, 8), (5, 13), (16, 17)):
        x = (1000.0 + torch.randn((n, C, H, W), generator=g)).float()
        x[:, :, 0, 0] = -1000.0 + torch.randn((n, C), generator=g)
        gam = torch.randn((C,), generator=g).float()
        bet = torch.randn((C,), generator=g).float()
        got = ops.layernorm_nchw(x.cuda(), gam.cuda(), bet.cuda(), eps).double().cpu()
        xd = x.double()
        mean = xd.mean(1, keepdim=True)
        d = xd - mean
        var = (d * d).mean(1, keepdim=True)
        r = 1.0 / torch.sqrt(var + eps)
        gd, bd = gam.double().view(1, -1, 1, 1), bet.double().view(1, -1, 1, 1)
        ref = d * r * gd + bd
        e_m = (C + 1) * U * xd.abs().mean(1, keepdim=True)
        e_d = e_m + U * d.abs()
        e_v = (2 * (d.abs() * e_d).sum(1, keepdim=True) + (C + 2) * U * (d * d).sum(1, keepdim=True)) / C
        e_r = r * (e_v / (2 * (var + eps)) + 3 * U)
        tol = 2 * (gd.abs() * (e_d * r + d.abs() * e_r) + 3 * U * ref.abs() + U * bd.abs())
        err = (got - ref).abs()
        assert bool((err <= tol).all()), f"C={C} {H}x{W}: error {float((err / tol).max()):.3f} x the per-element bound"
