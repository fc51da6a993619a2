"""Exact-arithmetic conformance of the convolution kernels (and the LayerNorm / linear kernels around them).

Inputs, weights, biases and residuals are small integers and `in_scale` values powers of two, so every product and partial sum
is an integer (or a quarter-integer) far below 2^24: fp32 computes it exactly in ANY summation order and any K split, and a
kernel result must equal the fp64 reference BIT FOR BIT (torch.equal), not merely come close.  `_exact_bound` asserts the
fp64 bound sum|w||x| + |b| + |r| of every output element before each comparison, so a fixture cannot lose exactness unnoticed.

Output channels get weight magnitudes 0, 1 and 2 (counted from the LAST channel, which therefore always has magnitude 2) and
input pixels magnitudes 1 and 2 per float4, so a wrong zero, a misplaced channel or a dropped partial sum is visible in every
element it touches rather than hidden under a tolerance normalised by max|ref|.

Shapes are derived from the kernels' tiling constants; the case ids name the constant a case aims at:
  heal_conv1x1        K chunks of 32 channels (double-buffered on the chunk parity), Cout padded to 64 (BM), 64-pixel tiles (BN),
                      float4 pixel pieces; HEAL_C1_CFG tiles (64|128) x (64|128) x 32; split K = ceil(chunks / ceil(chunks / k))
  heal_conv3x3        chunks of 8 input channels, 64-channel m-blocks, 16-pixel-wide tiles of TH = 4 | 8 | 16 rows
  Winograd F(2x2,3x3) chunks of 8 channels, 8x16 (4 waves) or 16x16 (8 waves) pixel tiles, split K as above
  k_gconv_small       16-channel super-groups, 32 x TH (stride 1) / 16 x 8 (stride 2) output tiles
  k_depthwise         32 x 8 output tiles
Activations other than none / ReLU are compared with torch's fp32 silu / gelu on the device applied to the exact
pre-activation, within 2 ulp per element.

Part 2 (LayerNorm over channels, LayerNorm statistics feeding heal_linear) cannot be exact: those comparisons use a first-order
error bound stated per element, never a tolerance relative to the largest output."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # unit roundoff of fp32
EXACT = 2.0 ** 22              # |partial sums| stay below this: exact in fp32 with two bits to spare (quarter-integers)
POISON = 0x7FBADBAD            # a NaN bit pattern: guard words and the memory around poisoned operands
PAD = 16384                    # poisoned words on each side of an operand: 64 KiB
ACT_ULP = 2                    # SiLU / GELU: at most 2 ulp from torch's fp32 function of the exact pre-activation


def _need_experimental():
    from heal_amd import ops
    if not ops.experimental_build():
        pytest.skip("libheal_amd.so was built without HEAL_BUILD_EXPERIMENTAL=1 (measured-negative kernels are not shipped)")


def _env(monkeypatch, **kv):
    """Pin every switch that selects a kernel variant: a case states the variant it tests, nothing leaks in from outside."""
    base = {"HEAL_ARITH": None, "HEAL_C1_TILED": None, "HEAL_C1_CFG": None, "HEAL_C1_KSPLIT": "1", "HEAL_C3_ALGO": None,
            "HEAL_C3_TH": None, "HEAL_C3_KSPLIT": "1", "HEAL_WG_WAVES": None, "HEAL_WG_KC": "8", "HEAL_GCONV_MFMA": None,
            "HEAL_GS_TH": None}
    base.update(kv)
    for k, v in base.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def _bias(g, c):
    """Bias values in +-[1, 8]: never zero, so a bias that is skipped or misplaced changes every element it should reach."""
    return _ints(g, (c,), 1, 8) * (2 * _ints(g, (c,), 0, 1) - 1)


def _chan_mag(c):
    """Weight magnitude per output channel: 2, 1, 0, 2, 1, 0, ... counted backwards from the last channel."""
    return torch.tensor([(2.0, 1.0, 0.0)[(c - 1 - i) % 3] for i in range(c)])


def _pix_mag(h, w):
    """Input magnitude per pixel: 1 or 2, alternating every 4 pixels of the flattened map (one float4 piece)."""
    p = torch.arange(h * w)
    return (1.0 + (p // 4) % 2).reshape(h, w)


def _conv_weight(g, cout, cin, k, lo=-2, hi=2):
    return _ints(g, (cout, cin, k, k), lo, hi) * _chan_mag(cout).view(-1, 1, 1, 1)


def _input(g, n, c, h, w, lo=-3, hi=3):
    return _ints(g, (n, c, h, w), lo, hi) * _pix_mag(h, w)


def _exact_bound(bound, limit=EXACT):
    m = float(bound.max()) if bound.numel() else 0.0
    assert m < limit, f"fixture is not exact in fp32: an output's sum |w||x| + |b| + |r| reaches {m} >= {limit}"


def _assert_equal(got, ref, what=""):
    got = got.detach().cpu()
    ref = ref.detach().cpu().to(torch.float32)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    first = tuple(int(v) for v in idx[0])
    chans = sorted({int(v) for v in idx[:, 1]}) if got.dim() > 1 else []
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at {first}: got {float(got[first])} "
                         f"want {float(ref[first])}; channels {chans[:16]}{'...' if len(chans) > 16 else ''}")


def _ordered(t):
    """fp32 -> int64 on which neighbouring floats are 1 apart and +0 == -0."""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _assert_act(got, pre64, act, what=""):
    """act(exact pre-activation): none / ReLU bit for bit, SiLU / GELU within ACT_ULP of torch's fp32 function on the device."""
    pre = pre64.to(torch.float32)          # exact: the fixtures keep the pre-activation an fp32 number
    if act in (0, "none", None):
        return _assert_equal(got, pre, what)
    if act in (1, "relu"):
        return _assert_equal(got, torch.relu(pre), what)
    fn = F.silu if act in (2, "silu") else F.gelu
    ref = fn(pre.cuda()).cpu()
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert not torch.isnan(got).any(), f"{what}: NaN in the result"
    d = (_ordered(got) - _ordered(ref)).abs()
    assert int(d.max()) <= ACT_ULP, f"{what}: {int((d > ACT_ULP).sum())} elements more than {ACT_ULP} ulp away (max {int(d.max())})"


def _poisoned(src):
    """(backing buffer, view): src's values as a contiguous, 16-B aligned view in the middle of a NaN-filled buffer with PAD
    poisoned words on each side.  A kernel that reads past the operand reads NaN -- inside the same allocation, so the poison
    itself can never fault the device."""
    n = src.numel()
    buf = torch.full((PAD + (n + 3) // 4 * 4 + PAD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    view = buf[PAD:PAD + n].view(src.shape)
    if n:
        view.copy_(src.to(device="cuda", dtype=torch.float32))
    return buf, view


def _assert_poison_outside(buf, lo, hi, what):
    """Every word of buf outside [lo, hi) still holds the poison pattern."""
    w = buf.view(torch.int32)
    for part, name in ((w[:lo], "before"), (w[hi:], "after")):
        bad = int((part != POISON).sum())
        assert bad == 0, f"{what}: {bad} words {name} the region written"


# ================================================================================================ ops.conv1x1
def _c1_ref(x, w, b, r, s, stride):
    """fp64 pre-activation and exactness bound of act(W (s . x) + b (+ r))."""
    x = x.double().cpu()
    if s is not None:
        x = x * s.double().cpu()[:, :, None, None]
    if stride == 2:
        x = x[:, :, ::2, ::2]
    n, cin, ho, wo = x.shape
    w2 = w.double().cpu().reshape(w.shape[0], cin)
    pre = torch.einsum("oc,ncp->nop", w2, x.reshape(n, cin, -1))
    bound = torch.einsum("oc,ncp->nop", w2.abs(), x.abs().reshape(n, cin, -1))
    if b is not None:
        pre = pre + b.double().cpu().view(1, -1, 1)
        bound = bound + b.double().cpu().abs().view(1, -1, 1)
    pre, bound = pre.reshape(n, -1, ho, wo), bound.reshape(n, -1, ho, wo)
    if r is not None:
        pre, bound = pre + r.double().cpu(), bound + r.double().cpu().abs()
    return pre, bound


def _c1_operands(seed, n, cin, cout, H, W, stride=1):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = _input(g, n, cin, H, W)
    w = _conv_weight(g, cout, cin, 1)
    b = _bias(g, cout)
    r = _ints(g, (n, cout, Ho, Wo), -4, 4)
    s = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n, cin), generator=g)]
    return x, w, b, r, s


def _c1_check(x, w, b, r, s, act, stride=1, what="", out_guard=True):
    """One conv1x1 call with x / bias / residual / in_scale poisoned around and the result written into the middle of a
    poisoned buffer (`out=`): value, no write outside the result, no operand modified."""
    from heal_amd import ops
    n, cin, H, W = x.shape
    cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    pre, bound = _c1_ref(x, w, b, r, s, stride)
    _exact_bound(bound)
    bx, xv = _poisoned(x)
    ops_in = [(bx, xv, x)]
    bv = rv = sv = None
    if b is not None:
        bb, bv = _poisoned(b); ops_in.append((bb, bv, b))
    if r is not None:
        br, rv = _poisoned(r); ops_in.append((br, rv, r))
    if s is not None:
        bs, sv = _poisoned(s); ops_in.append((bs, sv, s))
    bo, ov = _poisoned(torch.empty((n, cout, Ho, Wo)))
    bo.view(torch.int32).fill_(POISON)
    got = ops.conv1x1(xv, w.cuda(), bv, rv, act, sv, stride=stride, out=ov if out_guard else None)
    if out_guard:
        assert got.data_ptr() == ov.data_ptr()
        _assert_poison_outside(bo, PAD, PAD + ov.numel(), what + " out=")
    torch.cuda.synchronize()
    for buf, view, src in ops_in:
        _assert_poison_outside(buf, PAD, PAD + view.numel(), what + " operand buffer")
        assert torch.equal(view.cpu(), src.cpu()), what + ": an operand was modified"
    _assert_act(got, pre, act, what)


# (n, Cin, Cout, H, W): Cin 4 / 31 (one partial chunk), 32 (one full chunk), 33 (one channel into a second chunk: even chunk
# count), 96 (three chunks: odd), 1152 (36 chunks); Cout 4 / 20 (part of one 64-row m-block), 64 (one block), 65 (one
# channel into a second block), 176 (2.75 blocks); HW 64 (one 64-pixel tile), 68 / 132 (one float4 past a tile), 124 (one
# float4 short of two tiles), 128 (two tiles); n 1 | 3.
_C1_SHAPES = [
    pytest.param(1, 4, 4, 8, 8, id="cin4-1chunk_cout4_hw64-1tile_n1"),
    pytest.param(3, 31, 20, 4, 17, id="cin31-1chunk_cout20_hw68-tile+f4_n3"),
    pytest.param(1, 32, 64, 4, 31, id="cin32-1chunk_cout64-1block_hw124-2tiles-f4_n1"),
    pytest.param(3, 33, 65, 8, 16, id="cin33-2chunks-even_cout65-block+1_hw128-2tiles_n3"),
    pytest.param(1, 96, 176, 12, 11, id="cin96-3chunks-odd_cout176_hw132-2tiles+f4_n1"),
    pytest.param(3, 1152, 176, 4, 17, id="cin1152-36chunks_cout176_hw68_n3"),
    pytest.param(1, 1152, 65, 4, 31, id="cin1152-36chunks_cout65_hw124_n1"),
    pytest.param(1, 4, 65, 11, 12, id="cin4_cout65_hw132_n1"),
]


@pytest.mark.parametrize("n,cin,cout,H,W", _C1_SHAPES)
def test_conv1x1_exact(n, cin, cout, H, W, monkeypatch):
    """k_conv1x1<64,64,32,1> (no K split): act 0-3, each with bias + residual + in_scale and with none of them."""
    _env(monkeypatch)
    x, w, b, r, s = _c1_operands(cin * 131 + cout * 7 + H * W + n, n, cin, cout, H, W)
    for act in (0, 1, 2, 3):
        _c1_check(x, w, b, r, s, act, what=f"act{act} all operands")
        _c1_check(x, w, None, None, None, act, what=f"act{act} bare")
    # each optional operand on its own (a path that applies one only when another is present would show here)
    _c1_check(x, w, b, None, None, 0, what="bias only")
    _c1_check(x, w, None, r, None, 0, what="residual only")
    _c1_check(x, w, None, None, s, 0, what="in_scale only")


@pytest.mark.parametrize("n,cin,cout,H,W", [
    pytest.param(3, 33, 65, 9, 15, id="s2_H9-odd_W15-odd_Wo8_cin33_cout65"),
    pytest.param(1, 96, 20, 17, 23, id="s2_H17-odd_W23-odd_Wo12_cin96-3chunks"),
    pytest.param(2, 31, 176, 8, 7, id="s2_H8_W7-odd_Wo4_cin31"),
    pytest.param(1, 1152, 64, 15, 8, id="s2_H15-odd_W8_Wo4_cin1152"),
])
def test_conv1x1_stride2_exact(n, cin, cout, H, W, monkeypatch):
    """k_conv1x1<64,64,32,2>: stride 2 on odd maps (the last input row / column is read, the one past it is not)."""
    _env(monkeypatch)
    x, w, b, r, s = _c1_operands(cin + cout + H * W, n, cin, cout, H, W, stride=2)
    for act in (0, 1, 2, 3):
        _c1_check(x, w, b, r, s, act, stride=2, what=f"s2 act{act}")
    _c1_check(x, w, None, None, None, 0, stride=2, what="s2 bare")


@pytest.mark.parametrize("n,cin,cout,H,W,stride", [
    pytest.param(3, 33, 20, 4, 17, 1, id="pm_cin33_cout20_hw68"),
    pytest.param(1, 96, 176, 12, 11, 1, id="pm_cin96_cout176_hw132"),
    pytest.param(1, 1152, 68, 4, 16, 1, id="pm_cin1152_cout68-block+4_hw64"),
    pytest.param(2, 31, 64, 9, 15, 2, id="pm_s2_cin31_cout64_Wo8"),
])
def test_conv1x1_pixel_major_exact(n, cin, cout, H, W, stride, monkeypatch):
    """Pixel-major epilogue ([n, HoWo, Cout]; float4 bias loads): act 0-2 with and without bias / in_scale."""
    from heal_amd import ops
    _env(monkeypatch)
    x, w, b, _r, s = _c1_operands(cin * 3 + cout + H, n, cin, cout, H, W, stride)
    for act in (0, 1, 2):
        for bias, scale in ((b, s), (None, None)):
            pre, bound = _c1_ref(x, w, bias, None, scale, stride)
            _exact_bound(bound)
            bx, xv = _poisoned(x)
            got = ops.conv1x1(xv, w.cuda(), None if bias is None else _poisoned(bias)[1],
                              None, act, None if scale is None else _poisoned(scale)[1], stride=stride, pixel_major=True)
            _assert_act(got, pre.flatten(2).transpose(1, 2), act, f"pixel-major act{act}")


_C1_TILES = ["64,64,32", "128,128,32", "64,128,32", "128,64,32"]     # every HEAL_C1_CFG tile conv1x1_launch instantiates


@pytest.mark.parametrize("cfg", _C1_TILES)
@pytest.mark.parametrize("n,cin,cout,H,W", [
    pytest.param(3, 33, 65, 12, 11, id="cin33_cout65-mpad128_hw132"),
    pytest.param(1, 96, 200, 4, 17, id="cin96_cout200-mpad256_hw68"),
    pytest.param(2, 1152, 128, 8, 33, id="cin1152_cout128_hw264-2x128+f4+4"),
])
def test_conv1x1_tile_configs_exact(cfg, n, cin, cout, H, W, monkeypatch):
    """HEAL_C1_CFG=bm,bn,kc: the 128-row (two m-tiles per wave) and 128-pixel (eight n-tiles per wave) variants."""
    _env(monkeypatch, HEAL_C1_CFG=cfg)
    x, w, b, r, s = _c1_operands(cin + cout * 5 + H, n, cin, cout, H, W)
    for act in (0, 3):
        _c1_check(x, w, b, r, s, act, what=f"cfg {cfg} act{act}")
    _c1_check(x, w, None, None, None, 1, what=f"cfg {cfg} bare")


def _legal_ksplits(chunks):
    """Every ksplit in [2, chunks] heal_conv1x1_splitk accepts: no empty split, i.e. (k - 1) * ceil(chunks / k) < chunks."""
    return [k for k in range(2, chunks + 1) if (k - 1) * -(-chunks // k) < chunks]


_KSPLIT_CASES = ([pytest.param(1, 1152, 65, 4, 17, k, id=f"cin1152-36chunks_ksplit{k}-{'equal' if 36 % k == 0 else 'unequal'}")
                  for k in _legal_ksplits(36)]
                 + [pytest.param(3, 96, 176, 12, 11, k, id=f"cin96-3chunks_ksplit{k}-{'equal' if 3 % k == 0 else 'unequal'}")
                    for k in _legal_ksplits(3)])


@pytest.mark.parametrize("n,cin,cout,H,W,ksplit", _KSPLIT_CASES)
def test_conv1x1_split_k_exact(n, cin, cout, H, W, ksplit, monkeypatch):
    """Split K (k_conv1x1 partials + k_conv1x1_splitk_reduce, which applies bias / residual / act 0-3) for every legal split of
    a deep and a shallow reduction, unequal last splits included."""
    from heal_amd import ops
    _env(monkeypatch, HEAL_C1_KSPLIT=ksplit)
    assert ops.conv1x1_ksplit(n, cin, cout, H * W) == ksplit     # the case runs the split it names
    x, w, b, r, s = _c1_operands(ksplit * 17 + cin, n, cin, cout, H, W)
    for act in (0, 1, 2, 3):
        _c1_check(x, w, b, r, s, act, what=f"ksplit {ksplit} act{act}")
    _c1_check(x, w, None, None, None, 3, what=f"ksplit {ksplit} bare act3")


@pytest.mark.parametrize("n,cin,C,H,W,k,ctot,off", [
    pytest.param(2, 33, 20, 5, 16, 1, 29, 7, id="k1_cin33_C20_off7_of29"),
    pytest.param(1, 96, 17, 3, 12, 2, 40, 20, id="k2_cin96_Cout68_off20_of40"),
    pytest.param(2, 31, 5, 4, 8, 4, 13, 3, id="k4_cin31_Cout80_off3_of13"),
    pytest.param(1, 1152, 9, 4, 4, 2, 10, 1, id="k2_cin1152_Cout36_off1_of10"),
])
def test_conv1x1_d2s_exact_and_writes_only_its_slice(n, cin, C, H, W, k, ctot, off, monkeypatch):
    """conv1x1_d2s (out_pm = 2): depth-to-space into channels [off, off + C) of dst; every other channel of dst and every word
    around it keeps its poison."""
    from heal_amd import ops
    _env(monkeypatch)
    cout = C * k * k
    x, w, b, _r, _s = _c1_operands(cin + C * 11 + k, n, cin, cout, H, W)
    for act in (0, 1, 2, 3):
        for bias in (b, None):
            pre, bound = _c1_ref(x, w, bias, None, None, 1)
            _exact_bound(bound)
            ref = F.pixel_shuffle(pre, k) if k > 1 else pre                       # [n, C, H k, W k]
            bx, xv = _poisoned(x)
            bb, bv = _poisoned(bias) if bias is not None else (None, None)
            bd, dst = _poisoned(torch.empty((n, ctot, H * k, W * k)))
            bd.view(torch.int32).fill_(POISON)
            got = ops.conv1x1_d2s(xv, w.cuda(), bv, act, k, dst, off)
            _assert_act(got, ref, act, f"d2s k{k} act{act}")
            inside = torch.zeros((n, ctot, H * k, W * k), dtype=torch.bool)
            inside[:, off:off + C] = True
            d = dst.view(torch.int32).cpu()
            assert bool((d[~inside] == POISON).all()), f"d2s k{k}: a channel outside [{off}, {off + C}) was written"
            _assert_poison_outside(bd, PAD, PAD + dst.numel(), f"d2s k{k} dst buffer")
            _assert_poison_outside(bx, PAD, PAD + xv.numel(), f"d2s k{k} x buffer")
            if bb is not None:
                _assert_poison_outside(bb, PAD, PAD + bv.numel(), f"d2s k{k} bias buffer")


# ================================================================================================ ops.conv3x3
def _conv_ref(x, w, b, r, stride, pad, groups=1):
    """fp64 conv2d (explicit (left, right, top, bottom) zero padding) and its exactness bound, on the host."""
    xd = F.pad(x.double().cpu(), pad)
    wd = w.double().cpu()
    pre = F.conv2d(xd, wd, None, stride, 0, 1, groups)
    bound = F.conv2d(xd.abs(), wd.abs(), None, stride, 0, 1, groups)
    if b is not None:
        pre = pre + b.double().cpu().view(1, -1, 1, 1)
        bound = bound + b.double().cpu().abs().view(1, -1, 1, 1)
    if r is not None:
        pre, bound = pre + r.double().cpu(), bound + r.double().cpu().abs()
    return pre, bound


def _winograd_bound(x, w, b, r):
    """F(2x2,3x3) keeps quarter-integers (U = G g G^T holds multiples of 1/4, the input / output transforms are +-1 sums): exact
    while 4 x (the largest Winograd-domain partial sum) < 2^24.  |V| <= 4 max|x|, a Winograd-domain sum <= Cin max|U| |V|, an
    output <= 9 of them (+ |b| + |r|)."""
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Uw = (G @ w.double().cpu() @ G.t()).abs().amax(dim=(2, 3)).sum(1)                         # [Cout]: sum_ci max|U|
    m = 9 * Uw.max() * 4 * x.abs().max().double()
    m = m + (b.abs().max().double() if b is not None else 0) + (r.abs().max().double() if r is not None else 0)
    return m.view(1)


def _c3_operands(seed, n, cin, cout, H, W, stride):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (_input(g, n, cin, H, W), _conv_weight(g, cout, cin, 3), _bias(g, cout), _ints(g, (n, cout, Ho, Wo), -4, 4))


# maps 15/16/17 x 31/32/33 and 7 x 9 (16-pixel tile columns, 4/8/16-row direct tiles, 8/16-row Winograd tiles);
# Cin 3 / 9 / 67 (partial 8-channel chunks) and 8 (one exact chunk); Cout 20 / 64 / 65 / 130 (64-channel m-blocks)
_C3_SHAPES = [
    pytest.param(1, 3, 20, 15, 31, id="cin3_cout20_15x31"),
    pytest.param(2, 8, 64, 16, 32, id="cin8-1chunk_cout64_16x32"),
    pytest.param(1, 9, 65, 17, 33, id="cin9-chunk+1_cout65-block+1_17x33"),
    pytest.param(2, 67, 130, 7, 9, id="cin67_cout130-2blocks+2_7x9"),
    pytest.param(1, 67, 20, 17, 31, id="cin67_cout20_17x31"),
    pytest.param(1, 8, 130, 15, 33, id="cin8_cout130_15x33"),
]
# kernel variant: direct k_conv3x3<STRIDE, TH> for every instantiated (STRIDE, TH); Winograd k_conv3x3_wino<waves, exact, 8>
# (exact = Cin % 8 == 0: the shapes above take both)
_C3_VARIANTS = ["direct_s1_th4", "direct_s1_th8", "direct_s1_th16", "direct_s2_th4", "direct_s2_th8", "winograd_w4", "winograd_w8"]


def _c3_env(monkeypatch, variant):
    if variant.startswith("direct"):
        _env(monkeypatch, HEAL_C3_ALGO="direct", HEAL_C3_TH=variant.rsplit("th", 1)[1])
        return int(variant.split("_s")[1][0])
    _env(monkeypatch, HEAL_C3_ALGO="winograd", HEAL_WG_WAVES=variant[-1], HEAL_WG_KC="8", HEAL_C3_KSPLIT="1")
    return 1


@pytest.mark.parametrize("variant", _C3_VARIANTS)
@pytest.mark.parametrize("n,cin,cout,H,W", _C3_SHAPES)
def test_conv3x3_exact(n, cin, cout, H, W, variant, monkeypatch):
    from heal_amd import ops
    stride = _c3_env(monkeypatch, variant)
    x, w, b, r = _c3_operands(cin * 17 + cout + H * W + stride, n, cin, cout, H, W, stride)
    for bias, res, relu in ((b, r, False), (b, r, True), (None, None, False), (b, None, True)):
        pre, bound = _conv_ref(x, w, bias, res, stride, (1, 1, 1, 1))
        _exact_bound(bound)
        if variant.startswith("winograd"):
            _exact_bound(4 * _winograd_bound(x, w, bias, res), 2.0 ** 24)
        got = ops.conv3x3(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), None if res is None else res.cuda(),
                          relu, stride)
        _assert_act(got, pre, 1 if relu else 0, f"{variant} bias={bias is not None} res={res is not None} relu={relu}")


@pytest.mark.parametrize("waves,ksplit", [pytest.param(4, k, id=f"w4_cin256-32chunks_ksplit{k}") for k in _legal_ksplits(32)]
                         + [pytest.param(8, k, id=f"w8_cin256-32chunks_ksplit{k}") for k in (2, 5, 32)])
def test_conv3x3_winograd_split_k_exact(waves, ksplit, monkeypatch):
    """Winograd split K (partials + the shared k_conv1x1_splitk_reduce) for every legal HEAL_C3_KSPLIT of a 256-channel
    reduction (32 chunks of 8)."""
    from heal_amd import ops
    _env(monkeypatch, HEAL_C3_ALGO="winograd", HEAL_WG_WAVES=waves, HEAL_C3_KSPLIT=ksplit)
    n, cin, cout, H, W = 1, 256, 65, 12, 16
    assert ops.conv3x3_winograd_ksplit(n, cin, cout, H, W, waves) == ksplit
    x, w, b, r = _c3_operands(ksplit + 7 * waves, n, cin, cout, H, W, 1)
    for bias, res, relu in ((b, r, True), (None, None, False)):
        pre, bound = _conv_ref(x, w, bias, res, 1, (1, 1, 1, 1))
        _exact_bound(bound)
        _exact_bound(4 * _winograd_bound(x, w, bias, res), 2.0 ** 24)
        got = ops.conv3x3(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), None if res is None else res.cuda(), relu, 1)
        _assert_act(got, pre, 1 if relu else 0, f"winograd w{waves} ksplit {ksplit}")


@pytest.mark.parametrize("n,cin,cout,H,W", [pytest.param(2, 16, 65, 17, 33, id="cin16_cout65_17x33"),
                                            pytest.param(1, 32, 130, 7, 9, id="cin32_cout130_7x9")])
def test_conv3x3_winograd_kc16_exact(n, cin, cout, H, W, monkeypatch):
    """Experimental 16-channel chunks (k_conv3x3_wino<8, true, 16>): the same F(2x2,3x3) arithmetic, so bit for bit too."""
    _need_experimental()
    from heal_amd import ops
    _env(monkeypatch, HEAL_C3_ALGO="winograd", HEAL_WG_WAVES="8", HEAL_WG_KC="16")
    x, w, b, r = _c3_operands(cin + cout, n, cin, cout, H, W, 1)
    pre, bound = _conv_ref(x, w, b, r, 1, (1, 1, 1, 1))
    _exact_bound(bound)
    _exact_bound(4 * _winograd_bound(x, w, b, r), 2.0 ** 24)
    _assert_act(ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), r.cuda(), True, 1), pre, 1, "winograd kc16")


@pytest.mark.parametrize("n,cin,cout,H,W", [pytest.param(2, 16, 65, 17, 33, id="cin16_cout65_17x33"),
                                            pytest.param(1, 67, 20, 7, 9, id="cin67_cout20_7x9")])
def test_conv3x3_winograd4_per_element_bound(n, cin, cout, H, W, monkeypatch):
    """Experimental F(4x4,3x3) cannot be exact: its filter transform holds sixths and twenty-fourths, which fp32 rounds.  Each
    output is held to a first-order bound of its own terms instead: 64 u sum|w||x| (the transforms add at most 6 x 6 terms
    of magnitude <= 1 per product, each rounding at most u) + u (|b| + |r|) for the epilogue."""
    _need_experimental()
    from heal_amd import ops
    _env(monkeypatch, HEAL_C3_ALGO="winograd4")
    x, w, b, r = _c3_operands(cin + cout + 4, n, cin, cout, H, W, 1)
    pre, bound = _conv_ref(x, w, b, r, 1, (1, 1, 1, 1))
    got = ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), r.cuda(), False, 1).double().cpu()
    err = (got - pre).abs()
    tol = 64 * U * bound + 2 * U * pre.abs()
    assert bool((err <= tol).all()), f"F(4x4) error {float((err / tol).max()):.3f} x the per-element bound"


# ================================================================================================ ops.grouped_conv3x3
# HEAL_GCONV_MFMA: 1 = k_gconv_small (":th8" / ":th16" = HEAL_GS_TH, reaching k_gconv_small<4,8,1> and <8,16,1>), 16 / 8 = the
# 16x16x4 kernel (stride 1; cg 16, and cg 8 paired), 0 = the vector-ALU stencil.  The maps give output widths that are not a
# multiple of the 32-wide (stride 1) / 16-wide (stride 2) tile, heights that are not a multiple of the 8 / 16 rows, and
# W % 4 != 0 (7 x 10 / 9 x 14: every mode falls back to the stencil).
_GC_MAPS = {1: [(9, 36), (17, 8), (7, 10)], 2: [(11, 24), (8, 40), (9, 14)]}


def _gconv_kernel(cg, stride, mode):
    """The kernel grouped_conv3x3 launches for a W % 4 == 0 map (the case id names it)."""
    m, _, th = mode.partition(":th")
    if m == "1":
        t = int(th) if th else (16 if cg == 4 and stride == 1 else 8)
        return f"k_gconv_small<{cg},{8 if stride == 2 or cg == 16 else t},{stride}>"
    if stride == 1 and (cg == 16 and m != "0" or cg == 8 and m == "8"):
        return "k_grouped16_conv3x3"
    return "stencil"


_GC_CASES = [pytest.param(cg, stride, mode, id=f"cg{cg}_s{stride}_mfma{mode}_{_gconv_kernel(cg, stride, mode)}")
             for cg in (4, 8, 16) for stride in (1, 2) for mode in ("1", "1:th8", "1:th16", "16", "8", "0")]


@pytest.mark.parametrize("cg,stride,mode", _GC_CASES)
def test_grouped_conv3x3_exact(cg, stride, mode, monkeypatch):
    from heal_amd import ops
    m, _, th = mode.partition(":th")
    _env(monkeypatch, HEAL_GCONV_MFMA=m, HEAL_GS_TH=th or None)
    C = 64
    g = torch.Generator().manual_seed(cg * 10 + stride)
    w = _conv_weight(g, C, cg, 3)
    b = _bias(g, C)
    for H, W in _GC_MAPS[stride]:
        x = _input(g, 2, C, H, W)
        for bias, relu in ((b, True), (None, False)):
            pre, bound = _conv_ref(x, w, bias, None, stride, (1, 1, 1, 1), C // cg)
            _exact_bound(bound)
            got = ops.grouped_conv3x3(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), C // cg, stride, relu)
            _assert_act(got, pre, 1 if relu else 0, f"cg{cg} s{stride} mode {mode} {H}x{W} relu={relu}")


# ================================================================================================ ops.depthwise_conv
@pytest.mark.parametrize("k,stride,pad", [
    pytest.param(3, 1, (1, 1, 1, 1), id="k3_s1_sym"), pytest.param(3, 1, (0, 1, 1, 0), id="k3_s1_asym"),
    pytest.param(3, 2, (0, 1, 0, 1), id="k3_s2_asym"), pytest.param(5, 1, (2, 1, 0, 2), id="k5_s1_asym"),
    pytest.param(5, 2, (1, 2, 2, 1), id="k5_s2_asym"), pytest.param(7, 1, (3, 2, 1, 3), id="k7_s1_asym"),
])
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_depthwise_conv_exact_with_channel_sums(k, stride, pad, act):
    """k_depthwise<K, STRIDE> for every instantiation, on maps spanning partial 32 x 8 tiles; the per-tile channel sums are
    integer sums too (bit for bit) except after SiLU, where each tile's sum is held to its own bound 8 u sum|y| (a depth-8
    reduction tree) around the fp64 sum of the kernel's outputs."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(k * 10 + stride)
    n, C = 2, 5
    for H, W in ((13, 37), (17, 70)):
        x = _input(g, n, C, H, W)
        w = _ints(g, (C, 1, k, k), -2, 2) * _chan_mag(C).view(-1, 1, 1, 1)
        b = _bias(g, C)
        pre, bound = _conv_ref(x, w, b, None, stride, pad, C)
        _exact_bound(bound)
        y, sums = ops.depthwise_conv(x.cuda(), w.cuda(), b.cuda(), stride, pad, act, channel_sums=True)
        _assert_act(y, pre, act, f"k{k} s{stride} {act} {H}x{W}")
        Ho, Wo = pre.shape[2:]
        ty, tx = -(-Ho // 8), -(-Wo // 32)
        yv = y.double().cpu() if act == "silu" else (torch.relu(pre) if act == "relu" else pre)
        tiles = F.pad(yv, (0, tx * 32 - Wo, 0, ty * 8 - Ho)).reshape(n, C, ty, 8, tx, 32)
        want = tiles.sum(dim=(3, 5)).reshape(n, C, ty * tx)
        if act == "silu":
            tol = 8 * U * tiles.abs().sum(dim=(3, 5)).reshape(n, C, ty * tx)
            assert bool(((sums.double().cpu() - want).abs() <= tol).all()), "depthwise channel sums beyond 8 u sum|y|"
        else:
            _assert_equal(sums, want, f"k{k} s{stride} {act} channel sums")
        y2 = ops.depthwise_conv(x.cuda(), w.cuda(), None, stride, pad, "none")
        _assert_equal(y2, _conv_ref(x, w, None, None, stride, pad, C)[0], f"k{k} s{stride} no bias")


def test_depthwise_conv_7x7_stride2_is_an_error():
    """k_depthwise<7, 2> is not instantiated: the call must fail, not fall back."""
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    x = torch.zeros((1, 4, 16, 16), device="cuda")
    with pytest.raises(HealAmdError, match="not instantiated"):
        ops.depthwise_conv(x, torch.zeros((4, 1, 7, 7), device="cuda"), None, 2, (3, 3, 3, 3))


# ================================================================================================ the other dense convolutions
@pytest.mark.parametrize("n,cin,cout,H,W,ks,stride", [
    pytest.param(2, 32, 128, 9, 16, 3, 1, id="3x3_s1_cin32_cout128_Wo16"),
    pytest.param(1, 64, 256, 17, 15, 3, 2, id="3x3_s2_cin64_cout256_Wo8_odd"),
    pytest.param(1, 32, 128, 33, 4, 3, 1, id="3x3_s1_Wo4-narrowest-tile"),
    pytest.param(1, 32, 128, 5, 12, 1, 1, id="1x1_s1_cin32_Wo12"),
    pytest.param(2, 64, 128, 9, 23, 1, 2, id="1x1_s2_cin64_Wo12_odd"),
])
def test_conv_gemm_exact(n, cin, cout, H, W, ks, stride):
    """heal_conv_gemm (128 x 128 x 32 implicit GEMM) at the shapes conv_gemm_supported accepts plus the narrowest pixel tile."""
    from heal_amd import ops
    assert ops.conv_gemm_supported(cin, cout, (W - 1) // stride + 1)
    g = torch.Generator().manual_seed(cin + cout + H + ks)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, w = _input(g, n, cin, H, W), _conv_weight(g, cout, cin, ks)
    b, r = _bias(g, cout), _ints(g, (n, cout, Ho, Wo), -4, 4)
    p = ks // 2
    for bias, res, relu in ((b, r, True), (b, r, False), (None, None, False)):
        pre, bound = _conv_ref(x, w, bias, res, stride, (p, p, p, p))
        _exact_bound(bound)
        got = ops.conv_gemm(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), None if res is None else res.cuda(),
                            relu, stride)
        _assert_act(got, pre, 1 if relu else 0, f"conv_gemm {ks}x{ks}/{stride} relu={relu}")


@pytest.mark.parametrize("n,cin,cout,H,W", [pytest.param(1, 32, 64, 15, 15, id="cout64_Wo8_odd"),
                                            pytest.param(2, 32, 128, 20, 7, id="cout128_Wo4"),
                                            pytest.param(1, 64, 100, 9, 16, id="cout100-padded")])
def test_conv7x7_s2_exact(n, cin, cout, H, W):
    from heal_amd import ops
    assert ops.conv7x7_s2_supported(cin, cout, W)
    g = torch.Generator().manual_seed(cin + cout + H)
    x, w, b = _input(g, n, cin, H, W, -2, 2), _conv_weight(g, cout, cin, 7, -1, 1), _bias(g, cout)
    for bias, relu in ((b, True), (None, False)):
        pre, bound = _conv_ref(x, w, bias, None, 2, (3, 3, 3, 3))
        _exact_bound(bound)
        got = ops.conv7x7_s2(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), relu)
        _assert_act(got, pre, 1 if relu else 0, f"conv7x7_s2 relu={relu}")


@pytest.mark.parametrize("n,cx,cin,H,W", [pytest.param(2, 4, 1, 37, 50, id="cin1-ks13"), pytest.param(1, 3, 2, 20, 17, id="cin2-ks25"),
                                          pytest.param(2, 4, 3, 37, 50, id="cin3-ks37_cx4"), pytest.param(1, 4, 4, 15, 9, id="cin4-ks49")])
@pytest.mark.parametrize("pool", [True, False])
def test_stem7x7_exact(n, cx, cin, H, W, pool):
    """heal_stem7x7 for every instantiated k-step count (Cin 1-4): relu(conv7x7/2 + b) (+ 3x3/2 max-pool), bit for bit."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin * 100 + H)
    x, w, b = _input(g, n, cx, H, W), _conv_weight(g, 64, cin, 7), _bias(g, 64)
    pre, bound = _conv_ref(x[:, :cin], w, b, None, 2, (3, 3, 3, 3))
    _exact_bound(bound)
    ref = torch.relu(pre)
    if pool:
        ref = F.max_pool2d(ref, 3, 2, 1)
    _assert_equal(ops.stem7x7(x.cuda(), w.cuda(), b.cuda(), pool), ref, f"stem7x7 cin{cin} pool={pool}")


@pytest.mark.parametrize("n,cin,cout,H,W,stride,pad", [
    pytest.param(2, 3, 20, 17, 33, 2, (0, 1, 0, 1), id="s2_pad0101_cin3"),
    pytest.param(1, 9, 65, 16, 31, 2, (1, 1, 0, 1), id="s2_pad1101_cout65"),
    pytest.param(1, 8, 130, 15, 16, 1, (1, 1, 1, 1), id="s1_pad1111_cout130"),
    pytest.param(2, 67, 20, 7, 9, 1, (0, 1, 1, 0), id="s1_pad0110_cin67"),
])
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_conv3x3_same_exact(n, cin, cout, H, W, stride, pad, act):
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin + cout + H + stride)
    x, w, b = _input(g, n, cin, H, W), _conv_weight(g, cout, cin, 3), _bias(g, cout)
    pre, bound = _conv_ref(x, w, b, None, stride, pad)
    _exact_bound(bound)
    _assert_act(ops.conv3x3_same(x.cuda(), w.cuda(), b.cuda(), stride, pad, act), pre, act, f"conv3x3_same {pad} {act}")


# ================================================================================================ heal_linear (exact)
@pytest.mark.parametrize("T,K,N", [pytest.param(100, 32, 128, id="T100-ragged_K32_N128"),
                                   pytest.param(257, 96, 256, id="T257_K96_N256"),
                                   pytest.param(64, 1152, 384, id="T64_K1152_N384")])
@pytest.mark.parametrize("act", [None, "relu", "gelu"])
def test_linear_exact(T, K, N, act):
    """heal_linear without LayerNorm statistics on integer fixtures: act(x W^T + b) + r bit for bit (GELU within ACT_ULP)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(T + K + N)
    x = _ints(g, (T, K), -3, 3)
    w = _ints(g, (N, K), -2, 2) * _chan_mag(N).view(-1, 1)
    b, r = _bias(g, N), _ints(g, (T, N), -4, 4)
    pre = x.double() @ w.double().t() + b.double()
    _exact_bound(x.double().abs() @ w.double().abs().t() + b.double().abs() + r.double().abs())
    for res in (r, None):
        got = ops.linear(x.cuda(), w.cuda(), b.cuda(), act=act, residual=None if res is None else res.cuda())
        if res is None:
            _assert_act(got, pre, {None: 0, "relu": 1, "gelu": 3}[act], f"linear {act}")
        elif act == "gelu":
            # the residual is added after the activation: ACT_ULP ulp (<= 2 u each) of gelu, then one rounding of the sum
            gl = F.gelu(pre.float().cuda()).cpu().double()
            ref = gl + res.double()
            tol = 2 * ACT_ULP * U * gl.abs() + U * ref.abs() + 2.0 ** -126
            assert bool(((got.cpu().double() - ref).abs() <= tol).all()), "linear gelu + residual beyond its bound"
        else:   # integers throughout: the residual subtracts exactly
            _assert_act(got.cpu() - res, pre, {None: 0, "relu": 1}[act], f"linear {act} + residual")


# ================================================================================================ part 2: per-element bounds
@pytest.mark.parametrize("C", [1, 3, 64, 96, 768])
def test_layernorm_nchw_per_element_bound(C):
    """heal_layernorm_nchw (two passes over the channels, one thread per pixel) on n = 3 maps of 13 x 23 pixels (not a multiple
    of the 256-pixel block) whose channel mean is far larger than their spread (|mean| ~ 1000 std): a one-pass variance would
    cancel catastrophically here.  First-order bound of every output, from the fp32 operation sequence of the kernel:
      mean:      e_m  = (C + 1) u mean|x|                     (C - 1 sequential additions and a division)
      x - mean:  e_d  = e_m + u |d|
      variance:  e_v  = (2 sum_c |d_c| e_d,c + (C + 2) u sum_c d_c^2) / C,   rstd: e_r / r = e_v / (2 (var + eps)) + 3 u
      output:    e_y  = |g| (e_d r + |d| e_r) + 3 u |y| + u |b|,  doubled for the second-order terms."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(C)
    n, H, W, eps = 3, 13, 23, 1e-6
    x = (1000.0 + torch.randn((n, C, H, W), generator=g)).float()
    x[:, :, 0, 0] = -1000.0 + torch.randn((n, C), generator=g)          # a pixel with a negative mean
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
    assert bool((err <= tol).all()), f"C={C}: error {float((err / tol).max()):.3f} x the per-element bound"


@pytest.mark.parametrize("T,K,N", [(100, 64, 128), (257, 256, 256), (64, 512, 384)])
def test_linear_layernorm_stats_per_element_bound(T, K, N):
    """ln_stats (mean, rstd per token; wave-tree sums) feeding heal_linear's prologue ((x - mean) rstd, then the fp32 GEMM), on
    tokens with |mean| >> std.  The statistics are checked against fp64 within e_m = (K + 8) u mean|x| and a relative
    e_r = e_v / (2 (var + eps)) + 3 u (e_v as in the LayerNorm test); each output within
      2 (r sum_k |W_nk| (e_m + u |d_k|) + |d|.|W_n| e_r + (K + 4) u sum_k |d_k| r |W_nk| + 2 u |b_n|)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(T + K)
    eps = 1e-5
    x = (50.0 + 0.5 * torch.randn((T, K), generator=g)).float()
    w = (torch.randn((N, K), generator=g) / K ** 0.5).float()
    b = torch.randn((N,), generator=g).float()
    stats = ops.ln_stats(x.cuda(), eps)
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    e_m = (K + 8) * U * xd.abs().mean(1, keepdim=True)
    e_d = e_m + U * d.abs()
    e_v = (2 * (d.abs() * e_d).sum(1, keepdim=True) + (K + 8) * U * (d * d).sum(1, keepdim=True)) / K
    rel_r = e_v / (2 * (var + eps)) + 3 * U
    st = stats.double().cpu()
    assert bool(((st[:, :1] - mean).abs() <= e_m).all()), "ln_stats mean beyond its bound"
    assert bool(((st[:, 1:] - r).abs() <= r * rel_r).all()), "ln_stats rstd beyond its bound"
    got = ops.linear(x.cuda(), w.cuda(), b.cuda(), stats=stats).double().cpu()
    wd, bd = w.double(), b.double()
    ref = (d * r) @ wd.t() + bd
    tol = 2 * (r * (e_d @ wd.abs().t()) + (d.abs() @ wd.abs().t()) * r * rel_r
               + (K + 4) * U * ((d.abs() * r) @ wd.abs().t()) + 2 * U * bd.abs())
    err = (got - ref).abs()
    assert bool((err <= tol).all()), f"error {float((err / tol).max()):.3f} x the per-element bound"


# ================================================================================================ part 3: operand checks
def _bias_cases():
    """(id, cout, call(bias) -> result): every wrapper / branch that takes a per-output-channel bias."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(5)
    x1 = _input(g, 2, 96, 8, 16).cuda()
    w1 = _conv_weight(g, 20, 96, 1).cuda()
    w128 = _conv_weight(g, 128, 96, 1).cuda()
    x3 = _input(g, 1, 64, 9, 16).cuda()
    w3 = _conv_weight(g, 20, 64, 3).cuda()
    wg = _conv_weight(g, 64, 8, 3).cuda()
    wd = _ints(g, (64, 1, 3, 3), -2, 2).cuda()
    xg = _input(g, 1, 32, 12, 16).cuda()
    wcg = _conv_weight(g, 128, 32, 3).cuda()
    w7 = _conv_weight(g, 64, 32, 7, -1, 1).cuda()
    xs = _input(g, 1, 3, 20, 24).cuda()
    ws = _conv_weight(g, 64, 3, 7).cuda()

    def env(**kv):
        def wrap(fn):
            def run(bias, mp):
                _env(mp, **kv)
                return fn(bias)
            return run
        return wrap
    return [
        ("conv1x1-nchw", 20, env()(lambda b: ops.conv1x1(x1, w1, b, None, 1))),
        ("conv1x1-splitk", 20, env(HEAL_C1_KSPLIT=2)(lambda b: ops.conv1x1(x1, w1, b, None, 3))),
        ("conv1x1-pixel-major", 20, env()(lambda b: ops.conv1x1(x1, w1, b, None, 1, pixel_major=True))),
        ("conv1x1-split-bf16", 128, env(HEAL_ARITH="bf16x6")(lambda b: ops.conv1x1(x1, w128, b, None, 1))),
        ("conv1x1-tiled", 128, env(HEAL_C1_TILED="force")(lambda b: ops.conv1x1(x1, w128, b, None, 1))),
        ("conv1x1_d2s", 20, env()(lambda b: ops.conv1x1_d2s(x1, w1, b, 1, 2, torch.zeros((2, 9, 16, 32), device="cuda"), 2))),
        ("grouped_conv3x3-small", 64, env(HEAL_GCONV_MFMA="1")(lambda b: ops.grouped_conv3x3(x3, wg, b, 8, 1))),
        ("grouped_conv3x3-16x16x4", 64, env(HEAL_GCONV_MFMA="8")(lambda b: ops.grouped_conv3x3(x3, wg, b, 8, 1))),
        ("grouped_conv3x3-stencil", 64, env(HEAL_GCONV_MFMA="0")(lambda b: ops.grouped_conv3x3(x3, wg, b, 8, 1))),
        ("depthwise_conv", 64, env()(lambda b: ops.depthwise_conv(x3, wd, b, 1, (1, 1, 1, 1)))),
        ("conv3x3-direct", 20, env(HEAL_C3_ALGO="direct")(lambda b: ops.conv3x3(x3, w3, b))),
        ("conv3x3-winograd", 20, env(HEAL_C3_ALGO="winograd")(lambda b: ops.conv3x3(x3, w3, b))),
        ("conv3x3_same", 20, env()(lambda b: ops.conv3x3_same(x3, w3, b, 2, (0, 1, 0, 1)))),
        ("conv_gemm", 128, env()(lambda b: ops.conv_gemm(xg, wcg, b))),
        ("conv7x7_s2", 64, env()(lambda b: ops.conv7x7_s2(xg, w7, b))),
        ("stem7x7", 64, env()(lambda b: ops.stem7x7(xs, ws, b))),
    ]


_BIAS_IDS = ["conv1x1-nchw", "conv1x1-splitk", "conv1x1-pixel-major", "conv1x1-split-bf16", "conv1x1-tiled", "conv1x1_d2s",
             "grouped_conv3x3-small", "grouped_conv3x3-16x16x4", "grouped_conv3x3-stencil", "depthwise_conv", "conv3x3-direct",
             "conv3x3-winograd", "conv3x3_same", "conv_gemm", "conv7x7_s2", "stem7x7"]


def _bias_case(name):
    if name == "conv1x1-tiled":
        _need_experimental()
    return next((c, fn) for i, c, fn in _bias_cases() if i == name)


@pytest.mark.parametrize("name", _BIAS_IDS)
def test_bias_strided_view_equals_contiguous_copy(name, monkeypatch):
    """A strided bias view (every other element of a 2C buffer: only ever read inside its own allocation) gives the result of
    its contiguous copy, bit for bit."""
    cout, fn = _bias_case(name)
    strided = (torch.arange(2 * cout, dtype=torch.float32, device="cuda") - cout)[::2]
    assert not strided.is_contiguous()
    want = fn(strided.contiguous(), monkeypatch).clone()
    got = fn(strided, monkeypatch)
    _assert_equal(got, want, f"{name}: strided bias")


@pytest.mark.parametrize("name", _BIAS_IDS)
def test_bias_wrong_dtype_or_length_is_an_error(name, monkeypatch):
    """A float64 bias (twice the bytes a f32 one has) and a bias longer than Cout raise HealAmdError instead of being misread."""
    from heal_amd._capi import HealAmdError
    cout, fn = _bias_case(name)
    with pytest.raises(HealAmdError, match="bias"):
        fn(torch.ones((cout,), dtype=torch.float64, device="cuda"), monkeypatch)
    with pytest.raises(HealAmdError, match="bias"):
        fn(torch.ones((cout + 4,), dtype=torch.float32, device="cuda"), monkeypatch)
