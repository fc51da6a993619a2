"""Float64 reference, per-element error bound, launch-layout restatements and hand-built fixtures of the K5 FORWARD conformance
suite (tests/test_gpu_k5_forward_conformance.py): k_warp_fuse<n>, k_warp_fuse_lds<n>, k_warp_agent<16>, k_fuse_warped and
k_warp_agents_pm of heal_amd/csrc/warp_fuse.hip -- numpy only, so that tests/test_k5_forward_refs_cpu.py can prove all of it on a
machine without a GPU.

Per ego pixel p the fused kernels compute
    score = (sigmoid(occ) + 1e-4f) * keep,   S_a = sum_k t_ak score_a[off_ak],   S == 0 -> -inf,   prob = softmax_a(S) (all masked: 0),
    X_a[c] = sum_k t_ak x[a, c, off_ak],     out[c] = sum_a prob_a X_a[c].
The taps (offsets and fp32 corner weights t) come from backward_refs.k5_taps, which forms them with the kernel's own fp32
operations, so they carry no error; everything after them is evaluated here in float64 and a kernel is held to
    |got - ref| <= k * EPS * T + TINY                       on every element,     T[c] = sum_a prob_a * (the sample of |x|)[a, c],
with k from k5_forward_k and the conventions of tests/backward_refs.py (EPS = 2^-24 per rounding, expf = 4 EPS, the library is
built with -ffp-contract=off).  Nothing is divided by a tensor-wide maximum.  Where fp32 computes without rounding (probabilities
0 / 1 or 1 / 2^j on dyadic data) the comparison is bit for bit."""
import numpy as np

from tests.backward_refs import (EPS, EXACT_LIMIT, F32, FAR, TINY, k5_collision, k5_exact_translation, k5_keep,      # noqa: F401
                                 k5_taps, max_ratio, shift_rows)
from tests.coalign_refs import IDENTITY, _gather, rotation_rows, sample_f32, sample_f64      # noqa: F401

OFFSET = float(F32(1e-4))          # the kernel adds the float32 constant 1e-4f
SATURATED = (-100.0, -30.0, -12.0, -6.0, -1.0, 0.0, 1.0, 6.0, 12.0, 30.0, 100.0)


# =====================================================================================================================
# the reference
# =====================================================================================================================
def _softmax_masked(S, mask_zero=True):
    """softmax over axis 0 with the reference's rules: S == 0 -> -inf, a column of -inf -> weights 0."""
    Sm = np.where(S == 0, -np.inf, S) if mask_zero else S
    mx = Sm.max(0, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(Sm - np.where(np.isfinite(mx), mx, 0.0))
    den = e.sum(0, keepdims=True)
    return np.where(den > 0, e / np.where(den > 0, den, 1.0), 0.0)


def k5_forward(feats, occ, rows, crop=None, grid_f64=True, *, offset=OFFSET, mask_zero=True, taps=None):
    """The float64 forward on the fp32 taps of k5_taps.  feats [n,C,H,W], occ [n,1,H,W] logits, rows [n,2,3], crop: per agent
    (h0,h1,w0,w1) or None (k5_keep's convention) -> dict
      out [C,H,W], T [C,H,W] = sum_a prob_a Xabs_a, prob [n,H,W], S [n,H,W] (the warped score, 0 where masked),
      X [n,C,H,W] = the sample of x, Xabs = the sample of |x|, count [H,W] = unmasked agents per pixel.
    The keyword arguments exist for the sensitivity tests alone (a wrong offset, no zero mask, other taps): the defaults are the
    operator."""
    x = np.asarray(feats, np.float64)
    n, C, H, W = x.shape
    HW = H * W
    off, tw, _ = k5_taps(rows, H, W, grid_f64) if taps is None else taps
    keep = k5_keep(crop, n, H, W)
    oc = np.asarray(occ, np.float64).reshape(n, HW)
    score = (1.0 / (1.0 + np.exp(-oc)) + offset) * keep
    S = (tw * score[np.arange(n)[:, None, None], off]).sum(-1)                  # [n, HW]
    prob = _softmax_masked(S, mask_zero)
    v = _gather(x.reshape(n, C, HW), off)                                        # [n, C, HW, 4]
    X = (v * tw[:, None]).sum(-1)
    Xabs = (np.abs(v) * tw[:, None]).sum(-1)
    out = (prob[:, None] * X).sum(0)
    T = (prob[:, None] * Xabs).sum(0)
    return dict(out=out.reshape(C, H, W), T=T.reshape(C, H, W), prob=prob.reshape(n, H, W), S=S.reshape(n, H, W),
                X=X.reshape(n, C, H, W), Xabs=Xabs.reshape(n, C, H, W), count=(S != 0).sum(0).reshape(H, W))


def k5_forward_k(n):
    """Roundings per term, in EPS, of the K5 forward kernels for n agents -> dict(out, score, split), each with +1 for the second
    order.

    Tap weights t: formed by the reference with the kernel's own fp32 operations (k5_taps): no error.

    prob (backward_refs.k5_k, the same code: score_at / sample_score / agent_softmax, and score_src / sample_score_src with the same
        products in the same order):
        score = 1 / (1 + expf(-occ)) + 1e-4f: expf 4, add 1, divide 1 -> sigmoid within 6; the second add 1 -> score within 7
                (both summands positive; expf overflowing to inf at occ < -88 gives sigmoid = 0 for a true value below 1e-38:
                 nothing against 1e-4).
        S_a   = up to 4 positive products score * t added in sequence: product 1, adds 3 -> within 11, S <= 1.0001.      k_score = 11
        e_a   = expf(S_a - mx): the argument's absolute error is <= 2 * 11 * 1.0001 + 1 < 24 EPS -> e within 24 + 4 = 28.
        den   = n positive terms, n - 1 sequential adds: 28 + n - 1;  prob = e / den: 1 more -> within 56 + n.
        One unmasked agent: the argument is 0, e = den = prob = 1 exactly.  A masked agent: prob = 0 exactly.
    k_warp_fuse and k_warp_fuse_lds (same statements; the tests require the two bit-equal):
        wt    = t * prob                                     1   -> 57 + n
        term  = src * wt                                     1   -> 58 + n
        v     = term0; v += term1; v += term2; v += term3    3   -> 61 + n   (each add rounds a partial sum of |terms| <= their sum)
        acc  += v over the agents, acc = 0.f first           n-1 -> 60 + 2 n                                        k_out = 60 + 2 n
    k_warp_agent: feat_ego is `sample` (compared bit for bit with sample_f32); score_ego is S_a above.               k_score = 11
    k_fuse_warped, the stored fp32 scores s_a in [0, 1.0001] and warped maps being its exact inputs:
        s_a - mx                                             1   (absolute: |s_a - mx| <= 1.0001)
        e_a   = expf(.)                                      4   -> e within 5
        den   = n - 1 sequential adds of terms within 5          -> 5 + n - 1
        prob  = e / den                                      1   -> 5 + (5 + n - 1) + 1 = 10 + n
                (each operation is counted once -- subtraction 1, expf 4, den n - 1, division 1 -- but the quotient inherits the
                 5 EPS of e twice, through the numerator and through den, exactly as 28 + 28 above)
        acc  += v * prob over the agents                     1 + (n - 1)                                          k_split = 10 + 2 n"""
    return dict(out=60 + 2 * n + 1, score=11 + 1, split=10 + 2 * n + 1)


def bound(k, T):
    return k * EPS * np.asarray(T, np.float64) + TINY


def split_reference(feats_ego, scores_ego):
    """k_fuse_warped in float64 on given fp32 warped maps [n,C,H,W] and scores [n,1,H,W] -> (out [C,H,W], T [C,H,W], prob)."""
    x = np.asarray(feats_ego, np.float64)
    n, C, H, W = x.shape
    prob = _softmax_masked(np.asarray(scores_ego, np.float64).reshape(n, H * W)).reshape(n, 1, H, W)
    return (prob * x).sum(0), (prob * np.abs(x)).sum(0), prob


def emulate_f32(feats, occ, rows, crop=None, grid_f64=True):
    """k_warp_fuse in fp32 numpy, statement for statement (score_at, sample_score, agent_softmax, wt = t * prob, the tap chain,
    acc += v) -> [C,H,W] float32.  A tap outside the map carries weight 0 here and is skipped there: the same sum.  numpy's fp32
    exp stands in for expf."""
    x = np.asarray(feats, F32)
    n, C, H, W = x.shape
    HW = H * W
    off, tw, _ = k5_taps(rows, H, W, grid_f64)
    t = tw.astype(F32)
    keep = k5_keep(crop, n, H, W).astype(F32)
    oc = np.asarray(occ, F32).reshape(n, HW)
    one = F32(1)
    with np.errstate(over="ignore", under="ignore"):
        score = ((one / (one + np.exp(-oc))).astype(F32) + F32(1e-4)).astype(F32) * keep
    sc = score[np.arange(n)[:, None, None], off]                                   # [n, HW, 4]
    S = (sc[..., 0] * t[..., 0]).astype(F32)
    for k in (1, 2, 3):
        S = (S + (sc[..., k] * t[..., k]).astype(F32)).astype(F32)
    Sm = np.where(S == 0, F32(-np.inf), S).astype(F32)
    mx = Sm.max(0)
    some = np.isfinite(mx)
    with np.errstate(invalid="ignore", under="ignore"):
        e = np.exp((Sm - np.where(some, mx, F32(0))[None]).astype(F32)).astype(F32)
    den = np.zeros(HW, F32)
    for a in range(n):
        den = (den + e[a]).astype(F32)
    prob = np.where(some[None], (e / np.where(some, den, one)[None]).astype(F32), F32(0)).astype(F32)
    wt = (t * prob[..., None]).astype(F32)                                         # [n, HW, 4]
    v = _gather(x.reshape(n, C, HW), off)                                          # [n, C, HW, 4]
    acc = np.zeros((C, HW), F32)
    for a in range(n):
        va = (v[a, ..., 0] * wt[a, None, :, 0]).astype(F32)
        for k in (1, 2, 3):
            va = (va + (v[a, ..., k] * wt[a, None, :, k]).astype(F32)).astype(F32)
        acc = (acc + va).astype(F32)
    return acc.reshape(C, H, W)


# =====================================================================================================================
# launch layouts restated (HEAL_K5_BLOCKS unset)
# =====================================================================================================================
def _cdiv(a, b):
    return -(-a // b)


def fused_layout(C, H, W):
    """heal_warp_fuse: 32 x 8 pixel tiles, channels per block so that about 1024 blocks run, in fours -> (cch, channel blocks)."""
    tiles = _cdiv(W, 32) * _cdiv(H, 8)
    cch = max(4, _cdiv(_cdiv(C * tiles, 1024), 4) * 4)
    if cch > C:
        cch = _cdiv(C, 4) * 4
    return cch, _cdiv(C, cch)


def lds_layout(levels):
    """launch_warp_fuse_levels: per level (C, H, W) 16 x 16 tiles, target 512 blocks, cg = ceil(512 / tiles) channel slices wanted,
    cpb = ceil(ceil(C / cg) / 8) * 8 channels per slice in whole staging rounds -> [dict(tiles_x, tiles, cpb, cgroups, block0,
    blocks, last)], `last` the channels of the last slice."""
    out, b0 = [], 0
    for C, H, W in levels:
        tiles_x = _cdiv(W, 16)
        tiles = tiles_x * _cdiv(H, 16)
        cg = max(1, _cdiv(512, tiles))
        cpb = _cdiv(_cdiv(C, cg), 8) * 8
        cgroups = _cdiv(C, cpb)
        out.append(dict(tiles_x=tiles_x, tiles=tiles, cpb=cpb, cgroups=cgroups, block0=b0, blocks=tiles * cgroups,
                        last=C - (cgroups - 1) * cpb))
        b0 += tiles * cgroups
    return out


def lds_boxes(rows, prob, H, W, grid_f64=True):
    """The source box k_warp_fuse_lds reduces per (16 x 16 ego tile, agent): over the tile's pixels with a tap weight t * prob != 0
    (fp32), the bounding box of ALL their taps inside the map (a zero-weight tap inside the map extends the box as well: the rule
    goes by okb, not by the weight).  -> int array [tiles, n, 4] = (x0, y0, bw, bh), bw = bh = 0 when no pixel of the tile sees
    the agent.  bw <= 32 and bh <= 32: staged through LDS with pitch bw | 1; else the direct-gather fallback."""
    off, tw, ok = k5_taps(rows, H, W, grid_f64)
    n = off.shape[0]
    wt = tw.astype(F32) * np.asarray(prob, F32).reshape(n, H * W, 1)
    use = ok & (wt != 0).any(-1)[..., None]
    big = 1 << 30
    xs, ys = off % W, off // W
    lo = lambda v: np.where(use, v, big).min(-1).reshape(n, H, W)        # noqa: E731
    hi = lambda v: np.where(use, v, -big).max(-1).reshape(n, H, W)       # noqa: E731
    x_lo, x_hi, y_lo, y_hi = lo(xs), hi(xs), lo(ys), hi(ys)
    boxes = []
    for ty in range(0, H, 16):
        for tx in range(0, W, 16):
            sl = (slice(None), slice(ty, ty + 16), slice(tx, tx + 16))
            row = []
            for a in range(n):
                x0, x1, y0, y1 = x_lo[sl][a].min(), x_hi[sl][a].max(), y_lo[sl][a].min(), y_hi[sl][a].max()
                row.append((x0, y0, x1 - x0 + 1, y1 - y0 + 1) if x0 <= x1 else (0, 0, 0, 0))
            boxes.append(row)
    return np.asarray(boxes, np.int64)


def staged(box):
    return 0 < box[2] <= 32 and 0 < box[3] <= 32


# =====================================================================================================================
# fixtures
# =====================================================================================================================
def data(seed, n, C, H, W, logits="normal"):
    """Normal features, and occupancy logits N(0, 2) clipped to +-6 or drawn from SATURATED -> (feats, occ) float32."""
    g = np.random.default_rng(seed)
    feats = g.standard_normal((n, C, H, W)).astype(F32)
    if logits == "saturated":
        occ = g.choice(np.asarray(SATURATED), (n, 1, H, W)).astype(F32)
    else:
        occ = np.clip(g.standard_normal((n, 1, H, W)) * 2, -6, 6).astype(F32)
    return feats, occ


def scale_row(k, tx=0.0, ty=0.0):
    return np.array([[k, 0.0, tx], [0.0, k, ty]])


def _fx(feats_occ, rows, crop=None, grid_exact=False):
    return dict(feats=feats_occ[0], occ=feats_occ[1], rows=np.asarray(rows, np.float64), crop=crop, grid_exact=grid_exact)


def far(n, C=5, H=16, W=8, seed=None, logits="normal"):
    """Half- and whole-pixel translations (the FAR list): taps off the map on all four sides, and -- at the whole-pixel shifts --
    taps inside the map with weight 0.  W < 16: less than one tile of either kernel."""
    return _fx(data(100 + n if seed is None else seed, n, C, H, W, logits), shift_rows(FAR[:n], H, W), None, True)


def counts(n=8, C=3, H=8, W=32):
    """Agent a keeps columns [0, 3 a + 6) of its own map (a crop window) under the FAR translations (at most 3 pixels): ego
    columns 3..5 see all n agents, each band to the right one fewer, the last columns none."""
    crop = [(0, H, 0, 3 * a + 6) for a in range(n)]
    return _fx(data(120 + n, n, C, H, W), shift_rows(FAR[:n], H, W), crop, True)


def rotations(n=4, C=7, H=24, W=40, seed=130):
    """Arbitrary rotations; agent 1 is translated wholly off the map (masked everywhere), agent 2 by about a map's half along x
    (partly off); the ego keeps a centre window only, so that pixels outside it which no rotated map reaches are all masked."""
    rows = rotation_rows(n, seed)
    rows[1, 0, 2] = 6.0
    rows[2, 0, 2] += 1.0
    return _fx(data(seed, n, C, H, W), rows, [(4, H - 4, 6, W - 6)] + [None] * (n - 1))


WINDOW_CROP = [None, (5, 20, 9, 30), (0, 15, 21, 48), (0, 1, 0, 0)]          # a camera window, one on the map's border, an EMPTY one
WINDOW_BOXES = [None, (4, 24, 8, 32), (0, 16, 20, 48), (0, 4, 0, 4)]         # window +- 1 inside; x0 and widths multiples of 4 floats


def window(C=9, H=32, W=48, seed=140):
    """Four agents under rotations: no window, a camera crop window, a window touching the map's border, and the empty window
    (0, 1, 0, 0) whose agent is masked everywhere.  WINDOW_BOXES are the boxes heal_warp_fuse_levels_src reads the windowed agents from."""
    rows = rotation_rows(4, seed, reach=0.3)
    return _fx(data(seed, 4, C, H, W), rows, list(WINDOW_CROP))


def saturated(n=4, C=3, H=16, W=16, seed=150):
    """Logits from SATURATED under the FAR translations, one agent behind a crop window: sigmoid is 0 or 1 to fp32 at the ends, and
    where it is 0 the score IS the 1e-4 offset."""
    crop = [None, (2, 12, 3, 14)] + [None] * (n - 2)
    return _fx(data(seed, n, C, H, W, "saturated"), shift_rows(FAR[2:2 + n], H, W), crop, True)


SHAPES = {"1xW": (1, 37), "Hx1": (19, 1), "5x7": (5, 7), "1x1": (1, 1)}


def shape(name, n=4, C=3):
    """Maps of one row, one column, less than a tile on both axes, one pixel: three translations and a mild rotation."""
    H, W = SHAPES[name]
    rows = np.concatenate([shift_rows([(0.0, 0.0), (0.5, 0.0), (-1.5, 0.5)], H, W),
                           np.array([[[np.cos(0.2), -np.sin(0.2), 0.1], [np.sin(0.2), np.cos(0.2), -0.05]]])])[:n]
    return _fx(data(160 + H + W, n, C, H, W), rows)


CHANNEL_TAILS = (1, 2, 3, 5, 7, 9, 17)
SLICED = (2, 70, 64, 256)          # n, C, H, W: heal_warp_fuse runs cch = 8 with a last slice of 6; the levels launch cpb = 16, last 6
BIG = (2, 20, 256, 256)            # the levels launch runs cpb = 16 with a last slice of 4
ROUNDS = (2, 268, 64, 64)          # the levels launch runs cpb = 16 with a last slice of 12: a second staging round of 4 channels
FOUR_LEVELS = [(17, 13, 21), (5, 40, 24), (3, 5, 3), (9, 1, 1)]
ZOOMS = (1.5, 2.0, 2.25)           # agent a + 1 is scaled by ZOOMS[a]: 16 ego pixels span 24, 32 and 36 source pixels


def sliced(which=SLICED, seed=170):
    n, C, H, W = which
    rows = rotation_rows(n, seed, reach=0.3)
    return _fx(data(seed, n, C, H, W), rows)


def four_levels(n=3, seed=180):
    """One launch of four levels of different shapes and channel counts -> [fixture per level], one set of rows."""
    rows = rotation_rows(n, seed, reach=0.4)
    return [_fx(data(seed + i, n, C, H, W), rows) for i, (C, H, W) in enumerate(FOUR_LEVELS)]


def zoom(C=11, H=64, W=64, seed=190):
    """The ego under the identity and one agent per entry of ZOOMS, scaled about the map's centre: the source footprint of a
    16 x 16 ego tile is a box of 16 * zoom pixels, 32 exactly at zoom 2 (staged) and 36 at zoom 2.25 (direct-gather fallback);
    tiles near the map's border are clipped to smaller boxes.  The 2.25 agent is also shifted by 8 pixels on both axes, so that
    the footprint of the ego tile at (16, 16) lies inside its map, unclipped."""
    rows = np.stack([IDENTITY] + [scale_row(k, 0.25 if k > 2 else 0.0, 0.25 if k > 2 else 0.0) for k in ZOOMS])
    return _fx(data(seed, len(ZOOMS) + 1, C, H, W), rows, None, True)


def equal_agents(n, C=3, H=8, W=16, seed=200):
    """n identical integer maps and logits under the identity (H, W powers of two: the nw tap has weight exactly 1): every e is
    expf(0) = 1, den = n, prob = fl(1 / n) -- one rounding, none when n is a power of two, and then out == the map bit for bit.
    For other n: wt 1, product 1, n - 1 adds -> |out - map| <= (n + 2) EPS |map|."""
    g = np.random.default_rng(seed + n)
    m = g.integers(-3, 4, (1, C, H, W)).astype(F32)
    occ = np.clip(g.standard_normal((1, 1, H, W)) * 2, -6, 6).astype(F32)
    fx = _fx((np.ascontiguousarray(np.repeat(m, n, 0)), np.ascontiguousarray(np.repeat(occ, n, 0))), np.tile(IDENTITY, (n, 1, 1)),
             None, True)
    fx["want"] = m[0]
    return fx


def exact_fixture(name):
    """The exact fixtures of the backward suite, reused: probabilities 0 or 1, dyadic tap weights, integer features."""
    fx = k5_exact_translation() if name == "translation" else k5_collision()
    return dict(feats=fx["feats"], occ=fx["occ"], rows=fx["rows"], crop=fx["crop"], grid_exact=True, unit=fx["unit"])


def bounded_fixtures():
    """name -> fixture: every bounded fixture of the suite that is small enough for the CPU tests to sweep."""
    out = {f"far{n}": far(n) for n in range(1, 9)}
    out.update(counts=counts(), rotations=rotations(), window=window(), saturated=saturated(), zoom=zoom())
    out.update({f"shape_{k}": shape(k) for k in SHAPES})
    out.update({f"c{C}": far(3, C=C, seed=210 + C) for C in CHANNEL_TAILS})
    return out


def reference(fx, grid_f64=True, **kw):
    return k5_forward(fx["feats"], fx["occ"], fx["rows"], fx["crop"], grid_f64, **kw)


def tiny_weights(fx, grid_f64=True):
    """Smallest non-zero tap weight: far above fp32 underflow means S == 0 is decided alike in fp32 and in float64."""
    n, _, H, W = fx["feats"].shape
    _, tw, _ = k5_taps(fx["rows"], H, W, grid_f64)
    return float(tw[tw != 0].min()) if (tw != 0).any() else 1.0
