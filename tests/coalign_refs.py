"""References, per-element error bound and hand-built fixtures of the CoAlign conformance suite (tests/test_gpu_coalign_conformance.py):
k_warp_att_fuse<n> of heal_amd/csrc/warp_fuse.hip in both modes -- numpy only, so that tests/test_coalign_refs_cpu.py can prove them
against the reference's float64 torch composition on a machine without a GPU.

Per ego pixel the kernel samples every agent's map bilinearly (agent 0, the ego, through its own affine row), x_j[c], and reduces
    att:  p = softmax_j(x_0 . x_j / sqrt_dim),  out[c] = sum_j p_j x_j[c]            max:  out[c] = max_j x_j[c].
An agent whose footprint misses the pixel is a zero map: its logit is 0 and keeps its exp(0 - max) share; in `max` it contributes 0.

The taps (offsets and fp32 corner weights) come from backward_refs.k5_taps, which forms them with the kernel's own fp32 operations,
so they carry no error.  sample_f32 then repeats the kernel's `tap4` operation for operation in fp32: `max` mode rounds nothing
else and is compared bit for bit.  `att` mode is evaluated in float64 ON those fp32 taps and held to
    |got - ref| <= SAFETY * EPS * (k * T + E) + TINY                      on every element,
with the conventions of tests/attention_refs.py (EPS = 2^-24 per rounding, expf = 4 EPS, -ffp-contract=off, SAFETY = 2 on the
first-order bound): T = sum_j p_j |x_j|[c] with |x_j| the sample of the absolute map, k from coalign_k, and E the logit error
carried through the softmax exactly as Cm is there: a logit is formed with c_s roundings and subtracted from the maximum with one
more, so its absolute error is (c_s + 1) EPS A_j with A_j = sum_c |x_0|[c] |x_j|[c] / sqrt_dim, and
    Cm_j = (c_s + 1) A_j + sum_i p_i (c_s + 1) A_i + 2 Amax,           E[c] = sum_j p_j Cm_j |x_j|[c].

EXACT.  Half-pixel translations on power-of-two maps (weights 0, 1/4, 1/2, 1), small integer features and a power-of-two sqrt_dim:
every sample is a multiple of 1/4, every product and partial sum of a dot product a multiple of 1/16 below 2^24 units, every logit
exact.  Nothing is needed from expf beyond expf(0) == 1 and expf(x) == 0 for x < -104 (below half the smallest denormal)."""
import numpy as np

from tests.attention_refs import EPS, EXACT_LIMIT, F32, SAFETY, TINY, max_ratio      # noqa: F401  (re-exported for the tests)
from tests.backward_refs import k5_taps, shift_rows

WA_SMALL_TILES = 1024          # warp_fuse.hip: a level with fewer 16 x 4 tiles than this runs 16 pixels x 16 channel slices
UNDERFLOW_GAP = 104.0          # expf(-104) = 6.8e-46 < 2^-150: rounds (or flushes) to 0


def coalign_layout(H, W):
    """The library's layout rule restated (heal_warp_att_fuse_levels): -> (pixels per block, channel slices)."""
    tiles = -(-W // 16) * -(-H // 4)
    pix = 16 if tiles < WA_SMALL_TILES else 64
    return pix, 256 // pix


def coalign_blocks(levels):
    """Blocks of every level of one launch [(C, H, W), ..] -> [(block0, blocks, pix)]: the ranges the kernel finds its level by."""
    out, b0 = [], 0
    for _, H, W in levels:
        pix, _ = coalign_layout(H, W)
        nb = -(-W // 16) * -(-H // (pix // 16))
        out.append((b0, nb, pix))
        b0 += nb
    return out


def f32_sqrt_dim(C):
    """sqrt(C) as the fp32 number the kernel divides by when the caller gives none."""
    return float(F32(np.sqrt(C)))


def coalign_k(n, C, n_slices):
    """Roundings per term of k_warp_att_fuse<n> in EPS, mode `att`; C channels in n_slices channel slices (4 or 16).

    x      = tap4: `v = x w; v += x w; v += x w; v += x w`: a tap's term takes its product 1 and at most 3 adds.   c_x  = 4
    dot    : `dot += x0 * xj` over the thread's ceil(C / n_slices) channels: both samples c_x each, the product 1, one rounded add
             per channel; then the slices' partial sums are added in slice order in LDS: n_slices - 1.
    logit  = dot / sqrt_dim: 1.                                             c_s  = 2 c_x + 1 + ceil(C / n_slices) + n_slices - 1 + 1
    e      = expf(logit - mx): the subtraction 1 (-> (c_s + 1) A and Amax in Cm, module docstring), expf 4.
    den    : `den += e` over the n agents from 0.f: n - 1 roundings of a positive sum, each term carrying its expf 4.
    p      = e / den: 1.                                                    k_p  = 4 + 4 + (n - 1) + 1                = n + 8
    out    : `acc += p * x` over the n agents from 0.f: p within k_p (+ Cm, in E), x within c_x, the product 1, n - 1 rounded adds.
                                                                            k_out = k_p + c_x + 1 + (n - 1)            = 2 n + 12
    One agent: logit - mx = 0 exactly, e = den = p = 1 and out = 1 * x + 0: the sample itself (asserted bit for bit, not through k)."""
    c_x = 4
    cper = -(-C // n_slices)
    c_s = 2 * c_x + 1 + cper + (n_slices - 1) + 1
    k_p = n + 8
    return dict(x=c_x, s=c_s, p=k_p, out=k_p + c_x + 1 + (n - 1))


def _gather(x, off):
    """x [n, C, HW], off [n, HW, 4] -> [n, C, HW, 4]."""
    n = x.shape[0]
    return x[np.arange(n)[:, None, None, None], np.arange(x.shape[1])[None, :, None, None], off[:, None, :, :]]


def sample_f32(feats, rows, grid_f64=True):
    """The kernel's tap4 in fp32 numpy, operation for operation: ((v0 w0 + v1 w1) + v2 w2) + v3 w3 with weight 0 for a tap outside the
    map (the kernel then reads element 0 of the plane, k5_taps the clipped neighbour: either way a finite value times 0).
    feats [n, C, H, W] float32, rows [n, 2, 3] -> [n, C, H, W] float32."""
    feats = np.asarray(feats, F32)
    n, C, H, W = feats.shape
    off, tw, _ = k5_taps(rows, H, W, grid_f64)
    v = _gather(feats.reshape(n, C, H * W), off)
    w = tw.astype(F32)[:, None]
    acc = (v[..., 0] * w[..., 0]).astype(F32)
    for k in (1, 2, 3):
        acc = (acc + (v[..., k] * w[..., k]).astype(F32)).astype(F32)
    return acc.reshape(n, C, H, W)


def sample_f64(feats, rows, grid_f64=True):
    """The same sample in float64 on the fp32 tap weights -> (x [n, C, H, W], |x| = the sample of the absolute map)."""
    feats = np.asarray(feats, np.float64)
    n, C, H, W = feats.shape
    off, tw, _ = k5_taps(rows, H, W, grid_f64)
    v = _gather(feats.reshape(n, C, H * W), off)
    return (v * tw[:, None]).sum(-1).reshape(n, C, H, W), (np.abs(v) * tw[:, None]).sum(-1).reshape(n, C, H, W)


def max_reference(feats, rows, grid_f64=True):
    """mode `max`: max_j sample_f32 -- an agent out of reach is a zero map and takes part.  Nothing else rounds: compared bit for bit."""
    return sample_f32(feats, rows, grid_f64).max(0)


def att_reference(feats, rows, sqrt_dim=None, grid_f64=True):
    """mode `att` in float64 on the fp32 taps.  sqrt_dim: the fp32 number the kernel divides by (None: f32_sqrt_dim(C)).
    -> dict(out, T, E, B [C, H, W] -- B the bound, SAFETY and EPS included --, p [n, H, W], logit [n, H, W], k, layout)."""
    n, C, H, W = np.asarray(feats).shape
    sd = f32_sqrt_dim(C) if sqrt_dim is None else float(F32(sqrt_dim))
    x, xa = sample_f64(feats, rows, grid_f64)
    pix, n_slices = coalign_layout(H, W)
    k = coalign_k(n, C, n_slices)
    logit = (x[:1] * x).sum(1) / sd                                  # [n, H, W]
    A = (xa[:1] * xa).sum(1) / sd
    e = np.exp(logit - logit.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    a = (k["s"] + 1) * A
    Cm = a + (p * a).sum(0, keepdims=True) + 2.0 * A.max(0, keepdims=True)
    out = (p[:, None] * x).sum(0)
    T = (p[:, None] * xa).sum(0)
    E = ((p * Cm)[:, None] * xa).sum(0)
    return dict(out=out, T=T, E=E, B=SAFETY * EPS * (k["out"] * T + E), p=p, logit=logit, k=k, layout=(pix, n_slices))


# =====================================================================================================================
# poses
# =====================================================================================================================
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
# half- and whole-pixel translations (sx, sy) in pixels, several with taps off the map on each side
HALF_SHIFTS = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (1.0, 2.0), (-0.5, 0.5), (-3.0, 1.0), (2.5, -1.5), (0.5, 0.5)]


def rotation_rows(n, seed, reach=0.6):
    """n normalised affine rows: the ego's identity, then rotations by arbitrary angles with translations of up to `reach` of the
    half map: taps leave the map over every border."""
    g = np.random.default_rng(seed)
    rows = [IDENTITY.copy()]
    for _ in range(n - 1):
        t = g.uniform(-np.pi, np.pi)
        rows.append(np.array([[np.cos(t), -np.sin(t), g.uniform(-reach, reach)], [np.sin(t), np.cos(t), g.uniform(-reach, reach)]]))
    return np.stack(rows)


def device_rows_case(seed=3):
    """The pose set of the device-row checks -> (n, H, W, rows): 3 agents on a 13 x 21 map (neither extent a multiple of any tile),
    the ego's identity and two rotations whose footprints lie partly on the map and partly off it (asserted)."""
    n, H, W = 3, 13, 21
    rows = rotation_rows(n, seed)
    r = reached(rows, H, W)
    assert r[0].all() and all(r[a].any() and not r[a].all() for a in (1, 2))
    return n, H, W, rows


def off_map_rows(n, whole=1, partial=2):
    """Identity rows, but agent `whole` translated by 3 maps (no ego pixel reaches it: every wave skips it) and agent `partial` by
    0.9 of a map along x only (the first tenth of every row reaches it: some waves in full, some in part, most not at all)."""
    rows = np.tile(IDENTITY, (n, 1, 1))
    if whole < n:
        rows[whole, 0, 2] = 6.0
    if partial < n:
        rows[partial, 0, 2] = 1.8
    return rows


def reached(rows, H, W, grid_f64=True):
    """[n, H, W] bool: some tap of the agent carries weight at the ego pixel."""
    _, tw, _ = k5_taps(rows, H, W, grid_f64)
    return (tw != 0).any(-1).reshape(-1, H, W)


def poses(kind, n, seed):
    """The pose sets of the suite -> rows [n, 2, 3] float64.
      identity : every agent under the identity.
      rot    : rotation_rows: taps off every border.
      ego      : rot, but the ego's own row is a rotation by 0.3 rad shifted by 0.35 of the half map: part of ITS sample is off the map.
      offmap   : off_map_rows: one neighbour out of every wave's reach, one reached by part of the waves."""
    if kind == "identity":
        return np.tile(IDENTITY, (n, 1, 1))
    if kind == "offmap":
        return off_map_rows(n)
    rows = rotation_rows(n, seed)
    if kind == "ego":
        rows[0] = np.array([[np.cos(0.3), -np.sin(0.3), 0.35], [np.sin(0.3), np.cos(0.3), -0.2]])
    return rows


def half_rows(n, H, W):
    """The half-pixel translations of HALF_SHIFTS for ONE H x W level (a shift in pixels is a normalised shift of that level only);
    the ego's is the identity."""
    return shift_rows(HALF_SHIFTS[:n], H, W)


# level sets [(C, H, W)] of one launch; at most 4 levels
PIX64 = (5, 253, 260)                          # 17 x 64 = 1088 tiles of 16 x 4: the 64-pixel layout, ragged on both axes
MIXED = [(17, 13, 21), PIX64, (3, 5, 3), (40, 1, 1)]      # 16 / 64 / 16 / 16: both block0 boundaries between layouts are crossed
SMALL = [(1, 7, 9), (64, 9, 37), (3, 19, 5)]   # C = 1 (15 empty slices), C = 64 (4 channels per slice), W < 16
THRESHOLD = [(2, 252, 256), (2, 256, 256)]     # 16 x 63 = 1008 tiles: 16 pixels; 16 x 64 = 1024 tiles: 64 pixels


def bound_fixture(n, levels, pose, seed, own_sqrt_dims=True):
    """Random float features for one launch -> dict(feats [level], rows, sqrt_dims or None).  own_sqrt_dims: 1.25 sqrt(C) per level
    (the wrapper takes them), so that a kernel dividing by sqrt(C) regardless is wrong; None leaves the library's own sqrt(C)."""
    feats = [random_feats(n, C, H, W, seed + 17 * i) for i, (C, H, W) in enumerate(levels)]
    sd = [float(F32(1.25 * np.sqrt(C))) for C, _, _ in levels] if own_sqrt_dims else None
    return dict(feats=feats, rows=poses(pose, n, seed), sqrt_dims=sd)


# =====================================================================================================================
# fixtures
# =====================================================================================================================
def random_feats(n, C, H, W, seed):
    """randn * C^(-1/4): the ego does not dominate the softmax (|x_0|^2 / sqrt(C) is about 1)."""
    g = np.random.default_rng(seed)
    return np.ascontiguousarray(g.standard_normal((n, C, H, W)) * C ** -0.25, F32)


def equal_agents(n, C, H, W, seed):
    """Exact fixture 1: every agent holds the same integer map under the identity (H, W powers of two: the identity samples each
    pixel with weight exactly 1).  All logits are equal, e = 1, den = n, p = 1 / n (n a power of two), every partial sum k x / n is an
    integer over 8: the output equals the map bit for bit.  -> dict(feats, rows, sqrt_dim, want, units)."""
    g = np.random.default_rng(seed)
    m = g.integers(-3, 4, (1, C, H, W)).astype(F32)
    feats = np.ascontiguousarray(np.repeat(m, n, 0))
    units = 16.0 * C * 9 / 0.5                                      # |dot| <= 9 C, / sqrt_dim 0.5, in units of 1/16
    return dict(feats=feats, rows=np.tile(IDENTITY, (n, 1, 1)), sqrt_dim=0.5, want=m[0], units=units)


SELECTOR_SCALE = 512.0
EQUAL_CASES = [(n, C, H, W) for n in (1, 2, 4, 8) for C, H, W in ((3, 8, 16), (2, 256, 256))]          # 16- and 64-pixel layout
SELECTOR_CASES = [(n, 17, 8, 16) for n in range(2, 9)] + [(4, 3, 256, 256)]


def selector(n, C, H, W, seed, chosen=None):
    """Exact fixture 2 (n >= 2): integer maps in [-2, 2]; the ego and neighbour `chosen` share one half-pixel translation and the
    neighbour's map is SELECTOR_SCALE times the ego's, so its sample is that multiple of the ego's sample at every pixel; the
    other neighbours hold independent integer maps under other half-pixel translations.  The ego map is zero on a band of columns.
    With sqrt_dim = 1/4:
      where the ego's sample is non-zero, |x_0|^2 >= 1/16 and logit_chosen - logit_j = (512 |x_0|^2 - x_0 . x_j) / (1/4) > 104 for
        every other j (asserted on the CPU, not assumed): expf underflows to 0, p is one-hot and out = the chosen sample, bit for bit;
      where the ego's sample is zero, every logit is 0: p = 1 / n, out = (sum_j x_j) / n -- exact for n a power of two (the chosen
        neighbour's sample is 0 there too).
    -> dict(feats, rows, sqrt_dim, chosen, units)."""
    assert n >= 2
    g = np.random.default_rng(seed)
    chosen = n - 1 if chosen is None else chosen
    feats = g.integers(-2, 3, (n, C, H, W)).astype(F32)
    feats[0, :, :, W // 2:W // 2 + max(3, W // 4)] = 0.0
    feats[chosen] = feats[0] * F32(SELECTOR_SCALE)
    shifts = [HALF_SHIFTS[(j + 1) % len(HALF_SHIFTS)] for j in range(n)]
    shifts[0] = (0.5, -0.5)
    shifts[chosen] = shifts[0]
    units = 16.0 * C * 2 * 2 * SELECTOR_SCALE / 0.25                # |x_0 . x_chosen| <= 4 * 512 C, / sqrt_dim, in units of 1/16
    return dict(feats=np.ascontiguousarray(feats), rows=shift_rows(shifts, H, W), sqrt_dim=0.25, chosen=chosen, units=units)


def selector_masks(fx):
    """-> (ego sample non-zero [H, W], ego sample zero [H, W], the smallest logit gap on the former)."""
    x, _ = sample_f64(fx["feats"], fx["rows"])
    nz = (x[0] != 0).any(0)
    logit = (x[:1] * x).sum(1) / fx["sqrt_dim"]
    others = np.delete(logit, fx["chosen"], 0)
    gap = (logit[fx["chosen"]][None] - others)[:, nz]
    return nz, ~nz, float(gap.min()) if gap.size else float("inf")
