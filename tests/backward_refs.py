"""Float64 numpy references and hand-built fixtures of the backward-kernel conformance suite (tests/test_gpu_backward_conformance.py:
heal_warp_fuse_backward (K5), heal_bev_pool_backward (K4), heal_pfn_moments / _features / _backward (K2)) -- numpy only, so that
tests/test_backward_refs_cpu.py can prove every reference against float64 torch autograd on a machine without a GPU.

Two kinds of comparison are built here.

EXACT.  The fixture holds small dyadic rationals (integers, quarters, powers of two) such that every term a kernel can form and
every partial sum of them, in any order, is a multiple of one grid unit `u` and smaller than 2^24 u.  fp32 then computes all of
it without rounding -- atomics in any order included -- and the float64 reference must equal the kernel's output bit for bit.
Each fixture carries `exact_units`, the largest sum of absolute terms divided by `u`; the tests assert it is below 2^24.

PER-ELEMENT BOUND.  Where a transcendental forbids exactness, the reference also returns T, the sum of the ABSOLUTE values of the
terms of each output element (the same formula on |x|, |G|, |weights| with the probabilities kept), and the test asserts
|got - ref| <= k * 2^-24 * T + tiny element by element.  k counts fp32 roundings per term (EPS = 2^-24 is half an ulp: one
rounding is a relative error of at most EPS; `expf` is taken as 2 ulp = 4 EPS, as in out_bound of tests/test_gpu_disconet.py).
The k of every output is derived in the docstring of its *_k function from the kernel's operation sequence; none was tuned on a
kernel's output.  The library is built with -ffp-contract=off, so a product followed by an add is two roundings and only the
`fmaf` calls written in the source are fused."""
import numpy as np

from oracle import oracle_np as O

F32 = np.float32
EPS = 2.0 ** -24
TINY = 1e-30
EXACT_LIMIT = 2.0 ** 24


def max_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the elements (0 where both error and bound are 0): <= 1 means the bound holds."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float((err / (np.asarray(bound, np.float64) + TINY)).max()) if err.size else 0.0


# =====================================================================================================================
# K5: heal_warp_fuse_backward
# =====================================================================================================================
def shift_rows(shifts, H, W):
    """Normalised affine rows (fp64) of pure translations by (sx, sy) pixels: the sample of ego pixel (y, x) is taken at
    (y + sy, x + sx).  With H and W powers of two and shifts that are multiples of 1/2, the sampling coordinates and the bilinear
    weights (0, 1/4, 1/2, 1) are exact in the kernel's arithmetic."""
    return np.array([[[1.0, 0.0, 2.0 * sx / W], [0.0, 1.0, 2.0 * sy / H]] for sx, sy in shifts], dtype=np.float64)


# the `far` shift list of tests/test_gpu_disconet.py: half- and whole-pixel translations, several with taps off the map on each side
FAR = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (1.0, 2.0), (-0.5, 0.5), (-3.0, 1.0), (2.5, -1.5), (0.5, 0.5)]


def _base_coord_f32(n):
    """base_coord<float> of heal_amd/csrc/warp_taps.h (= torch.linspace(-1, 1, n) * (n - 1) / n in fp32), operation for operation."""
    if n <= 1:
        return np.zeros(1, F32)
    j = np.arange(n)
    step = F32(2) / F32(n - 1)
    lo = F32(-1) + step * j.astype(F32)
    hi = F32(1) - step * (n - 1 - j).astype(F32)
    v = np.where(j < n // 2, lo, hi).astype(F32)
    return (v * F32(n - 1) / F32(n)).astype(F32)


def grid_f32(rows, H, W):
    """grid_point<float>: the affine grid built in fp32 (the rows rounded to fp32 first), ((m0 xs + m1 ys) + m2) -> [n,H,W,2]."""
    m = np.asarray(rows, np.float64).reshape(-1, 6).astype(F32)
    xs, ys = _base_coord_f32(W)[None, None, :], _base_coord_f32(H)[None, :, None]
    c = lambda k: m[:, k, None, None]      # noqa: E731
    gx = ((c(0) * xs).astype(F32) + (c(1) * ys).astype(F32)).astype(F32) + c(2)
    gy = ((c(3) * xs).astype(F32) + (c(4) * ys).astype(F32)).astype(F32) + c(5)
    return np.stack([gx.astype(F32), gy.astype(F32)], -1)


def k5_taps(rows, H, W, grid_f64=True):
    """The four bilinear taps of every (agent, ego pixel) by the reference's own arithmetic: oracle_np.affine_grid in float64
    (or grid_f32), rounded to fp32 (`.to(src)`), then the unnormalise / floor / corner-weight / `0 <= x <= W-1` rule of
    oracle_np.grid_sample_bilinear in fp32.  -> (off [n,H*W,4] int64 source pixel y*W+x, clipped where invalid;
    tw [n,H*W,4] float64, the fp32 weights; ok [n,H*W,4] bool)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 2, 3)
    grid = O.affine_grid(rows, H, W).astype(F32) if grid_f64 else grid_f32(rows, H, W)
    x, y = grid[..., 0], grid[..., 1]
    ix = ((x + F32(1)) * F32(W) - F32(1)) / F32(2)
    iy = ((y + F32(1)) * F32(H) - F32(1)) / F32(2)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + F32(1), y0 + F32(1)
    ws = [(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)]
    off, tw, ok = [], [], []
    for (xx, yy), w in zip(((x0, y0), (x1, y0), (x0, y1), (x1, y1)), ws):
        good = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        xi, yi = np.clip(xx, 0, W - 1).astype(np.int64), np.clip(yy, 0, H - 1).astype(np.int64)
        off.append(yi * W + xi)
        tw.append(np.where(good, w.astype(F32), F32(0)).astype(np.float64))
        ok.append(good)
    n = rows.shape[0]
    stack = lambda v: np.stack(v, -1).reshape(n, H * W, 4)      # noqa: E731
    return stack(off), stack(tw), stack(ok)


def k5_keep(crop, n, H, W):
    """[n, H*W] 0/1: the crop window (h0, h1, w0, w1) of every agent; None or h1 <= h0 keeps everything (the kernel's convention:
    an EMPTY window is therefore written with h1 > h0 and w1 <= w0, e.g. (0, 1, 0, 0))."""
    keep = np.ones((n, H, W))
    if crop is not None:
        for a, c in enumerate(crop):
            if c is not None and c[1] > c[0]:
                keep[a] = 0
                keep[a, c[0]:c[1], c[2]:max(c[3], c[2])] = 1
    return keep.reshape(n, H * W)


def k5_reference(feats, occ, rows, grad_out, crop=None, grid_f64=True, offset=float(F32(1e-4))):
    """Float64 gradient of out[c,p] = sum_a w_a(p) X_a[c](p) with respect to feats and occ (the comment above
    k_warp_fuse_backward): score = (sigmoid(occ) + 1e-4) * crop, S_a = sum_k t_ak score_a[off_ak], S == 0 -> -inf, all masked ->
    weights 0, w = softmax_a(S);
        dL/dx[a,c,off_ak]  += G[c,p] w_a t_ak
        dL/dS_a            = w_a (q_a - sum_b w_b q_b),   q_a = sum_c G[c,p] X_a[c](p)
        dL/docc[a,off_ak]  += dL/dS_a t_ak sg (1 - sg) crop.
    Returns a dict: g_feats, g_occ; T_feats, T1_occ, T2_occ (sums of absolute terms: the same formulas on |x|, |G| with the
    probabilities kept and q_a - sum w q replaced by q_a + sum w q; T1 carries sg (1 - sg), T2 carries sg sg, see k5_k);
    n_feats, n_occ (number of non-zero terms added into each element); prob [n, H*W].  offset: the kernel adds the float32
    constant 1e-4f."""
    x = np.asarray(feats, np.float64)
    n, C, H, W = x.shape
    HW = H * W
    x = x.reshape(n, C, HW)
    G = np.asarray(grad_out, np.float64).reshape(C, HW)
    oc = np.asarray(occ, np.float64).reshape(n, HW)
    off, tw, _ = k5_taps(rows, H, W, grid_f64)
    keep = k5_keep(crop, n, H, W)
    sg = 1.0 / (1.0 + np.exp(-oc))
    score = (sg + offset) * keep
    ar = np.arange(n)[:, None, None]
    S = (tw * score[ar, off]).sum(-1)                               # [n, HW]
    Sm = np.where(S == 0, -np.inf, S)
    mx = Sm.max(0, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(Sm - np.where(np.isfinite(mx), mx, 0.0))
    den = e.sum(0, keepdims=True)
    prob = np.where(den > 0, e / np.where(den > 0, den, 1.0), 0.0)  # [n, HW]
    out = {"prob": prob}
    for tag, xx, GG, sign in (("", x, G, -1.0), ("T", np.abs(x), np.abs(G), 1.0)):
        X = np.einsum("apk,acpk->acp", tw, xx[ar, :, off].transpose(0, 3, 1, 2))      # [n, C, HW]
        q = np.einsum("cp,acp->ap", GG, X)
        dS = prob * (q + sign * (prob * q).sum(0, keepdims=True))
        gf = np.zeros((n, C, HW))
        go = np.zeros((n, HW))
        go2 = np.zeros((n, HW))
        nf = np.zeros((n, C, HW))
        no = np.zeros((n, HW))
        for a in range(n):
            for k in range(4):
                d = GG * (prob[a] * tw[a, :, k])[None, :]           # [C, HW]
                np.add.at(gf[a], (slice(None), off[a, :, k]), d)
                t = dS[a] * tw[a, :, k] * keep[a, off[a, :, k]]
                np.add.at(go[a], off[a, :, k], t * (sg * (1 - sg))[a, off[a, :, k]])
                if tag:
                    np.add.at(go2[a], off[a, :, k], t * (sg * sg)[a, off[a, :, k]])
                    np.add.at(nf[a], (slice(None), off[a, :, k]), (d != 0).astype(np.float64))
                    np.add.at(no[a], off[a, :, k], (t != 0).astype(np.float64))
        if tag:
            out.update(T_feats=gf.reshape(n, C, H, W), T1_occ=go.reshape(n, 1, H, W), T2_occ=go2.reshape(n, 1, H, W),
                       n_feats=nf.reshape(n, C, H, W), n_occ=no.reshape(n, 1, H, W))
        else:
            out.update(g_feats=gf.reshape(n, C, H, W), g_occ=go.reshape(n, 1, H, W))
    return out


def k5_k(n, C):
    """Roundings per term of k_warp_fuse_backward, in EPS, for n agents and C channels (first order, +1 for the second order).

    Tap weights: the reference forms them with the kernel's own fp32 operations (k5_taps), so they carry no error.
    score  = 1 / (1 + expf(-occ)) + 1e-4: expf 4, add 1, divide 1 -> sg within 6; the second add 1 -> score within 7.
    S_a    = sum of <= 4 positive products score * t: product 1, sequential adds 3 -> within 11 (S <= 1.0001).
    prob   : the argument S_a - mx has an absolute error <= 2 * 11 * 1.0001 + 1 < 24 EPS, so e_a = expf(.) is within 24 + 4 = 28;
             den (n positive terms, n - 1 sequential adds) within 28 + n - 1; the division 1 -> prob within 56 + n.
             One unmasked agent: the argument is 0 exactly, e = den = prob = 1 exactly.
    g_feats: a term is (g * prob) * t: two products -> 58 + n per term; the element is the sum of N atomic adds, each rounding a
             partial sum that is at most T: N - 1.                                     k_feats = 59 + n + (N - 1)
    q_a    = fmaf(g, x, q) over C channels, x = sum of <= 4 products feats * t (1 + 3): within (4 + C) of its absolute sum Q_a.
    dot    = fmaf(prob_b, q_b, dot) over n agents: (4 + C) + (56 + n) + n of D = sum_b prob_b Q_b.
    dS_a   = prob_a * (q_a - dot): subtraction 1 of (Q_a + D), prob 56 + n, product 1: within 118 + C + 3 n of prob_a (Q_a + D),
             which is what the reference's T carries in place of |dS_a|.
    g_occ  : a term is dS * t * sg * (1 - sg): three products 3, sg 6, and (1 - sg) has its own rounding 1 relative to (1 - sg)
             plus the inherited 6 EPS sg ABSOLUTE -- not relative to (1 - sg), which may be small.  So the bound has two parts:
             (118 + C + 3 n + 3 + 6 + 1 + (N - 1) + 1) * T1  with T1 = sum |dS| t sg (1 - sg), and 6 * T2 with T2 = sum |dS| t sg sg.
    -> (k_feats without N, k1_occ without N, k2_occ); the caller adds the per-element N."""
    return 59 + n, 129 + C + 3 * n, 6


def k5_bounds(ref, n, C):
    kf, k1, k2 = k5_k(n, C)
    bf = EPS * (kf + np.maximum(ref["n_feats"] - 1, 0)) * ref["T_feats"]
    bo = EPS * ((k1 + np.maximum(ref["n_occ"] - 1, 0)) * ref["T1_occ"] + k2 * ref["T2_occ"])
    return bf, bo


def k5_ints(seed, n, C, H, W, gmax=3):
    """Small integer feats / grad_out and random occupancy logits N(0, 2) clipped to +-6."""
    g = np.random.default_rng(seed)
    feats = g.integers(-2, 3, (n, C, H, W)).astype(F32)
    gout = g.integers(-gmax, gmax + 1, (C, H, W)).astype(F32)
    occ = np.clip(g.standard_normal((n, 1, H, W)) * 2, -6, 6).astype(F32)
    return feats, occ, gout


def k5_exact_units(ref, unit):
    """Largest sum of absolute terms of g_feats in units of `unit` (the grid of the tap weights: 1/4 for half-pixel translations,
    1/64 for the scale-1/4 affine row): with probabilities 0 / 1 every term is |G| t."""
    return float(ref["T_feats"].max()) / unit


def k5_exact_translation(n=3, C=3, H=8, W=16, seed=0):
    """Case 1: at every ego pixel at most one agent has a non-zero score, so its softmax weight is expf(0) / 1 = 1 exactly.
    Agent a keeps only the vertical band of columns [a * W / n', ...) of ITS OWN map through a crop window; the translations are
    chosen so that the bands land on disjoint ego columns, with a gap of ego pixels that no agent reaches (all masked)."""
    assert n == 3 and W == 16
    feats, occ, gout = k5_ints(seed, n, C, H, W)
    # agent 0: own columns 0..3, not moved -> ego columns 0..3 (taps at whole pixels)
    # agent 1: own columns 6..9, sampled at x + 0.5 -> ego columns 5..9 read own columns (5,6)..(9,10): non-zero on ego 5..9
    # agent 2: own columns 13..15, sampled at (x + 1, y - 0.5) -> ego columns 12..14; ego column 15 samples off the map
    # ego columns 4, 10, 11, 15: every agent masked
    crop = [(0, H, 0, 4), (0, H, 6, 10), (0, H, 13, 16)]
    rows = shift_rows([(0.0, 0.0), (0.5, 0.0), (1.0, -0.5)], H, W)
    return dict(feats=feats, occ=occ, grad_out=gout, rows=rows, crop=crop, unit=0.25)


def k5_collision(seed=5):
    """Case 5: scale 1/4, no rotation, on a 16 x 16 map -- about sixteen ego pixels add into each source pixel of the centre
    4 x 4 (5 x 5 with the bilinear ring); tap weights are multiples of 1/64.  The second agent has an empty crop window: its score
    is 0 everywhere, it is masked, and the first agent's probability is exactly 1."""
    n, C, H, W = 2, 2, 16, 16
    feats, occ, gout = k5_ints(seed, n, C, H, W)
    rows = np.array([[[0.25, 0.0, 0.0], [0.0, 0.25, 0.0]]] * 2, np.float64)
    return dict(feats=feats, occ=occ, grad_out=gout, rows=rows, crop=[None, (0, 1, 0, 0)], unit=1.0 / 64)


def k5_unmasked_count(fx):
    """Per ego pixel the number of agents with a non-zero warped score -> [H*W] int."""
    n, _, H, W = fx["feats"].shape
    off, tw, _ = k5_taps(fx["rows"], H, W)
    keep = k5_keep(fx["crop"], n, H, W)
    S = (tw * keep[np.arange(n)[:, None, None], off]).sum(-1)      # the score itself is > 0 everywhere inside the window
    return (S != 0).sum(0)


# =====================================================================================================================
# K4: heal_bev_pool_backward
# =====================================================================================================================
K4_X = (-4.0, 1.0, 8)          # lower edge, cell size, cells: xbound [-4, 4, 1]
K4_Y = (-2.0, 0.5, 8)          # ybound [-2, 2, 0.5]
K4_Z1 = (-1.0, 4.0, 1)         # one z bin:  zbound [-1, 3, 4]: the frustum's z = 1 is at fz = 0.5
K4_Z2 = (-0.5, 1.0, 2)         # two z bins: zbound [-0.5, 1.5, 1]: z = 1 is at fz = 1.5 (bin 1); a camera translated by -1 cell: bin 0


def k4_fixture(fpos, cam_cells, n_agents, n_cams, nz=1):
    """Exact lift-splat geometry.  fpos [D,fH,fW,2]: the position of every frustum point in CELL units (fx, fy) before the camera
    translation; cam_cells [n_agents*n_cams,3]: whole-cell translations (tx, ty, tz) per camera.  With identity rotations and
    intrinsics lss_cell_key computes (fr.x * fr.z, fr.y * fr.z, fr.z) + trans with fr.z = 1, so the point of camera bn lands at
    f = fpos + (tx, ty), fz = z0 + tz in cell units -- every operation exact (powers of two and small integers).
    The fixture, not any geometry code, decides the cell: a point is in the grid iff -1 < f < n on every axis (the reference's
    `.long()` truncates toward zero, so -1 < f < 0 is cell 0), and its cell is trunc(f).
    -> dict(frustum [D,fH,fW,3] f32, trans [BN,3] f32, dx, bx, nx, cell [BN,D,fH,fW] int64 flat index (iz*ny+iy)*nx+ix within the
       agent or -1, f [BN,D,fH,fW,3] the cell-unit positions)."""
    fpos = np.asarray(fpos, np.float64)
    cam_cells = np.asarray(cam_cells, np.float64).reshape(n_agents * n_cams, 3)
    zs = K4_Z1 if nz == 1 else K4_Z2
    lo = np.array([K4_X[0], K4_Y[0], zs[0]])
    dx = np.array([K4_X[1], K4_Y[1], zs[1]])
    nx = np.array([K4_X[2], K4_Y[2], zs[2]], np.int64)
    D, fH, fW, _ = fpos.shape
    fr = np.ones((D, fH, fW, 3))
    fr[..., :2] = lo[:2] + fpos * dx[:2]
    z0 = (1.0 - lo[2]) / dx[2]
    f = np.concatenate([fpos, np.full((D, fH, fW, 1), z0)], -1)[None] + cam_cells[:, None, None, None, :]
    inside = ((f > -1) & (f < nx)).all(-1)
    c = np.trunc(f).astype(np.int64)
    inside &= ((c >= 0) & (c < nx)).all(-1)
    cell = np.where(inside, (c[..., 2] * nx[1] + c[..., 1]) * nx[0] + c[..., 0], -1)
    frustum, trans = fr.astype(F32), (cam_cells * dx).astype(F32)
    assert np.array_equal(frustum.astype(np.float64), fr) and np.array_equal(trans.astype(np.float64), cam_cells * dx)
    return dict(frustum=frustum, trans=trans, dx=dx.astype(F32), bx=(lo + dx / 2).astype(F32), nx=nx, cell=cell, f=f,
                n_agents=n_agents, n_cams=n_cams)


def k4_centres(D, fH, fW, seed, lo=0, hi=8):
    """Cell-centre positions (k + 0.5) with k random in [lo, hi) on both axes -> fpos [D,fH,fW,2]."""
    g = np.random.default_rng(seed)
    return g.integers(lo, hi, (D, fH, fW, 2)).astype(np.float64) + 0.5


def k4_edge_positions():
    """Case 6 (D = 4, 2 x 3 pixels).  Pixel (0,0): every bin outside the grid.  Pixel (0,1), along x: fx = -0.5 (half a cell below
    the grid: cell 0 by truncation toward zero), fx = -1 (lo - dx: out), fx = nx (the far edge: out) and one interior point.
    Pixel (1,2): the same along y.  The rest are interior cell centres."""
    fpos = k4_centres(4, 2, 3, 8)
    fpos[:, 0, 0, 0] = [-1.5, 8.5, 9.5, -2.5]
    fpos[:, 0, 1, 0] = [-0.5, -1.0, 8.0, 3.5]
    fpos[:, 1, 2, 1] = [-0.5, -1.0, 8.0, 3.5]
    return fpos


def k4_data(fx, D, C, seed, exact, fmax=2):
    """logit [BN,D,fH,fW], feat [BN,C,fH,fW], grad_out [n_agents, nz*C, ny, nx] (f32).  exact: equal logits per pixel (an integer
    that differs from pixel to pixel) and integer feat / grad_out in [-fmax, fmax]; else logits N(0,1) clipped to +-4 and normal
    feat / grad_out."""
    g = np.random.default_rng(seed)
    BN = fx["n_agents"] * fx["n_cams"]
    _, fH, fW, _ = fx["frustum"].shape
    nx = fx["nx"]
    shape_g = (fx["n_agents"], int(nx[2]) * C, int(nx[1]), int(nx[0]))
    if exact:
        logit = np.broadcast_to(g.integers(-3, 4, (BN, 1, fH, fW)), (BN, D, fH, fW)).astype(F32)
        feat = g.integers(-fmax, fmax + 1, (BN, C, fH, fW)).astype(F32)
        gout = g.integers(-fmax, fmax + 1, shape_g).astype(F32)
    else:
        logit = np.clip(g.standard_normal((BN, D, fH, fW)), -4, 4).astype(F32)
        feat = g.standard_normal((BN, C, fH, fW)).astype(F32)
        gout = g.standard_normal(shape_g).astype(F32)
    return np.ascontiguousarray(logit), feat, gout


def k4_point_rows(fx, grad_out, C):
    """G of every lifted point's cell, [BN,D,fH,fW,C] float64 (0 for a point outside the grid): grad_out is
    [n_agents, nz*C, ny, nx] with channel z * C + c -- the layout oracle_np.bev_pool produces (final[b,:,z,y,x], the z slices
    concatenated along the channels; tests/test_backward_refs_cpu.py checks that on the forward oracle)."""
    nx = fx["nx"]
    n_agents, n_cams = fx["n_agents"], fx["n_cams"]
    g = np.asarray(grad_out, np.float64).reshape(n_agents, int(nx[2]), C, int(nx[1]) * int(nx[0]))
    rows = g.transpose(0, 1, 3, 2).reshape(n_agents, -1, C)          # [agent, (iz*ny+iy)*nx+ix, C]
    cell = fx["cell"]
    agent = (np.arange(cell.shape[0]) // n_cams)[:, None, None, None]
    return np.where((cell >= 0)[..., None], rows[agent, np.clip(cell, 0, None)], 0.0)


def k4_reference(fx, logit, feat, grad_out):
    """The comment above k_lss_backward in float64: p = softmax_d(logit), dL/df[c] = sum_d p_d G[cell_d][c],
    dL/dlogit_d = p_d (s_d - sum_d' p_d' s_d'), s_d = sum_c f[c] G[cell_d][c].  Also T_feat = sum_d p_d |G|, and
    T_logit = p_d (s|.|_d + sum p s|.|) with s|.| = sum_c |f| |G|."""
    lg = np.asarray(logit, np.float64)
    ft = np.asarray(feat, np.float64)
    Gp = k4_point_rows(fx, grad_out, ft.shape[1])
    e = np.exp(lg - lg.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    s = np.einsum("ncvu,ndvuc->ndvu", ft, Gp)
    sa = np.einsum("ncvu,ndvuc->ndvu", np.abs(ft), np.abs(Gp))
    return dict(g_feat=np.einsum("ndvu,ndvuc->ncvu", p, Gp), g_logit=p * (s - (p * s).sum(1, keepdims=True)),
                T_feat=np.einsum("ndvu,ndvuc->ncvu", p, np.abs(Gp)), T_logit=p * (sa + (p * sa).sum(1, keepdims=True)), p=p)


def k4_k(D):
    """Roundings per term of k_lss_backward in EPS, for logits in [-4, 4] (k4_data clips them).

    p      : lg - mx is one rounding of a number <= 8: the argument is within 8 EPS absolute, e = expf(.) within 8 + 4 = 12; wave_sum
             is a 6-level butterfly of positive terms: 6; the division 1 -> p within 12 + 12 + 6 + 1 = 31.
    g_feat = fmaf(p_d, G, gf) over the D bins: p 31, one rounding of the partial sum per bin: D.       k_feat = 31 + D + 1
    s_d    = fmaf(f, G, part) over 4 channel groups: 4, wave_sum 6 -> within 10 of s|.|.
    dot    = wave_sum(p * s): p 31, product 1, s 10, butterfly 6 -> 48 of sum p s|.|.
    g_logit= p * (s - dot): subtraction 1 of (s|.| + sum p s|.|), p 31, product 1, and the errors of s (10) and dot (48) each bounded
             by 48 of the same sum -> 81.                                                              k_logit = 82
    -> (k_feat, k_logit)"""
    return 32 + D, 82


def k4_exact_units(D, C, fmax):
    """Exact fixture: p = 1/D, integer f and G in [-fmax, fmax].  g_feat is a multiple of 1/D with |.| <= fmax; s is an integer with
    |s| <= C fmax^2, dot a multiple of 1/D below the same, p (s - dot) a multiple of 1/D^2 with |.| <= 2 C fmax^2 / D.  Every value
    and partial sum in units of 1/D^2 is below 2 C fmax^2 D^2."""
    return 2.0 * C * fmax * fmax * D * D


# =====================================================================================================================
# K2: heal_pfn_moments / heal_pfn_features / heal_pfn_backward
# =====================================================================================================================
K2_VOXEL = (1.0, 1.0, 4.0)
K2_RANGE = (0.0, 0.0, -2.0, 4.0, 4.0, 2.0)      # pillar centres at x + 0.5, y + 0.5, 0


def k2_pillars(M, P, seed, nps=None):
    """M hand-built pillars of P slots.  Coordinates are multiples of 1/4; the points of a pillar come in pairs mean +- d (and one
    point at the mean if the count is odd), so that the mean is a multiple of 1/4 whatever the count -- the kernel's fp32 sum of
    the slots is exact and so is its IEEE division by the count.  Slots past num_points are zero, as the voxeliser leaves them.
    nps: the point counts (default: a cycle through 1, P, 2, P - 1, 3, P // 2 + 1, 16, 17 clipped to [1, P]).
    -> voxels [M,P,4] f32, coords [M,4] i32 (agent, z, y, x), num_points [M] i32."""
    g = np.random.default_rng(seed)
    if nps is None:
        cyc = [1, P, 2, P - 1, 3, P // 2 + 1, 16, 17]
        nps = [min(max(cyc[m % len(cyc)], 1), P) for m in range(M)]
    nps = np.asarray(nps, np.int32)
    vox = np.zeros((M, P, 4), np.float64)
    coords = np.zeros((M, 4), np.int32)
    for m in range(M):
        n = int(nps[m])
        coords[m] = (0, 0, g.integers(0, 4), g.integers(0, 4))
        mean = np.array([coords[m, 3], coords[m, 2], -1.0]) + g.integers(0, 4, 3) / 4.0
        pts = np.repeat(mean[None], n, 0)
        d = g.integers(-4, 5, (n // 2, 3)) / 4.0
        pts[0:2 * (n // 2):2] += d
        pts[1:2 * (n // 2):2] -= d
        vox[m, :n, :3] = pts[g.permutation(n)]
        vox[m, :n, 3] = g.integers(0, 5, n) / 4.0
    return vox.astype(F32), coords, nps


def k2_params(seed, exact=True):
    """weight [64,10], bn_scale, bn_shift, mean, rstd [64] (f32).  exact: integer weights in [-2, 2], rstd and gamma powers of two
    (scale = gamma rstd in {1/4 .. 4}), integer mean in [-2, 2], integer shift in [-3, 3] with both signs and zero."""
    g = np.random.default_rng(seed)
    if exact:
        w = g.integers(-2, 3, (64, 10)).astype(np.float64)
        rstd = 2.0 ** g.integers(-1, 2, 64)
        gamma = 2.0 ** g.integers(-1, 2, 64)
        mean = g.integers(-2, 3, 64).astype(np.float64)
        shift = g.integers(-3, 4, 64).astype(np.float64)
    else:
        w = g.standard_normal((64, 10)) * 0.5
        rstd = g.uniform(0.5, 2.0, 64)
        gamma = g.uniform(0.5, 1.5, 64)
        mean = g.standard_normal(64) * 0.5
        shift = g.standard_normal(64) * 0.5
    f = lambda a: np.ascontiguousarray(a, F32)      # noqa: E731
    w, rstd, mean, shift = f(w), f(rstd), f(mean), f(shift)
    scale = f(f(gamma).astype(np.float64) * rstd.astype(np.float64))
    return dict(weight=w, scale=scale, shift=shift, mean=mean, rstd=rstd)


def k2_features64(voxels, coords, num_points, voxel_size=K2_VOXEL, lidar_range=K2_RANGE):
    """oracle_np.pillar_features in float64, and fabs: per feature the sum of the absolute operands it was formed from
    (|pt| for the raw point, |pt| + mean|pt| for point - mean, |pt| + |x vx| + |offset| for point - centre), masked like f."""
    v = np.asarray(voxels, np.float64)
    M, P, _ = v.shape
    n = np.asarray(num_points, np.float64).reshape(M, 1, 1)
    mean = v[:, :, :3].sum(1, keepdims=True) / n
    mabs = np.abs(v[:, :, :3]).sum(1, keepdims=True) / n
    c = np.asarray(coords, np.float64)
    vs = np.asarray(voxel_size, np.float64)
    offs = vs / 2 + np.asarray(lidar_range[:3], np.float64)
    cen = c[:, [3, 2, 1]] * vs + offs
    cabs = np.abs(c[:, [3, 2, 1]] * vs) + np.abs(offs)
    f = np.concatenate([v, v[:, :, :3] - mean, v[:, :, :3] - cen[:, None]], -1)
    fa = np.concatenate([np.abs(v), np.abs(v[:, :, :3]) + mabs, np.abs(v[:, :, :3]) + cabs[:, None]], -1)
    mask = (np.arange(P)[None, :] < np.asarray(num_points).reshape(M, 1))[:, :, None]
    return f * mask, fa * mask


def k2_moments(f):
    return f.sum((0, 1)), np.einsum("mpj,mpk->jk", f, f)


def k2_forward(f, num_points, prm):
    """z = W f, y = relu(scale z + shift) per row; the max over the P rows with the zero padding rows included when np < P.
    -> (out [M,64], z [M,P,64], y [M,P,64], pad [64] = relu(shift))."""
    w, sc, sh = (np.asarray(prm[k], np.float64) for k in ("weight", "scale", "shift"))
    z = f @ w.T
    y = np.maximum(z * sc + sh, 0.0)
    M, P, _ = z.shape
    live = (np.arange(P)[None, :] < np.asarray(num_points).reshape(M, 1))[:, :, None]
    pad = np.maximum(sh, 0.0)
    best_real = np.where(live, y, -1.0).max(1)
    has_pad = (np.asarray(num_points).reshape(M, 1) < P)
    out = np.where(has_pad, np.maximum(best_real, pad[None]), best_real)
    return out, z, y, pad


def k2_backward(f, num_points, prm, grad, tie="kernel", fabs=None):
    """A = sum dy f_{p*} [64,10], B = sum dy [64], Cx = sum dy xhat_{p*} [64] (include/heal_amd.h), xhat = (z - mean) rstd,
    dy = grad where y* > 0.

    The arg-max row p*: FIRST occurrence among the real rows (k_pfn_backward walks p upwards and replaces on a strict `>`;
    torch.max(dim) returns the first maximal index and its gradient goes there).  The padding rows (z = 0, f = 0, y = relu(shift))
    exist when np < P and count once.
      tie="kernel": the padding row starts as the incumbent and a real row needs y > relu(shift) strictly: the padding row wins
                    ties with real rows.
      tie="torch":  the padding rows sit at p >= np, after every real row, so the first maximal index is a real row: a real row
                    wins ties with the padding rows.
    The two differ only when a real row has y equal to relu(shift) > 0 to the bit, i.e. W_c . f rounds to 0 under the shift for
    a non-zero f -- a weight row that is (still) zero, or integer fixtures like these; B and Cx agree even then (z = 0 on both
    sides), only A loses dy f_p for pillars with np < P.  tests/test_backward_refs_cpu.py counts such ties in the fixtures and
    proves the reference under the "torch" rule against autograd; the GPU tests use the "kernel" rule.
    With fabs (k2_features64) the T of the three outputs are returned too: sum |dy| fabs*, sum |dy|, sum |dy| (z|.|* + |mean|) rstd."""
    w, mu, rs = (np.asarray(prm[k], np.float64) for k in ("weight", "mean", "rstd"))
    out, z, y, pad = k2_forward(f, num_points, prm)
    M, P, _ = z.shape
    npt = np.asarray(num_points).reshape(M)
    live = (np.arange(P)[None, :] < npt[:, None])[:, :, None]
    yr = np.where(live, y, -1.0)
    p_star = yr.argmax(1)                                           # first occurrence, [M,64]
    best_real = yr.max(1)
    has_pad = (npt < P)[:, None]
    pad_wins = has_pad & ((pad[None] >= best_real) if tie == "kernel" else (pad[None] > best_real))
    dy = np.where(out > 0, np.asarray(grad, np.float64), 0.0)       # [M,64]
    mi = np.arange(M)[:, None]
    f_star = np.where(pad_wins[..., None], 0.0, f[mi, p_star])      # [M,64,10]
    z_star = np.where(pad_wins, 0.0, z[mi, p_star, np.arange(64)[None]])
    res = dict(A=np.einsum("mc,mck->ck", dy, f_star), B=dy.sum(0), Cx=(dy * (z_star - mu) * rs).sum(0), pad_wins=pad_wins,
               p_star=p_star, dy=dy)
    if fabs is not None:
        fa_star = np.where(pad_wins[..., None], 0.0, fabs[mi, p_star])
        za = np.einsum("mck,ck->mc", fa_star, np.abs(w))
        res.update(T_A=np.einsum("mc,mck->ck", np.abs(dy), fa_star), T_B=np.abs(dy).sum(0),
                   T_Cx=(np.abs(dy) * (za + np.abs(mu)) * np.abs(rs)).sum(0))
    return res


def k2_out_T(fabs, num_points, prm):
    """T of the forward output: max over the rows of |scale| sum_k |w_k| fabs_k + |shift| (relu and max are 1-Lipschitz)."""
    w, sc, sh = (np.abs(np.asarray(prm[k], np.float64)) for k in ("weight", "scale", "shift"))
    return ((fabs @ w.T) * sc + sh).max(1)


def k2_k():
    """Roundings per term of the three K2 training kernels in EPS, for M <= 16384 pillars (one pass of the grid-stride loop).

    f      : raw point features are the inputs: 0.  mean = (sum of the 32 slots) / np: pa + pb 1, a 4-level butterfly 4, the
             division 1 -> 6 of mean|pt|; point - mean: 1 more -> 7 of fabs.  centre = x * vx + offset: 2, point - centre: 1 -> 3.
             Every feature is within 7 of its fabs.
    s1     = sum f: the thread's two rows 2, wave butterfly 6, four waves 2 (the host adds blocks in float64): 7 + 10.   k_s1 = 18
    S      = sum f_j f_k by fmaf: the product carries 7 + 7, then as s1.                                                k_S  = 25
    out    : z = 10-term fmaf chain: 7 (features) + 10 of z|.| = sum |w| fabs; fmaf(z, scale, shift): 1 -> 18 of |scale| z|.| + |shift|;
             relu and max do not amplify.                                                                                k_out = 19
    A      = fmaf(dy, f*, acc) once per thread, two shuffles, four waves 2: 7 + 1 + 2 + 2.                               k_A  = 13
    B      = acc += dy: 1 + 2 + 2.                                                                                       k_B  = 6
    Cx     = fmaf(dy, (z* - mean) * rstd, acc): z 17, subtraction 1, product 1, then 1 + 2 + 2.                          k_Cx = 25
    (each with +1 for the second order).  A, B, Cx additionally assume the same arg-max row as the reference: the random fixture is
    checked (on the CPU) to have no (pillar, channel) whose two best rows are closer than twice the forward bound."""
    return dict(s1=18, S=25, out=19, A=13, B=6, Cx=25)


def k2_argmax_margin(f, fabs, num_points, prm, k=18):
    """Smallest (gap between the best and the second-best candidate of a (pillar, channel), or distance of the best pre-ReLU
    value from 0) minus twice the forward error bound of those candidates: > 0 means fp32 cannot pick another row or another
    side of the ReLU.  Candidates: the pre-ReLU values of the real rows, and `shift` for the padding rows if np < P.
    k: the forward error of a pre-ReLU value in EPS (18 for the four-pillars-per-wave kernels, see k2_k)."""
    w, sc, sh = (np.asarray(prm[k], np.float64) for k in ("weight", "scale", "shift"))
    M, P, _ = f.shape
    npt = np.asarray(num_points).reshape(M)
    v = (f @ w.T) * sc + sh                                          # pre-ReLU [M,P,64]
    b = k * EPS * ((fabs @ np.abs(w).T) * np.abs(sc) + np.abs(sh))
    worst = np.inf
    for m in range(M):
        cand, cb = v[m, :npt[m]], b[m, :npt[m]]
        if npt[m] < P:
            cand, cb = np.concatenate([cand, sh[None]]), np.concatenate([cb, np.zeros((1, 64))])
        order = np.argsort(-cand, 0)
        top, tb = np.take_along_axis(cand, order[:1], 0)[0], np.take_along_axis(cb, order[:1], 0)[0]
        worst = min(worst, float((np.abs(top) - 2 * tb).min()))
        if cand.shape[0] > 1:
            sec = np.take_along_axis(cand, order[1:2], 0)[0]
            sbd = np.take_along_axis(cb, order[1:2], 0)[0]
            gap = np.where(top > 0, top - np.maximum(sec, 0.0) - 2 * np.maximum(tb, sbd), np.inf)
            worst = min(worst, float(gap.min()))
    return worst


def k2_random(M=67, P=20, seed=11):
    """Case 7: normal coordinates, weights and statistics; random point counts in [1, P]."""
    g = np.random.default_rng(seed)
    nps = g.integers(1, P + 1, M).astype(np.int32)
    nps[:3] = (1, P, 2)
    vox = g.standard_normal((M, P, 4)) * (np.arange(P)[None, :, None] < nps[:, None, None])
    coords = np.stack([np.zeros(M), np.zeros(M), g.integers(0, 4, M), g.integers(0, 4, M)], 1).astype(np.int32)
    return vox.astype(F32), coords, nps, k2_params(seed + 1, exact=False)


def k2_exact_units(f, prm, grad_max=2):
    """Exact fixture bound in units of 1/64 (features are multiples of 1/4, their products of 1/16, scale down to 1/4 and rstd down
    to 1/2 on quarter-valued z): the largest of sum |f_j f_k| over ALL rows, max |scale z| + |shift|, and
    sum_m |dy| (|z| + |mean|) rstd -- every sum any kernel forms is a partial sum of one of these."""
    w, sc, sh, mu, rs = (np.abs(np.asarray(prm[k], np.float64)) for k in ("weight", "scale", "shift", "mean", "rstd"))
    fa = np.abs(f)
    S = np.einsum("mpj,mpk->jk", fa, fa).max()
    za = fa @ w.T
    y = (za * sc + sh).max()
    cx = (grad_max * (za.max(1) + mu) * rs).sum(0).max()
    a = (grad_max * fa.max(1)).sum(0).max()
    return 64.0 * max(S, y, cx, a)
