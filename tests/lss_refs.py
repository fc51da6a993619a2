"""Float64 numpy references and hand-built fixtures of the lift-splat FORWARD conformance suite (tests/test_gpu_lss_conformance.py:
k_lss_scatter<1..4>, k_lss_canvas, k_bev_stem<32|64>, the sorted pipeline k_lss_keys / _segments / _transpose / _reduce_tiles /
_combine, and heal_camera_matrices) -- numpy only, so that tests/test_lss_refs_cpu.py can prove every reference and fixture
property on a machine without a GPU.  The conventions are those of tests/backward_refs.py, whose K4 fixture this generalises:

EXACT.  Integer features and depth probabilities in {0, 1/2^k}: every term and every partial sum, in any order, is a multiple of
one quantum and below 2^24 quanta, so fp32 -- matrix cores, atomics in any order, tile partials -- computes it without rounding and
the float64 reference must equal the kernel's output bit for bit.

PER-ELEMENT BOUND.  |got - ref| <= k * 2^-24 * T with T = sum p |f| over the points of the element's cell and k the number of fp32
roundings a term meets (k_fused, k_sorted: derived from the kernels' operation sequences, never tuned on a kernel's output).

GEOMETRY.  The fixture, not geometry code, decides the cell of every lifted point: positions are dyadic numbers on grids whose
cell size is a power of two, every operation of lss_cell_key on them is exact, and the cell table is computed from the positions
in cell units under the reference's rule (in the grid iff -1 < f < n on every axis -- `.long()` truncates toward zero, so
-1 < f < 0 is cell 0 -- and the cell is trunc(f)).  The one fixture on a grid with dx = 0.4 (lss_edge_fixture) takes its cells from
lss_cell_f32, an np.float32 emulation of the reference's IEEE division."""
import numpy as np

from oracle import oracle_np as O
from tests import backward_refs as B
from tests.backward_refs import EPS, EXACT_LIMIT, F32, TINY, max_ratio  # noqa: F401  (re-exported for the tests)

LSS_TILE = 32          # points per wave of k_lss_reduce_tiles (csrc/bev_pool.hip)
COLD = -200.0          # logit of a cold depth bin: expf(-200) and __expf(-200) are exactly 0 in fp32 (no -inf anywhere)


def _is_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(F32).astype(np.float64), a))


def _cells_of(f, n):
    """The reference's rule on cell-unit positions f [..., 3]: flat index (iz*ny + iy)*nx + ix within the agent, or -1."""
    n = np.asarray(n, np.int64)
    inside = ((f > -1) & (f < n)).all(-1)
    c = np.trunc(f).astype(np.int64)
    inside &= ((c >= 0) & (c < n)).all(-1)
    return np.where(inside, (c[..., 2] * n[1] + c[..., 1]) * n[0] + c[..., 0], -1)


# =====================================================================================================================
# fixtures
# =====================================================================================================================
def lss_fixture(n_agents, n_cams, cam_cells, fpos=None, xs=None, ys=None, ds=None, grid=None, nz=1):
    """Exact lift-splat geometry with identity rotations, intrinsics and post-rotation and zero post-translation: lss_cell_key lifts
    frustum entry (x, y, z) of camera bn to (x z, y z, z) + trans[bn].

    GENERAL mode (fpos [D,fH,fW,2], cell units, frustum z = 1): backward_refs.k4_fixture itself, on its K4 grid (nz = 1 or 2).  The
    frustum is not separable, so ops.bev_pool routes it to the sorted pipeline.

    SEPARABLE mode (xs [fW], ys [fH], ds [D], ego units): frustum[d][v][u] = (xs[u], ys[v], ds[d]) -- what the fused path requires.
    grid = ((lo, dx, n) for x, y, z) with every dx a power of two; the K4 constants are the default.  cam_cells [BN,3]: translation of
    every camera in cells (trans = cam_cells * dx).  Asserted: every frustum value, every product xs[u] ds[d] / ys[v] ds[d], every sum
    with the translation and every difference with the grid's lower edge is representable in fp32, so the kernel's fp32 arithmetic
    reproduces the float64 positions without rounding and a * fl(1 / dx) is exact.
    -> dict(frustum [D,fH,fW,3] f32, trans [BN,3] f32, dx, bx f32, nx int64, cell [BN,D,fH,fW] flat index within the agent or -1,
            f [BN,D,fH,fW,3] positions in cell units, n_agents, n_cams)."""
    BN = n_agents * n_cams
    cam_cells = np.asarray(cam_cells, np.float64).reshape(BN, 3)
    if fpos is not None:
        assert grid is None and xs is None
        return B.k4_fixture(fpos, cam_cells, n_agents, n_cams, nz=nz)
    grid = grid if grid is not None else (B.K4_X, B.K4_Y, B.K4_Z1 if nz == 1 else B.K4_Z2)
    lo = np.array([g[0] for g in grid], np.float64)
    dx = np.array([g[1] for g in grid], np.float64)
    n = np.array([g[2] for g in grid], np.int64)
    assert (np.frexp(dx)[0] == 0.5).all(), "cell sizes must be powers of two"
    xs, ys, ds = (np.asarray(a, np.float64) for a in (xs, ys, ds))
    D, fH, fW = ds.size, ys.size, xs.size
    fr = np.empty((D, fH, fW, 3))
    fr[..., 0], fr[..., 1], fr[..., 2] = xs[None, None, :], ys[None, :, None], ds[:, None, None]
    lifted = np.stack([fr[..., 0] * fr[..., 2], fr[..., 1] * fr[..., 2], fr[..., 2]], -1)
    trans = cam_cells * dx
    e = lifted[None] + trans[:, None, None, None, :]
    bx = lo + dx / 2
    for name, a in (("frustum", fr), ("lifted", lifted), ("trans", trans), ("ego", e), ("ego - lo", e - lo), ("bx", bx), ("lo", lo)):
        assert _is_f32(a), f"{name} is not exact in fp32"
    f = (e - lo) / dx
    assert _is_f32(f)
    return dict(frustum=fr.astype(F32), trans=trans.astype(F32), dx=dx.astype(F32), bx=bx.astype(F32), nx=n, cell=_cells_of(f, n), f=f,
                n_agents=n_agents, n_cams=n_cams)


def lss_depth_fixture(D, fH, fW, n_agents=1, n_cams=1, cam_cells=None, yden=1024):
    """The separable work-horse: ds[d] = d + 1 on a z axis with one bin per depth bin (nz = D, bin d at fz = d + 0.5), so the D bins
    of an image column have D different cells and a bin <-> cell mix-up is a wrong value; xs[u] = (2u + 1) / 128 and
    ys[v] = (v + 1) / yden on an 8 x 8 grid of 0.25 x 0.5 cells: fx = (2u + 1)(d + 1) / 32, fy = (v + 1)(d + 1) 2 / yden.  Near bins
    keep a column in one cell (one run, no leftover); far bins spread it over several cells (leftover runs) and push it over the far
    faces of the grid (fx >= 8 or fy >= 8: dropped), fy = 8 exactly included."""
    grid = ((0.0, 0.25, 8), (0.0, 0.5, 8), (0.5, 1.0, D))
    cam_cells = cam_cells if cam_cells is not None else [(0, 0, 0)] * (n_agents * n_cams)
    return lss_fixture(n_agents, n_cams, cam_cells, xs=(2.0 * np.arange(fW) + 1) / 128, ys=(np.arange(fH) + 1.0) / yden,
                       ds=np.arange(D) + 1.0, grid=grid)


def lss_column_fixture(rows, D=4, n_agents=1, n_cams=1, cam_cells=None, grid=None, nz=1, xcells=(2.5, 5.5)):
    """Runs along an image column by choice of ys: `rows` lists the y position (cell units) of every image row v, the image columns
    sit at x = xcells (cell units), and ds = 1 for every bin: all D bins of a column share its cells."""
    grid = grid if grid is not None else (B.K4_X, B.K4_Y, B.K4_Z1 if nz == 1 else B.K4_Z2)
    cam_cells = cam_cells if cam_cells is not None else [(0, 0, 0)] * (n_agents * n_cams)
    xs = grid[0][0] + np.asarray(xcells, np.float64) * grid[0][1]
    ys = grid[1][0] + np.asarray(rows, np.float64) * grid[1][1]
    return lss_fixture(n_agents, n_cams, cam_cells, xs=xs, ys=ys, ds=np.ones(D), grid=grid, nz=nz)


OUT = -3.5                                   # a row position outside the grid
RUNS_MAIN_REENTERED = [OUT, OUT, 1.5, 1.25, 4.5, 1.75, 9.5, 6.5]     # [out, out, A, A, B, A, out, C]
RUNS_BAB = [4.5, 1.5, 4.25]                                             # [B, A, B]
RUNS_LEFTOVER_REENTERED = [1.5, 4.5, 1.25, 4.75, 6.5, 4.25]            # [A, B, A, B, C, B]: leftover cell B entered three times
RUNS_ALL_DIFFERENT = [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5]          # fH different cells


def lss_face_fixture():
    """The truncation rule and the grid's faces on x, y and z (nz = 2, K4_Z2: the frustum's z = 1 is at fz = 1.5).  Four image
    columns at fx = -0.5 (cell 0), -1 (out), 8 = n (out), 3.5; five image rows at fy = -0.5, -1, 8, 3.5, 7.5; four cameras translated
    along z by 0, -2 (fz = -0.5: bin 0), -2.5 (fz = -1: out) and +0.5 (fz = 2 = n: out) cells."""
    return lss_column_fixture([-0.5, -1.0, 8.0, 3.5, 7.5], D=4, n_agents=1, n_cams=4, nz=2, xcells=(-0.5, -1.0, 8.0, 3.5),
                              cam_cells=[(0, 0, 0), (0, 0, -2.0), (0, 0, -2.5), (0, 0, 0.5)])


def lss_stem_fixture(nx, ny, kind="two_maps"):
    """Pooled maps for k_bev_stem on an nx x ny grid of unit cells (one z bin), two agents with one camera each, D = 4 with ds = 1.
    two_maps  the points are the product of the columns {0, 1, 3, nx/2, nx-1} and the rows {1, ny-1} (every row twice: two pixels
              per cell).  Agent 0 is not translated: its LAST row is tagged, its first is empty.  Agent 1 is translated by one row
              towards y = 0: its FIRST row is tagged, its last is empty -- a 3x3 tap that leaves agent 1's map at the top, or agent
              0's at the bottom of an odd ny, aliases a tagged cell of the neighbour in flat cell indexing.  The tagged cell
              (nx-1, 1) is the flat predecessor of (0, 2): the ix = -1 tap of the output pixel at x = 0 aliases it.  With an odd nx
              the tagged cell (0, y) is the flat successor of (nx-1, y-1): the ix = nx tap of the last output pixel aliases it.
    single    one tagged cell in agent 0, agent 1 empty.       empty     every point outside the grid."""
    grid = ((0.0, 1.0, nx), (0.0, 1.0, ny), (0.0, 2.0, 1))
    if kind == "two_maps":
        cols, rows, cams = sorted({0, 1, 3 % nx, nx // 2, nx - 1}), [1, ny - 1, 1, ny - 1], [(0, 0, 0), (0, -1, 0)]
    else:
        cols, rows = [2], [1]
        cams = [(0, 0, 0), (nx + 4, 0, 0)] if kind == "single" else [(nx + 4, 0, 0), (0, ny + 4, 0)]
    return lss_fixture(2, 1, cams, xs=np.asarray(cols) + 0.5, ys=np.asarray(rows) + 0.5, ds=np.ones(4), grid=grid)


def lss_run_fixture(D, fH, fW, runs, seed=0):
    """Sorted-path run lengths: `runs` = [(cell, count), ...] with ascending cells of the K4 grid (one agent, one camera).  The
    D*fH*fW points are dealt their cells through a random permutation (the radix sort has real work to do); the points left over are
    invalid -- on the faces f = -1 and f = n and beyond them.  After the stable sort by cell key the run of runs[i] occupies
    [sum(counts[:i]), sum(counts[:i+1])) of the sorted list, which is what places it relative to the 32-point tiles."""
    total = D * fH * fW
    cells = [c for c, _ in runs]
    assert cells == sorted(set(cells)) and sum(k for _, k in runs) <= total
    labels = np.concatenate([np.full(k, c, np.int64) for c, k in runs] + [np.full(total - sum(k for _, k in runs), -1, np.int64)])
    lab = np.empty(total, np.int64)
    lab[np.random.default_rng(seed).permutation(total)] = labels
    lab = lab.reshape(D, fH, fW)
    nxg, nyg = B.K4_X[2], B.K4_Y[2]
    fpos = np.stack([lab % nxg + 0.5, lab // nxg % nyg + 0.5], -1).astype(np.float64)
    outs = np.array([(-1.0, 3.5), (8.0, 3.5), (3.5, -1.0), (3.5, 8.0), (-2.5, 9.5)])
    bad = lab < 0
    fpos[bad] = outs[np.arange(int(bad.sum())) % len(outs)]
    fx = lss_fixture(1, 1, [(0, 0, 0)], fpos=fpos)
    assert np.array_equal(fx["cell"][0], lab)
    return fx


def lss_sorted_layout(fx):
    """What k_lss_keys + the stable radix sort + k_lss_segments produce, in numpy: (sorted keys, seg_start, seg_end, invalid key);
    key = agent * cells + cell, the invalid key = n_agents * cells sorts last; seg_start / seg_end are -1 for an empty cell."""
    cell = fx["cell"]
    cells = int(np.prod(fx["nx"]))
    invalid = fx["n_agents"] * cells
    agent = (np.arange(cell.shape[0]) // fx["n_cams"])[:, None, None, None]
    keys = np.where(cell >= 0, agent * cells + cell, invalid).reshape(-1)
    sk = keys[np.argsort(keys, kind="stable")]
    seg_start, seg_end = np.full(invalid, -1, np.int64), np.full(invalid, -1, np.int64)
    for j, k in enumerate(sk):
        if k >= invalid:
            break
        if j == 0 or sk[j - 1] != k:
            seg_start[k] = j
        seg_end[k] = j + 1
    return sk, seg_start, seg_end, invalid


# ---- cell edges on the production grid ---------------------------------------------------------------------------------------
def lss_cell_f32(e, lo, dx, n=None):
    """The reference's cell index ((e - lo) / dx).long() in np.float32 with an IEEE division: trunc(quotient); with n, the bounds
    filter too: -1 where the quotient is not in (-1, n) -- the float comparison the kernels make before converting."""
    q = (np.asarray(e, F32) - F32(lo)) / F32(dx)
    assert q.dtype == F32
    if n is None:
        return np.trunc(q).astype(np.int64)
    return np.where((q > F32(-1)) & (q < F32(n)), np.trunc(q), -1).astype(np.int64)


def lss_cell_reciprocal_f32(e, lo, dx, n):
    """The same index through a * fl(1 / dx) WITHOUT the near-integer guard of lss_cell_key: what the edge fixture must tell apart."""
    t = (np.asarray(e, F32) - F32(lo)) * (F32(1) / F32(dx))
    assert t.dtype == F32
    return np.where((t > F32(-1)) & (t < F32(n)), np.trunc(t), -1).astype(np.int64)


def lss_guard_f32(e, lo, dx):
    """lss_near_integer on t = (e - lo) * fl(1 / dx), in np.float32: True where the kernel evaluates the IEEE division."""
    t = (np.asarray(e, F32) - F32(lo)) * (F32(1) / F32(dx))
    return np.abs(t - np.rint(t)) <= F32(4e-7) * np.maximum(np.abs(t), F32(1))


def lss_production_grid():
    """dx, bx, nx of the production grid (xbound = ybound = [-51.2, 51.2, 0.4], zbound = [-10, 10, 20]) and lo = bx - dx / 2 in fp32,
    as the kernels form it."""
    dx, bx, nx = O.gen_dx_bx([-51.2, 51.2, 0.4], [-51.2, 51.2, 0.4], [-10, 10, 20.0])
    return dx, bx, nx, (bx - dx / F32(2.0)).astype(F32)


def lss_edge_coords():
    """The 257 cell edges lo + k * 0.4 of a production axis and the fp32 values up to 2 ulp either side of each
    -> (coords f32 [1285], diverges bool [1285]: the reciprocal's cell differs from the division's)."""
    dx, _, nx, lo = lss_production_grid()
    edge = (np.float64(lo[0]) + np.arange(int(nx[0]) + 1) * np.float64(dx[0])).astype(F32)
    cols = [edge]
    up, dn = edge, edge
    for _ in range(2):
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
        cols += [up, dn]
    coords = np.unique(np.stack(cols, 1).reshape(-1))
    div = lss_cell_f32(coords, lo[0], dx[0], nx[0]) != lss_cell_reciprocal_f32(coords, lo[0], dx[0], nx[0])
    return coords, div


def lss_edge_fixture(n_div=24, n_same=8):
    """Ego coordinates within 2 ulp of cell edges of the production grid, on x and on y.  With identity cameras, ds = 1 and no
    translation lss_cell_key computes ex = xs[u] and ey = ys[v] bit for bit (products with 1, sums with 0), so the frustum axes ARE
    the ego coordinates: n_div coordinates per axis where trunc(a * fl(1 / dx)) != trunc(a / dx), spread over the axis, and n_same
    of their neighbours where the two agree.  The cell table comes from lss_cell_f32 (the reference's division).  D = 4, ez = 1."""
    dx, bx, nx, lo = lss_production_grid()
    coords, div = lss_edge_coords()

    def pick(offset):
        d, s = coords[div], coords[~div]
        a = d[(np.arange(n_div) * len(d) // n_div + offset) % len(d)]
        b = s[(np.arange(n_same) * len(s) // n_same + offset) % len(s)]
        out = np.concatenate([a, b])
        assert len(np.unique(out)) == len(out)
        return out[np.random.default_rng(offset).permutation(len(out))]
    xs, ys = pick(0), pick(3)
    D = 4
    fr = np.empty((D, len(ys), len(xs), 3), F32)
    fr[..., 0], fr[..., 1], fr[..., 2] = xs[None, None, :], ys[None, :, None], F32(1)
    ix = lss_cell_f32(xs, lo[0], dx[0], nx[0])
    iy = lss_cell_f32(ys, lo[1], dx[1], nx[1])
    assert lss_cell_f32(F32(1), lo[2], dx[2], nx[2]) == 0
    cell = np.where((iy[:, None] >= 0) & (ix[None, :] >= 0), iy[:, None] * int(nx[0]) + ix[None, :], -1)
    cell = np.broadcast_to(cell, (1, D) + cell.shape).copy()
    ixr = lss_cell_reciprocal_f32(xs, lo[0], dx[0], nx[0])
    iyr = lss_cell_reciprocal_f32(ys, lo[1], dx[1], nx[1])
    return dict(frustum=fr, trans=np.zeros((1, 3), F32), dx=dx, bx=bx, nx=nx, cell=cell, f=None, n_agents=1, n_cams=1, xs=xs, ys=ys,
                div_x=ix != ixr, div_y=iy != iyr)


def lss_key_replay(fx):
    """lss_cell_key in np.float32, operation by operation in the kernel's order (identity 3x3 matrices spelled out as the products
    and sums the kernel makes), near-integer guard and IEEE division included -> the cell table [BN,D,fH,fW]."""
    fr = np.asarray(fx["frustum"], F32)
    tr = np.asarray(fx["trans"], F32)[:, None, None, None, :]
    one, zero = F32(1), F32(0)
    p = [fr[None, ..., k] - zero for k in range(3)]
    eye = [[one if r == c else zero for c in range(3)] for r in range(3)]
    mat = lambda M, a: [(M[r][0] * a[0] + M[r][1] * a[1]) + M[r][2] * a[2] for r in range(3)]
    q = mat(eye, p)
    u = [q[0] * q[2], q[1] * q[2], q[2]]
    m = mat(eye, u)
    dx, bx = np.asarray(fx["dx"], F32), np.asarray(fx["bx"], F32)
    lo, rdx = bx - dx / F32(2.0), F32(1) / dx
    inside, idx = True, []
    for k in range(3):
        e = m[k] + tr[..., k]
        a = e - lo[k]
        t = a * rdx[k]
        near = np.abs(t - np.rint(t)) <= F32(4e-7) * np.maximum(np.abs(t), one)
        f = np.where(near, a / dx[k], t)
        assert f.dtype == F32
        n = int(fx["nx"][k])
        c = np.trunc(f).astype(np.int64)
        inside = inside & (f > F32(-1)) & (f < F32(n)) & (c >= 0) & (c < n)
        idx.append(c)
    nxg = [int(v) for v in fx["nx"]]
    return np.where(inside, (idx[2] * nxg[1] + idx[1]) * nxg[0] + idx[0], -1)


# =====================================================================================================================
# data
# =====================================================================================================================
def lss_hot(D):
    """Default number of hot depth bins: a quarter of the largest power of two <= D (at least one), so that cold bins exist."""
    return max(1, (1 << (int(D).bit_length() - 1)) // 4)


def lss_exact_data(fx, C, hot=None, fmax=125, seed=0):
    """Exact inputs.  logit [BN,D,fH,fW]: 0 on `hot` (a power of two) cyclically consecutive depth bins and COLD elsewhere, so
    p = 1/hot on the hot bins and 0 elsewhere for ANY D; the block of hot bins starts at bin ((v fW + u) hot + bn) % D: it rotates with
    the pixel.  feat [BN,C,fH,fW]: integer codes (97 bn + 131 v + 37 u + 17 c + 7 seed) mod (2 fmax + 1) - fmax with a prime modulus:
    neighbouring cameras, rows, columns and channels carry different numbers, so a swapped row or channel is a wrong value.
    -> (logit f32, feat f32, quantum = 1/hot)."""
    BN, D, fH, fW = fx["cell"].shape
    H = lss_hot(D) if hot is None else hot
    assert H & (H - 1) == 0 and 1 <= H <= D
    bn, v, u = np.ogrid[:BN, :fH, :fW]
    start = ((v * fW + u) * H + bn) % D
    d = np.arange(D)[None, :, None, None]
    logit = np.where((d - start[:, None]) % D < H, 0.0, COLD).astype(F32)
    mod = 2 * fmax + 1
    assert all(m % mod for m in (97, 131, 37, 17)) and all(mod % q for q in range(2, int(mod ** 0.5) + 1))
    code = (97 * bn + 131 * v + 37 * u + 7 * seed)[:, None] + 17 * np.arange(C)[None, :, None, None]
    feat = (code % mod - fmax).astype(F32)
    return np.ascontiguousarray(logit), np.ascontiguousarray(feat), 1.0 / H


def lss_random_data(fx, C, seed):
    """logit N(0,1) clipped to [-4, 4], normal features (f32)."""
    g = np.random.default_rng(seed)
    BN, D, fH, fW = fx["cell"].shape
    return (np.clip(g.standard_normal((BN, D, fH, fW)), -4, 4).astype(F32), g.standard_normal((BN, C, fH, fW)).astype(F32))


def lss_head(logit, feat, pad=0):
    """The pixel-major head tensor [BN, fH*fW, C + D + pad] of ops.bev_pool_pm: per pixel the C features, the D logits and `pad`
    words of NaN (nothing past C + D may be read)."""
    BN, D, fH, fW = logit.shape
    C = feat.shape[1]
    head = np.full((BN, fH * fW, C + D + pad), np.nan, F32)
    head[..., :C] = feat.transpose(0, 2, 3, 1).reshape(BN, fH * fW, C)
    head[..., C:C + D] = logit.transpose(0, 2, 3, 1).reshape(BN, fH * fW, D)
    return head


# =====================================================================================================================
# reference
# =====================================================================================================================
def lss_softmax(logit):
    """softmax over the depth bins in float64.  An fp32 exponential of an argument below -150 is exactly 0 (the smallest fp32
    denormal is 2^-149 = e^-103.3), in float64 it is not: such a bin (COLD) gets the probability every fp32 softmax gives it, 0."""
    lg = np.asarray(logit, np.float64)
    x = lg - lg.max(1, keepdims=True)
    e = np.where(x < -150.0, 0.0, np.exp(x))
    return e / e.sum(1, keepdims=True)


def lss_pool(fx, p, feat):
    """sum over the points of every cell of p * f -> rows [n_agents * cells, C] float64 (cell order (iz*ny + iy)*nx + ix)."""
    cell = fx["cell"]
    cells = int(np.prod(fx["nx"]))
    agent = (np.arange(cell.shape[0]) // fx["n_cams"])[:, None, None, None]
    row, ok = agent * cells + cell, cell >= 0
    ft = np.asarray(feat, np.float64).transpose(0, 2, 3, 1)                      # [BN,fH,fW,C]
    vals = np.asarray(p, np.float64)[..., None] * ft[:, None]                    # [BN,D,fH,fW,C]
    rows = np.zeros((fx["n_agents"] * cells, ft.shape[-1]))
    np.add.at(rows, row[ok], vals[ok])
    return rows


def lss_dense(fx, rows):
    """rows [n_agents * cells, C] -> the reference's [n_agents, nz*C, ny, nx] with channel z * C + c (final[b,:,z,y,x], the z slices
    concatenated along the channels: heter_encoders.py:214-217)."""
    nx, ny, nz = (int(v) for v in fx["nx"])
    C = rows.shape[-1]
    return rows.reshape(fx["n_agents"], nz, ny, nx, C).transpose(0, 1, 4, 2, 3).reshape(fx["n_agents"], nz * C, ny, nx)


def lss_atomic_adds(fx):
    """fp32 atomic adds k_lss_scatter makes per channel of every cell [n_agents * cells]: one per image column (camera, depth bin,
    u) into the column's main cell -- the cell of its first valid point -- plus one per leftover run (consecutive rows of another
    cell; a main-cell or dropped point ends the run, so a cell that is re-entered is added to again)."""
    cell = fx["cell"]
    BN, D, fH, fW = cell.shape
    cells = int(np.prod(fx["nx"]))
    agent = np.broadcast_to((np.arange(BN) // fx["n_cams"])[:, None, None], (BN, D, fW))
    valid = cell >= 0
    first = valid.argmax(2)
    main = np.where(valid.any(2), np.take_along_axis(cell, first[:, :, None, :], 2)[:, :, 0, :], -1)      # [BN,D,fW]
    adds = np.zeros(fx["n_agents"] * cells, np.int64)
    np.add.at(adds, (agent * cells + main)[main >= 0], 1)
    left = np.where(valid & (cell != main[:, :, None, :]), cell, -1)
    prev = np.concatenate([np.full((BN, D, 1, fW), -1), left[:, :, :-1]], 2)
    starts = (left >= 0) & (left != prev)
    agent4 = np.broadcast_to((np.arange(BN) // fx["n_cams"])[:, None, None, None], cell.shape)
    np.add.at(adds, (agent4 * cells + left)[starts], 1)
    return adds


def lss_forward_reference(fx, logit, feat):
    """The lift (lss_submodule.py:129-134: softmax over the depth bins (x) features) and the splat (heter_encoders.py:161-217: every
    lifted point added to its cell, z folded into the channels) in float64, on the fixture's cell table:
        out[b, z*C + c, y, x] = sum over the points of cell (b, z, y, x) of p * f[c],  p = softmax_d(logit).
    -> dict(out [n_agents, nz*C, ny, nx], T = sum p |f| (same shape), rows / T_rows [n_agents*cells, C] (the pixel-major map),
            npts [n_agents*cells] points per cell, adds [n_agents*cells] atomic adds of the fused kernel per cell, p)."""
    p = lss_softmax(logit)
    rows = lss_pool(fx, p, feat)
    T = lss_pool(fx, p, np.abs(np.asarray(feat, np.float64)))
    cell = fx["cell"]
    cells = int(np.prod(fx["nx"]))
    agent = (np.arange(cell.shape[0]) // fx["n_cams"])[:, None, None, None]
    npts = np.bincount((agent * cells + cell)[cell >= 0], minlength=fx["n_agents"] * cells)
    return dict(out=lss_dense(fx, rows), T=lss_dense(fx, T), rows=rows, T_rows=T, npts=npts, adds=lss_atomic_adds(fx), p=p)


def lss_per_element(fx, per_cell, C):
    """A per-cell quantity [n_agents*cells] laid out like the output [n_agents, nz*C, ny, nx]."""
    return lss_dense(fx, np.repeat(np.asarray(per_cell, np.float64)[:, None], C, 1))


def lss_exact_units(ref, quantum):
    """Exactness budget of an exact fixture: every term is a multiple of quantum * 1 (p in {0, quantum}, integer f) and every partial
    sum of the terms of an element, in any order and any grouping, is bounded by T -- so T / quantum < 2^24 is all fp32 needs."""
    return float(ref["T"].max()) / quantum


# =====================================================================================================================
# roundings per term
# =====================================================================================================================
def k_probability_fused(D):
    """p of k_lss_scatter, logits in [-4, 4], in EPS = 2^-24 relative.
    x = lg - mx      one rounding of a number in (-8, 0]: half an ulp there is at most 2^-22 = 4 EPS absolute -> 4 relative on e^x.
    e = __expf(x)    = v_exp_f32(fl(x * fl(log2 e))).  The constant and the product are one rounding each of a number <= 8 * 1.4427 =
                     11.55: 23.1 EPS absolute on the exponent, ln 2 * 23.1 = 16 relative on 2^y -- the part the kernel's "2 ulp"
                     comment leaves out.  For v_exp_f32 itself the kernel guides on hand give no figure; the instruction set
                     documentation specifies the transcendental unit to 1 ulp, and this suite's convention for an exponential
                     (backward_refs) is 2 ulp = 4 EPS, which covers it.                                            e: 4 + 16 + 4 = 24
    sum              a lane adds its 4 ceil(D/16) values in sequence (zeros add exactly): at most 4 ceil(D/16) - 1 roundings of
                     positive partial sums, then two quad butterflies: 2.                           sum: 24 + 4 ceil(D/16) + 1
    inv = 1 / sum    correctly rounded division: 1.   p = e * inv: 1.
    -> 24 + (24 + 4 ceil(D/16) + 1) + 1 + 1 = 51 + 4 ceil(D/16)."""
    return 51 + 4 * ((D + 15) // 16)


def k_fused(D, fH, adds):
    """Roundings per term p f of k_lss_scatter (+ k_lss_canvas, which copies).  p: k_probability_fused.  A term then enters either
    the fp32 MFMA accumulation over the fH4 = 4 ceil(fH/4) image rows (counted as unfused: the product 1, and one rounding of a
    partial sum bounded by T per row added: fH4) or the leftover walk's acc += p * x (product 1, at most fH additions) -- fH4 + 1
    covers both.  The column's result is then added to the cell's row by one fp32 atomic per column or leftover run: every add
    rounds a partial sum bounded by T, `adds` (lss_atomic_adds, per cell) of them.
    -> k_probability_fused(D) + 1 + fH4 + adds."""
    return k_probability_fused(D) + 1 + (fH + 3) // 4 * 4 + np.asarray(adds, np.float64)


def k_sorted(D, npts):
    """Roundings per term of the sorted pipeline.
    p (k_lss_keys)   x = lg - mx: 4 (as above); expf (the library's, not the hardware instruction): 2 ulp = 4 by this suite's
                     convention -> e: 8.  den: each of the 4 depth groups adds its ceil(D/4) values in sequence (the first to 0:
                     exact), ceil(D/4) - 1 roundings, then the 4-way LDS sum: 3.  p = e / den: 1.
                                                                   -> 8 + (8 + ceil(D/4) + 2) + 1 = 19 + ceil(D/4)
    k_lss_reduce_tiles   acc += p * v with contraction off: the product 1, then the additions that follow inside the 32-point tile:
                     at most min(npts, 32) roundings of partial sums bounded by T.
    k_lss_combine    a run of npts points meets at most ceil(npts / 32) tile boundaries: one addition of partial rows each.
    npts = points of the cell (array).  -> 19 + ceil(D/4) + 1 + min(npts, 32) + ceil(npts / 32)."""
    npts = np.asarray(npts, np.float64)
    return 19 + (D + 3) // 4 + 1 + np.minimum(npts, LSS_TILE) + np.ceil(npts / LSS_TILE)


def lss_bounds(fx, ref, D, fH, C):
    """(fused bound, sorted bound) per output element: EPS * k * T."""
    kf = lss_per_element(fx, k_fused(D, fH, ref["adds"]), C)
    ks = lss_per_element(fx, k_sorted(D, ref["npts"]), C)
    return EPS * kf * ref["T"], EPS * ks * ref["T"]


# =====================================================================================================================
# shared cases (the CPU proofs and the GPU tests build the same fixtures)
# =====================================================================================================================
def lss_bounded_cases():
    """name -> (fixture, D, fH, C) of the per-element-bound tests: the two shapes of the issue on the depth fixture (two cameras
    whose columns share cells; rows spread over several cells in the far bins) and a high-collision fixture in which every depth bin
    of every pixel of both cameras lands in ONE cell (768 points)."""
    return {
        "d48_h12_c64": (lss_depth_fixture(48, 12, 4, 1, 2, yden=128), 48, 12, 64),
        "d20_h17_c80": (lss_depth_fixture(20, 17, 3, 1, 2, cam_cells=[(0, 0, 0), (1, 1, 0)], yden=64), 20, 17, 80),
        "collide": (lss_column_fixture([3.5] * 8, D=16, n_agents=1, n_cams=2, xcells=(2.5, 2.25, 2.75)), 16, 8, 32),
    }


def lss_run_cases():
    """name -> (fixture, [(cell, start, end), ...]) of the sorted pipeline's run-length tests: where each cell's run must sit in the
    sorted point list, against the 32-point tiles of k_lss_reduce_tiles.
    tiles   455 points: [0,32) a run of exactly one aligned tile; [32,65) a run of 33; [65,96) a run that starts mid-tile and ends on
            a boundary; [96,426) a run over 11 tiles (k_lss_combine adds 10 partial rows: its 8-wide loop twice, the second time
            ragged); [426,448) the last valid run, ending on a tile boundary and followed by 7 invalid keys only; 455 % 32 != 0.
    full    128 points, no invalid key: two runs of two whole tiles each, the last ending with the list.
    tiny    30 points (fewer than one tile), 5 of them invalid.
    none    60 points, every one invalid: an all-zero output."""
    def case(D, fH, fW, runs, seed):
        fx = lss_run_fixture(D, fH, fW, runs, seed)
        pos, want = 0, []
        for c, k in runs:
            want.append((c, pos, pos + k))
            pos += k
        return fx, want
    return {
        "tiles": case(5, 7, 13, [(3, 32), (12, 33), (20, 31), (33, 330), (60, 22)], 1),
        "full": case(4, 4, 8, [(0, 64), (63, 64)], 2),
        "tiny": case(2, 3, 5, [(7, 10), (8, 15)], 3),
        "none": case(3, 4, 5, [], 4),
    }
