"""Float64 references and hand-built fixtures of the LiDAR pillar-path conformance suite (tests/test_gpu_pillar_conformance.py:
k_pfn / k_pfn4 through heal_pfn_pillars and heal_pfn_scatter, k_canvas, k_pillar_stem2 / k_pillar_stem) -- numpy and CPU torch only,
so that tests/test_pillar_refs_cpu.py can prove every reference and every fixture property on a machine without a GPU.

The K2 forward arithmetic (decorated features, Linear -> BN -> ReLU -> max with the padding-row rule) is the one of
tests/backward_refs.py (k2_pillars, k2_params, k2_features64, k2_forward, k2_out_T); this module adds what the inference entries
need on top: pillars placed on larger grids with several agents, the forward-only exactness budget, the cell -> pillar map, the
canvas gather and the two stride-2 convolutions of the first BasicBlock.  EXACT and PER-ELEMENT BOUND mean what they mean in
tests/backward_refs.py; the constants k are derived in the docstrings of k_pfn_k and stem_k, none was tuned on a kernel's output."""
import numpy as np
import torch

from tests import backward_refs as B

F32 = np.float32
EPS = B.EPS
EXACT_LIMIT = B.EXACT_LIMIT
max_ratio = B.max_ratio

K2_VOXEL = B.K2_VOXEL           # unit cells in x and y: every decorated feature of a dyadic pillar stays a multiple of 1/4
K2_RANGE = B.K2_RANGE           # only the lower corner enters the kernels (the cell centres); the grid size is an argument


# =====================================================================================================================
# K2 forward on larger grids
# =====================================================================================================================
def k_pfn_counts(P):
    """The point counts the k_pfn cases cycle through: 1, 2, both sides of the 32-lane half, P - 1 and P."""
    return [min(max(c, 1), P) for c in (1, 2, 31, 32, 33, P - 1, P)]


def k2_cycle(M, counts):
    return [counts[m % len(counts)] for m in range(M)]


def place_pillars(vox, coords, nps, cells):
    """Move the dyadic pillars of backward_refs.k2_pillars to the cells `cells` [M,3] = (agent, y, x) (z stays 0): the points of a
    pillar are translated by the whole-cell offset, so every coordinate stays a multiple of 1/4 and the point - mean and
    point - centre features do not change at all.  The cells need not lie inside any grid (the map drops such pillars; their
    features are computed all the same).  -> voxels [M,P,4] f32, coords [M,4] i32."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    M, P, _ = vox.shape
    live = (np.arange(P)[None, :] < np.asarray(nps).reshape(M, 1)).astype(np.float64)
    v = np.asarray(vox, np.float64).copy()
    v[:, :, 0] += (cells[:, 2] - coords[:, 3])[:, None] * live
    v[:, :, 1] += (cells[:, 1] - coords[:, 2])[:, None] * live
    out = v.astype(F32)
    assert np.array_equal(out.astype(np.float64), v)
    c = np.stack([cells[:, 0], np.zeros(M, np.int64), cells[:, 1], cells[:, 2]], 1).astype(np.int32)
    return out, c


def random_cells(M, n_agents, ny, nx, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(0, n_agents, M), g.integers(0, ny, M), g.integers(0, nx, M)], 1)


def k2_grid_pillars(M, P, seed, n_agents, ny, nx, nps=None, base=None):
    """M dyadic pillars of P slots on random cells of n_agents ny x nx grids (duplicates happen and are wanted).  base: build only
    `base` distinct pillars and repeat them cyclically before placing them (the large-M fixtures; choose a base count that does
    not divide the launch's grid stride, so that the pillar a wave meets in its second pass differs from its first).
    -> voxels, coords, num_points as k2_pillars."""
    M0 = M if base is None else min(base, M)
    if nps is not None:
        nps = list(nps)[:M0]
    vox, coords, npt = B.k2_pillars(M0, P, seed, nps=nps)
    if M0 < M:
        idx = np.arange(M) % M0
        vox, coords, npt = vox[idx], coords[idx], npt[idx]
    vox, coords = place_pillars(vox, coords, npt, random_cells(M, n_agents, ny, nx, seed + 1))
    return vox, coords, np.ascontiguousarray(npt, np.int32)


def k2_forward_units(vox, f, prm):
    """Forward-only exactness budget in units of 1/64: the features must be multiples of 1/4 (asserted); returned is the largest of
    the sum over a pillar's slots of |coordinate| (every partial sum of the wave's butterfly for the mean is below it) and of
    |scale| sum_k |w_k f_k| + |shift| over the rows (every partial sum of the fmaf chain and the BN fmaf is below it; products are
    multiples of 1/4, scale down to 1/4 makes them multiples of 1/16).  Below EXACT_LIMIT = 2^24 fp32 computes the pillar features
    without rounding.  Unlike backward_refs.k2_exact_units this does not sum anything over the pillars, so it does not grow with M."""
    assert np.array_equal(f * 4, np.round(f * 4))
    w, sc, sh = (np.abs(np.asarray(prm[k], np.float64)) for k in ("weight", "scale", "shift"))
    y = 0.0
    for s in range(0, f.shape[0], 4096):
        y = max(y, float(((np.abs(f[s:s + 4096]) @ w.T) * sc + sh).max()))
    slots = float(np.abs(np.asarray(vox, np.float64)[:, :, :3]).sum(1).max())
    return 64.0 * max(y, slots)


def k2_forward_chunked(vox, coords, nps, prm, chunk=2048):
    """k2_features64 + k2_forward over slices of `chunk` pillars (the [M,P,64] intermediates of the large-M fixtures would not fit
    otherwise) -> (out [M,64] float64, exact units as k2_forward_units)."""
    outs, units = [], 0.0
    for s in range(0, vox.shape[0], chunk):
        sl = slice(s, s + chunk)
        f, _ = B.k2_features64(vox[sl], coords[sl], nps[sl])
        units = max(units, k2_forward_units(vox[sl], f, prm))
        outs.append(B.k2_forward(f, nps[sl], prm)[0])
    return (np.concatenate(outs) if outs else np.zeros((0, 64))), units


def k_pfn_k():
    """Roundings per term of k_pfn's pillar feature in EPS: backward_refs.k2_k's count for `out` with the one-pillar-per-wave
    kernel's mean.

    f      : raw point features are the inputs: 0.  mean = wave_sum(slot) / np: the 6-level butterfly over the 64 lanes 6 (lanes
             past P add exact zeros), the division 1 -> 7 of mean|pt| (k_pfn4: pa + pb 1, a 4-level butterfly 4, the division 1 -> 6);
             point - mean: 1 more -> 8 of fabs.  centre = x * vx + offset: 2, point - centre: 1 -> 3.  Every feature is within 8
             of its fabs; the multiplication by the 0 / 1 mask is exact.
    out    : z = 10-term fmaf chain: 8 (features) + 10 of z|.| = sum |w| fabs; fmaf(z, scale, shift): 1 -> 19 of
             |scale| z|.| + |shift| = T (backward_refs.k2_out_T); relu and max do not amplify; +1 for the second order.    k = 20"""
    return 20


def k_pfn_random(M=67, P=40, seed=21):
    """The bounded k_pfn case: backward_refs.k2_random at a slot count only k_pfn takes (33 <= P <= 64)."""
    return B.k2_random(M, P, seed)


# =====================================================================================================================
# cell map and canvas
# =====================================================================================================================
def cell_map_ref(coords, n_live, n_agents, ny, nx):
    """PointPillarScatter's addressing as a map: for the first n_live rows of coords (agent, z, y, x), in row order,
    map[agent][z + y * nx + x] = row (point_pillar_scatter.py: the index is used flat); a row whose agent is outside
    [0, n_agents) or whose index is outside [0, ny * nx) is skipped; later rows overwrite earlier ones; every other cell is -1.
    -> int32 [n_agents, ny, nx]."""
    m = np.full((n_agents, ny * nx), -1, np.int32)
    c = np.asarray(coords, np.int64)
    for r in range(min(int(n_live), c.shape[0])):
        a, idx = int(c[r, 0]), int(c[r, 1] + c[r, 2] * nx + c[r, 3])
        if 0 <= a < n_agents and 0 <= idx < ny * nx:
            m[a, idx] = r
    return m.reshape(n_agents, ny, nx)


def cell_semantics(P=8, seed=6):
    """48 pillars on 3 agents of 6 x 10 cells, one for every rule of the map.  Rows are numbered as the kernels group them (k_pfn4:
    4 pillars per wave, 16 per block; k_pfn: one per wave, 4 per block).
      duplicates  rows 0 and 2 (one 4-pillar group), 5 and 9 (two waves of a block), 3 and 40 (two blocks), 1, 18 and 35 (three
                  blocks): the largest row wins
      dropped     row 6 agent -1, row 7 agent 3; row 10 y = ny (index 62), row 15 (y = ny, x = 0: index ny * nx exactly);
                  row 11 x = -3 in row 0 (index -3)
      kept        row 12 x = -2 in row 1: the index 8 is inside the grid, the reference writes cell (0, 8); row 13 agent 2's last
                  cell; row 14 agent 0's cell 0
    -> dict(voxels, coords, num_points, n_agents, ny, nx)."""
    n_agents, ny, nx, M = 3, 6, 10, 48
    g = np.random.default_rng(seed)
    special = [11, 60 + 23, 120 + 7, 44, 60 + 8, 179, 0]           # the cells named above: every other pillar has a cell of its own
    flat = g.permutation(n_agents * ny * nx)
    flat = flat[~np.isin(flat, special)][:M]
    cells = np.stack([flat // (ny * nx), flat // nx % ny, flat % nx], 1)
    for rows, cell in (((0, 2), (0, 1, 1)), ((5, 9), (1, 2, 3)), ((3, 40), (2, 0, 7)), ((1, 18, 35), (0, 4, 4)), ((6,), (-1, 2, 2)),
                       ((7,), (3, 2, 2)), ((10,), (1, ny, 2)), ((15,), (0, ny, 0)), ((11,), (0, 0, -3)), ((12,), (1, 1, -2)),
                       ((13,), (2, ny - 1, nx - 1)), ((14,), (0, 0, 0))):
        cells[list(rows)] = cell
    vox, coords, nps = B.k2_pillars(M, P, seed)
    vox, coords = place_pillars(vox, coords, nps, cells)
    return dict(voxels=vox, coords=coords, num_points=nps, n_agents=n_agents, ny=ny, nx=nx)


def canvas_ref(pillars, cell_map):
    """canvas[b, c, y, x] = pillars[map[b, y, x], c] where the map is >= 0, +0.0 elsewhere -- as BIT PATTERNS (uint32
    [n, C, ny, nx]): a gather moves -0.0, denormals and NaN payloads unchanged."""
    bits = np.ascontiguousarray(pillars, F32).view(np.uint32)
    n, ny, nx = cell_map.shape
    out = np.zeros((n, bits.shape[1], ny, nx), np.uint32)
    for b in range(n):
        yy, xx = np.nonzero(cell_map[b] >= 0)
        out[b][:, yy, xx] = bits[cell_map[b][yy, xx]].T
    return out


def special_values():
    """Values a copy must not touch: negative, -0.0, the smallest and a mid-range denormal of both signs, quiet NaNs with a payload."""
    return np.array([0xBF800000, 0x80000000, 0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x7FC12345, 0xFFC00001],
                    np.uint32).view(F32)


def canvas_pattern(t, b):
    """Occupancy bits of the 4-cell group t of agent b (bit j = cell 4 t + j holds a pillar)."""
    return (t + 3 * b + 10) % 16


CANVAS_SHAPES = ((2, 2), (4, 255), (32, 32), (4, 257))        # cells / 4 = 1, 255, 256, 257: one thread, one short of a block,
                                                               # exactly a block, one thread in a ragged second block


def canvas_fixture(n_agents, ny, nx, seed, C=64):
    """A hand-made map whose 4-cell groups follow canvas_pattern (all 16 patterns as soon as an agent has 16 groups; the all-empty
    group, whose thread takes the kernel's fast path, is among them; with 3 agents of a single group they are 10, 13 and 0) and
    pillar rows that are each referenced once, in a random order -- rows 0 and M - 1 included.  Row values: normal floats with
    special_values() written into row 0, row M - 1 and a middle row.  -> dict(pillars [M,C] f32, cell_map [n,ny,nx] i32)."""
    assert (ny * nx) % 4 == 0
    g = np.random.default_rng(seed)
    groups = ny * nx // 4
    pat = np.array([[canvas_pattern(t, b) for t in range(groups)] for b in range(n_agents)])
    occ = ((pat[:, :, None] >> np.arange(4)[None, None, :]) & 1).astype(bool).reshape(n_agents, ny * nx)
    M = int(occ.sum())
    cell_map = np.full((n_agents, ny * nx), -1, np.int32)
    cell_map[occ] = g.permutation(M).astype(np.int32)
    pillars = g.standard_normal((max(M, 1), C)).astype(F32)
    sp = special_values()
    for r in {0, M // 2, max(M - 1, 0)}:
        at = g.permutation(C)[:sp.size]
        pillars[r, at] = sp
    return dict(pillars=pillars, cell_map=cell_map.reshape(n_agents, ny, nx), patterns=pat)


# =====================================================================================================================
# pillar stem: relu(conv3x3 stride 2 pad 1 + b1), conv1x1 stride 2 + bd of the canvas the map stands for
# =====================================================================================================================
def stem_ref(pillars, cell_map, w1, b1, wd, bd):
    """Densify (canvas_ref) and convolve in float64 -> (main, ident, T_main, T_ident), each [n, 64, Ho, Wo] float64;
    T = conv(|x|, |w|) + |b|, the sum of the absolute terms of every element.  b1 / bd may be None."""
    Fn = torch.nn.functional
    x = torch.from_numpy(canvas_ref(pillars, cell_map).view(F32).astype(np.float64))
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))     # noqa: E731
    ta = lambda a: None if a is None else torch.from_numpy(np.abs(np.ascontiguousarray(a, np.float64)))     # noqa: E731
    main = torch.relu(Fn.conv2d(x, t(w1), t(b1), stride=2, padding=1))
    ident = Fn.conv2d(x, t(wd), t(bd), stride=2)
    T_main = Fn.conv2d(x.abs(), ta(w1), ta(b1), stride=2, padding=1)
    T_id = Fn.conv2d(x.abs(), ta(wd), ta(bd), stride=2)
    return main.numpy(), ident.numpy(), T_main.numpy(), T_id.numpy()


def stem_k():
    """Roundings per term of the two stem kernels in EPS -> (k_main, k_ident).  The classical bound of a floating-point sum
    suffices, whatever the order inside the matrix instructions: a term w * x is rounded once as a product and once by every
    addition it passes through, and it passes through fewer additions than there are terms in its accumulator.  conv1 adds 9 taps
    x 64 channels = 576 terms, split over two partial accumulators (even / odd k-steps) that are merged by one addition, then the
    bias is added: at most 576 + 1 + 1 roundings per term, +1 for the second order.  The downsample adds 64 terms the same way:
    64 + 1 + 1 + 1.  ReLU does not amplify."""
    return 9 * 64 + 3, 64 + 3


def stem_params(seed, exact=True):
    """w1 [64,64,3,3], b1 [64], wd [64,64,1,1], bd [64] float32.  exact: integer weights in [-2, 2] and integer biases in [-3, 3]
    (with integer pillar rows in [-3, 3] every partial sum is an integer below 9 * 64 * 6 + 3 = 3459); else normal."""
    g = np.random.default_rng(seed)
    if exact:
        w1, wd = g.integers(-2, 3, (64, 64, 3, 3)), g.integers(-2, 3, (64, 64, 1, 1))
        b1, bd = g.integers(-3, 4, 64), g.integers(-3, 4, 64)
    else:
        w1, wd = g.standard_normal((64, 64, 3, 3)) / 24.0, g.standard_normal((64, 64, 1, 1)) / 8.0
        b1, bd = g.standard_normal(64), g.standard_normal(64)
    return tuple(np.ascontiguousarray(a, F32) for a in (w1, b1, wd, bd))


def stem_exact_units(T_main, T_id):
    """Largest sum of absolute terms (integers): below 3 500 by construction, asserted against EXACT_LIMIT by the tests."""
    return float(max(T_main.max(), T_id.max()))


def stem_fixture(cells, ny, nx, seed, spare=3, poison=False, exact=True):
    """A hand-made map: cells[b] = the (y, x) cells of agent b that hold a pillar.  Every such cell gets a pillar row of its own;
    the rows are dealt in a random order from 1 .. M - 1, so that row 0 -- the row the kernels' clamped `max(id, 0)` read touches
    for an empty cell -- and `spare` further rows are referenced by nobody.  Rows: integers in [-3, 3] (exact) or normal floats.
    poison: the unreferenced rows hold NaN (a product with them, even by a zero weight, would show).
    -> dict(pillars [M,64] f32, cell_map [n,ny,nx] i32, unreferenced [rows])."""
    g = np.random.default_rng(seed)
    n = len(cells)
    total = sum(len(c) for c in cells)
    M = total + 1 + spare
    ids = 1 + g.permutation(M - 1)[:total]
    pillars = (g.integers(-3, 4, (M, 64)) if exact else g.standard_normal((M, 64))).astype(F32)
    cell_map = np.full((n, ny, nx), -1, np.int32)
    k = 0
    for b, cs in enumerate(cells):
        assert len(set(cs)) == len(cs)
        for (y, x) in cs:
            assert 0 <= y < ny and 0 <= x < nx
            cell_map[b, y, x] = ids[k]
            k += 1
    unref = np.setdiff1d(np.arange(M), ids)
    if poison:
        pillars[unref] = np.nan
    return dict(pillars=pillars, cell_map=cell_map, unreferenced=unref)


STEM_SHAPES = ((1, 8), (5, 8), (4, 7), (17, 24), (16, 64), (6, 136), (9, 72))


def stem_two_maps_cells(ny, nx):
    """Two agents laid out as lss_refs.lss_stem_fixture lays out its pooled maps: columns {0, 1, 3, nx / 2, nx - 1}; agent 0 holds
    them in row 1 and in its LAST row (its first row is empty), agent 1 in its FIRST row and in row ny - 2 (its last row is empty).
    In flat cell indexing the iy = -1 tap of agent 1's top output row aliases agent 0's tagged last row, the iy = ny tap of agent
    0's bottom output row (odd ny) aliases agent 1's tagged first row, the ix = -1 tap of output pixel (x = 0, y = 1) aliases the
    tagged cell (nx - 1, 1), and with an odd nx the ix = nx tap of the last output pixel aliases the tagged cell (0, y + 1).
    With ny = 1 both agents hold the columns in their only row (with different pillar rows)."""
    cols = sorted({0, 1, 3 % nx, nx // 2, nx - 1})
    rows0 = sorted({min(1, ny - 1), ny - 1})
    rows1 = sorted({0, max(ny - 2, 0)})
    return [[(y, x) for y in rows0 for x in cols], [(y, x) for y in rows1 for x in cols]]


def stem_occupancy_cells(ny, nx, seed, p=0.3):
    """A random map with about p of the cells occupied (the bounded case)."""
    g = np.random.default_rng(seed)
    occ = g.random((2, ny, nx)) < p
    return [[(int(y), int(x)) for y, x in zip(*np.nonzero(occ[b]))] for b in range(2)]


COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)      # both sides of every 16-pixel group edge of a 64-pixel tile
COUNT_NY, COUNT_NX = 4, 64                                        # Ho x Wo = 2 x 32: exactly one tile of k_pillar_stem2


def stem_count_cells(parity, seed=0):
    """Thirteen agents of 4 x 64 cells, agent i with COUNTS[i] active output pixels.
    parity "even": COUNTS[i] pillars on even-even cells (2 oy, 2 ox) of a random pixel subset -- each is seen by its own pixel
             alone, through the centre tap.
    parity "odd":  pillars on odd-odd cells.  (1, 2 j + 1) is seen by the pixels (0, j), (0, j + 1) through taps 6 and 8 and by
             (1, j), (1, j + 1) through taps 0 and 2; (3, 2 j + 1) by (1, j), (1, j + 1) through taps 6 and 8.  For a count c = a + b
             (a <= b active columns 0 .. a - 1 of pixel row 0 and 0 .. b - 1 of row 1; a = 0 or a >= 2) the pillars are (1, 2 j + 1),
             j < a - 1 and (3, 2 j + 1), max(a - 1, 0) <= j < b - 1: every pillar reaches two or four pixels, and the 16-pixel groups
             of the compacted list see different tap sets.  The only exception is c = 1: one pillar in the corner cell (3, 63), which
             only pixel (1, 31) sees (tap 8)."""
    g = np.random.default_rng(seed)
    cells = []
    for c in COUNTS:
        if parity == "even":
            px = np.sort(g.permutation(64)[:c])
            cells.append([(2 * int(p // 32), 2 * int(p % 32)) for p in px])
        elif c == 1:
            cells.append([(3, 63)])
        elif c == 0:
            cells.append([])
        else:
            a = 0 if c <= 32 else max(c - 32, 2)      # 33 = 2 + 31, 47 = 15 + 32, 48 = 16 + 32, ... 64 = 32 + 32
            b = c - a
            assert (a == 0 or a >= 2) and a <= b <= 32 and b >= 2
            cells.append([(1, 2 * j + 1) for j in range(a - 1)] + [(3, 2 * j + 1) for j in range(max(a - 1, 0), b - 1)])
    return cells


def stem_tap_bits(cell_map):
    """Per output pixel the 9-bit set of taps (bit ky * 3 + kx) under which the pixel sees a pillar -> int [n, Ho, Wo].  Computed as
    tests/test_gpu_kernels.py computes `reach`: the occupancy padded by one cell, one stride-2 window per pixel -- a 3x3 stride-2
    max-pool of the occupancy is `bits != 0`."""
    occ = (np.asarray(cell_map) >= 0)
    n, ny, nx = occ.shape
    Ho, Wo = (ny - 1) // 2 + 1, (nx - 1) // 2 + 1
    pad = np.zeros((n, 2 * Ho + 1, 2 * Wo + 1), bool)
    pad[:, 1:ny + 1, 1:nx + 1] = occ
    bits = np.zeros((n, Ho, Wo), np.int64)
    for ky in range(3):
        for kx in range(3):
            bits |= pad[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].astype(np.int64) << (ky * 3 + kx)
    return bits


def stem_tile_groups(bits, th=2, tw=32):
    """What k_pillar_stem2's prologue makes of a map: per th x tw tile (pixel p = row * tw + column inside the tile, ascending) the
    compacted list of active pixels, cut into groups of 16 -> list of (agent, ty, tx, n_act, [tap set of each group])."""
    n, Ho, Wo = bits.shape
    out = []
    for b in range(n):
        for ty in range(0, Ho, th):
            for tx in range(0, Wo, tw):
                tile = bits[b, ty:ty + th, tx:tx + tw]
                full = np.zeros((th, tw), np.int64)
                full[:tile.shape[0], :tile.shape[1]] = tile
                act = full.reshape(-1)[full.reshape(-1) != 0]
                groups = [int(np.bitwise_or.reduce(act[s:s + 16])) for s in range(0, act.size, 16)]
                out.append((b, ty // th, tx // tw, int(act.size), groups))
    return out


SELECT_CI = (0, 15, 16, 31, 32, 63)
SELECT_NY, SELECT_NX = 6, 8
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))


def stem_selector(ci):
    """Four agents of 6 x 8 cells, agent i with ONE pillar at the cell (2 + py, 2 + px) of parity PARITIES[i], whose row is one-hot
    in channel ci.  W1[co][ci][tap] = 1 + co + 64 tap + 576 ci (at most 36 864: exact), Wd[co][ci] = -(1 + co + 64 ci), no bias:
    an output pixel sees the pillar under at most one tap, so conv1's element IS the weight that was read, and (value - 1) names
    (co, tap, ci) -- see stem_decode.  -> (fixture, w1, wd)."""
    cells = [[(2 + py, 2 + px)] for py, px in PARITIES]
    fx = stem_fixture(cells, SELECT_NY, SELECT_NX, seed=ci, spare=2)
    for b in range(4):
        r = fx["cell_map"][b].max()
        fx["pillars"][r] = 0
        fx["pillars"][r, ci] = 1
    co, cin, tap = np.arange(64)[:, None, None], np.arange(64)[None, :, None], np.arange(9)[None, None, :]
    w1 = (1 + co + 64 * tap + 576 * cin).astype(F32).reshape(64, 64, 3, 3)
    wd = (-(1 + co + 64 * cin)).astype(F32)[:, :, 0].reshape(64, 64, 1, 1)
    return fx, w1, wd


def stem_decode(v):
    """(co, tap, ci) of a conv1 value of the selector fixture, or None for 0."""
    v = int(round(float(v)))
    if v <= 0:
        return None
    v -= 1
    return v % 64, v // 64 % 9, v // 576
