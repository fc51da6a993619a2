"""The LiDAR inference front end, element by element at its edges: the pillar feature net through its inference entries
(heal_pfn_pillars / heal_pfn_scatter: k_pfn for 33 <= max_points <= 64, k_pfn4 below, both with the cell -> pillar map), the canvas
gather (k_canvas<4, false> through PillarBEV.dense() and pfn_scatter(out=...)) and the pillar stem in both weight layouts
(k_pillar_stem2 "lanes", k_pillar_stem "tiles").

Every assertion is one of: torch.equal / uint32 equality with the float64 reference on a fixture that fp32 computes without
rounding; an exact zero or an exact bias; or the per-element bound |got - ref| <= k * 2^-24 * T with k derived in
tests/pillar_refs.py (k_pfn_k, stem_k) from the operation sequence.  Nothing is normalised by a tensor-wide maximum.  The references
and the fixture properties relied on here are proven on the CPU in tests/test_pillar_refs_cpu.py.

Not covered: the other k_canvas instantiations (HEAL_CANVAS_CG = 1, 2, 8, 16, 32, 64 and HEAL_CANVAS_NT) and k_pfn for
max_points <= 32 (HEAL_PFN_1PW): those switches are read once per process, and this file sets no environment and starts no child."""
import numpy as np
import pytest
import torch

from heal_amd import ops
from tests import backward_refs as B
from tests import pillar_refs as R
from tests.report import note

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def assert_bits(got, want_bits, what):
    """uint32 equality (the canvas: a gather must not touch a bit)."""
    g = bits(got)
    assert g.shape == want_bits.shape, (what, g.shape, want_bits.shape)
    bad = np.argwhere(g != want_bits)
    assert bad.size == 0, (what, len(bad), "first", tuple(bad[0]), hex(int(g[tuple(bad[0])])), hex(int(want_bits[tuple(bad[0])])))


def assert_equal(got, ref64, what):
    """torch.equal with the float64 reference, which is representable in fp32 on an exact fixture (checked); the first differing
    element goes into the message."""
    r = np.asarray(ref64, np.float64)
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r), what
    g = got.detach().cpu().numpy()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.argwhere(~(g.astype(np.float64) == r))
    assert bad.size == 0, (what, len(bad), "first", tuple(bad[0]), float(g[tuple(bad[0])]), float(r[tuple(bad[0])]))


def within(name, got, ref, bound, **tags):
    """The per-element bound; the largest err / bound goes on record before the assertion."""
    ratio = R.max_ratio(got.detach().cpu().double().numpy(), ref, bound)
    print(f"{name} {tags}: largest err / bound = {ratio:.4f}")
    note(name, ratio=ratio, **tags)
    return ratio <= 1.0


# ================================================================================================= K2 forward, inference entries
def pfn_args(vox, coords, nps, prm, n_agents, ny, nx):
    return (dev(vox), dev(coords), dev(nps), dev(prm["weight"]), dev(prm["scale"]), dev(prm["shift"]), R.K2_VOXEL, R.K2_RANGE,
            n_agents, ny, nx)


def k2_exact(vox, coords, nps, prm, n_agents, ny, nx, scatter=True):
    """Pillar features and the map of pfn_pillars, and pfn_scatter's features and canvas, bit for bit -> (PillarBEV, reference)."""
    ref, units = R.k2_forward_chunked(vox, coords, nps, prm)
    assert units < R.EXACT_LIMIT
    M = vox.shape[0]
    want_map = R.cell_map_ref(coords, M, n_agents, ny, nx)
    args = pfn_args(vox, coords, nps, prm, n_agents, ny, nx)
    pb = ops.pfn_pillars(*args)
    assert_equal(pb.pillars[:M], ref, "pfn_pillars features")
    assert np.array_equal(pb.cell_map.cpu().numpy(), want_map), "pfn_pillars map"
    if scatter:
        canvas, pillars = ops.pfn_scatter(*args, return_pillars=True)
        assert_equal(pillars, ref, "pfn_scatter features")
        assert_bits(canvas, R.canvas_ref(pillars.cpu().numpy(), want_map), "pfn_scatter canvas")      # a gather of those rows
    return pb, ref


@pytest.mark.parametrize("P", [33, 47, 48, 49, 63, 64])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 17, 67])
def test_k_pfn_exact(M, P):
    """The one-pillar-per-wave kernel (max_points > 32): partial blocks (four waves per block), slot counts on both sides of the
    lanes that hold a point, point counts 1, 2, 31, 32, 33, P - 1, P."""
    nps = R.k2_cycle(M, R.k_pfn_counts(P))
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=100 * M + P, n_agents=2, ny=4, nx=4, nps=nps)
    k2_exact(vox, coords, nps, B.k2_params(7 * M + P), 2, 4, 4)


@pytest.mark.parametrize("P", [1, 16, 17, 32])
def test_k_pfn4_exact_through_the_inference_entries(P):
    """k_pfn4 with a non-null map: equal to the reference and to pfn_features (null map, no device count) on the same input."""
    M = 67
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=P, n_agents=2, ny=4, nx=6)
    prm = B.k2_params(P + 1)
    pb, _ = k2_exact(vox, coords, nps, prm, 2, 4, 6)
    feat = ops.pfn_features(dev(vox), dev(coords), dev(nps), dev(prm["weight"]), dev(prm["scale"]), dev(prm["shift"]), R.K2_VOXEL,
                            R.K2_RANGE)
    assert torch.equal(pb.pillars[:M], feat)


def _intensity_only(P, nps, shift, w3):
    """Pillars whose z depends on the (positive) intensity alone: weight[c] = w3 on feature 3, 0 elsewhere; scale 1 (as
    _k2_intensity_only of tests/test_gpu_backward_conformance.py)."""
    M = len(nps)
    vox, coords, nps = B.k2_pillars(M, P, seed=9, nps=nps)
    g = np.random.default_rng(4)
    vox[:, :, 3] = g.integers(1, 3, (M, P)) * (np.arange(P)[None, :] < nps[:, None])
    prm = B.k2_params(3)
    prm["weight"] = np.zeros((64, 10), np.float32)
    prm["weight"][:, 3] = w3
    prm["scale"] = np.ones(64, np.float32)
    prm["shift"] = np.full(64, shift, np.float32)
    return vox, coords, nps, prm


@pytest.mark.parametrize("nps,shift,w3,want", [([1, 3, 39, 33, 2], 3.0, -1.0, 3.0), ([40] * 5, 3.0, -8.0, 0.0),
                                               ([1, 3, 39, 33, 2], -1.0, -1.0, 0.0)])
def test_k_pfn_padding_row_rule(nps, shift, w3, want):
    """P = 40.  np < P and every real row below relu(shift) = 3: exactly relu(shift); np == P and every real y = relu(3 - 8 I) = 0:
    there is no padding row, the feature is 0, not 3; shift < 0: 0."""
    vox, coords, nps, prm = _intensity_only(40, nps, shift, w3)
    pb, ref = k2_exact(vox, coords, nps, prm, 1, 4, 4)
    assert (ref == want).all()
    assert torch.equal(pb.pillars[:len(nps)], torch.full((len(nps), 64), want, device=DEV))


@pytest.mark.parametrize("P,M", [(2, 65536 + 16 + 3), (33, 32768 + 5)])
def test_grid_stride_second_pass(P, M):
    """More pillars than one pass of the launch holds (k_pfn4: 4096 blocks x 16; k_pfn: 8192 blocks x 4, with the software prefetch
    of the wave's next pillar), on a 256 x 256 grid with duplicated cells: features and map in full."""
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=P, n_agents=1, ny=256, nx=256, nps=R.k2_cycle(509, R.k_pfn_counts(P)), base=509)
    k2_exact(vox, coords, nps, B.k2_params(P), 1, 256, 256, scatter=False)


@pytest.mark.parametrize("P", [8, 40])
@pytest.mark.parametrize("count", [0, 1, 36, 37, 42])
def test_device_pillar_count(count, P):
    """Host M = 37, the live count read on the device: rows below min(count, M) equal the reference, the map is the map of that
    many rows, the canvas is zero wherever the map is -1.  Rows at or beyond the live count are not compared."""
    M, n_agents, ny, nx = 37, 2, 4, 4
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=P, n_agents=n_agents, ny=ny, nx=nx)
    prm = B.k2_params(P)
    ref, units = R.k2_forward_chunked(vox, coords, nps, prm)
    assert units < R.EXACT_LIMIT
    live = min(count, M)
    want_map = R.cell_map_ref(coords, live, n_agents, ny, nx)
    n_dev = torch.tensor([count], dtype=torch.int32, device=DEV)
    args = pfn_args(vox, coords, nps, prm, n_agents, ny, nx)
    pb = ops.pfn_pillars(*args, n_voxels_dev=n_dev)
    assert_equal(pb.pillars[:live], ref[:live], "features of the live rows")
    assert np.array_equal(pb.cell_map.cpu().numpy(), want_map)
    canvas, pillars = ops.pfn_scatter(*args, n_voxels_dev=n_dev, return_pillars=True)
    assert_equal(pillars[:live], ref[:live], "pfn_scatter features of the live rows")
    want = R.canvas_ref(pillars.cpu().numpy(), want_map)          # the map names live rows only
    assert_bits(canvas, want, "canvas")
    empty = np.broadcast_to((want_map < 0)[:, None], want.shape)
    assert not bits(canvas)[empty].any()


@pytest.mark.parametrize("P", [8, 40])
def test_no_pillars(P):
    """M = 0: the map is all -1, the canvas all +0.0."""
    prm = B.k2_params(1)
    args = pfn_args(np.zeros((0, P, 4), np.float32), np.zeros((0, 4), np.int32), np.zeros((0,), np.int32), prm, 2, 4, 6)
    pb = ops.pfn_pillars(*args)
    assert tuple(pb.cell_map.shape) == (2, 4, 6) and bool((pb.cell_map == -1).all())
    canvas = ops.pfn_scatter(*args, out=torch.full((2, 64, 4, 6), float("nan"), device=DEV))
    assert not bits(canvas).any()
    assert not bits(pb.dense()).any()


@pytest.mark.parametrize("P", [8, 40])
def test_cell_map_semantics(P):
    """3 agents on 6 x 10 (tests/pillar_refs.py cell_semantics): duplicates inside one four-pillar group, across waves and across
    blocks (the largest row wins), agents -1 and 3, y = ny, a negative flat index, agent 2's last cell, agent 0's cell 0."""
    fx = R.cell_semantics(P)
    k2_exact(fx["voxels"], fx["coords"], fx["num_points"], B.k2_params(2), fx["n_agents"], fx["ny"], fx["nx"])


@pytest.mark.parametrize("P", [8, 40])
def test_second_launch_does_not_depend_on_the_first(P):
    """Two launches on different inputs through the same workspace (pfn_scatter keeps its map there): a full map first, then three
    pillars -- every cell the first launch filled is empty again."""
    n_agents, ny, nx = 2, 4, 6
    prm = B.k2_params(4)
    vox, coords, nps = R.k2_grid_pillars(67, P, seed=1, n_agents=n_agents, ny=ny, nx=nx)
    k2_exact(vox, coords, nps, prm, n_agents, ny, nx)
    vox2, coords2, nps2 = R.k2_grid_pillars(3, P, seed=2, n_agents=n_agents, ny=ny, nx=nx)
    assert int((R.cell_map_ref(coords, 67, n_agents, ny, nx) >= 0).sum()) > 3 * 8
    k2_exact(vox2, coords2, nps2, prm, n_agents, ny, nx)


def test_k_pfn_random_floats_within_the_bound():
    """Normal data at P = 40 (k_pfn): guards against the exact fixtures being blind to something.  No (pillar, channel) has a
    near-tie between its two best rows (asserted here and on the CPU)."""
    vox, coords, nps, prm = R.k_pfn_random()
    f, fabs = B.k2_features64(vox, coords, nps)
    k = R.k_pfn_k()
    assert B.k2_argmax_margin(f, fabs, nps, prm, k=k) > 0
    ref = B.k2_forward(f, nps, prm)[0]
    pb = ops.pfn_pillars(*pfn_args(vox, coords, nps, prm, 1, 4, 4))
    assert within("k_pfn_random:out", pb.pillars[:vox.shape[0]], ref, R.EPS * k * B.k2_out_T(fabs, nps, prm), P=vox.shape[1])


# ================================================================================================================== k_canvas
@pytest.mark.parametrize("n_agents", [1, 3])
@pytest.mark.parametrize("ny,nx", R.CANVAS_SHAPES)
def test_canvas_gather_is_a_copy(n_agents, ny, nx):
    """Hand-made maps (every occupancy pattern of a 4-cell group, the all-empty fast path, the ragged last block) and pillar rows
    with negative values, -0.0, denormals and NaN payloads, compared as uint32.  The output starts as NaN: every element is
    written, empty cells are +0.0 bit for bit."""
    fx = R.canvas_fixture(n_agents, ny, nx, seed=ny + nx)
    pb = ops.PillarBEV(dev(fx["pillars"]), dev(fx["cell_map"]), n_agents, ny, nx)
    want = R.canvas_ref(fx["pillars"], fx["cell_map"])
    assert_bits(pb.dense(), want, "dense()")
    assert_bits(pb.dense(), want, "dense() again")


@pytest.mark.parametrize("P", [8, 40])
def test_scatter_into_a_prefilled_output(P):
    """pfn_scatter(out=...) with `out` full of NaN: every element is written, empty cells are +0.0."""
    n_agents, ny, nx = 3, 4, 255
    M = 300
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=P + 1, n_agents=n_agents, ny=ny, nx=nx)
    prm = B.k2_params(P)
    ref, units = R.k2_forward_chunked(vox, coords, nps, prm)
    assert units < R.EXACT_LIMIT
    out = torch.full((n_agents, 64, ny, nx), float("nan"), device=DEV)
    canvas, pillars = ops.pfn_scatter(*pfn_args(vox, coords, nps, prm, n_agents, ny, nx), return_pillars=True, out=out)
    assert canvas.data_ptr() == out.data_ptr()
    assert_equal(pillars, ref, "features")
    want_map = R.cell_map_ref(coords, M, n_agents, ny, nx)
    assert_bits(out, R.canvas_ref(pillars.cpu().numpy(), want_map), "canvas")


# ================================================================================================================ pillar stem
LAYOUTS = ["lanes", "tiles"]


def run_stem(fx, layout, w1, b1, wd, bd):
    n, ny, nx = fx["cell_map"].shape
    pb = ops.PillarBEV(dev(fx["pillars"]), dev(fx["cell_map"]), n, ny, nx)
    assert pb.stem_supported(64, 64)
    pb.weight_layout = layout
    wm, wdf = pb.fragments(dev(w1), dev(wd))
    return pb.stem_block(wm, None if b1 is None else dev(b1), wdf, None if bd is None else dev(bd))


def stem_exact(fx, layout, prm, what):
    w1, b1, wd, bd = prm
    main, ident, Tm, Ti = R.stem_ref(fx["pillars"], fx["cell_map"], w1, b1, wd, bd)
    assert R.stem_exact_units(Tm, Ti) < R.EXACT_LIMIT
    got_main, got_id = run_stem(fx, layout, w1, b1, wd, bd)
    assert_equal(got_main, main, what + ": conv1")
    assert_equal(got_id, ident, what + ": downsample")
    return (got_main, got_id), (main, ident)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ny,nx", R.STEM_SHAPES)
def test_stem_shapes_exact(ny, nx, layout):
    """Ho = 1, odd ny (the bottom tap is off the map), odd nx, Wo = 4, 12, 32, 36, 68 and Ho = 9, 5 (ragged against both tile
    shapes); two agents whose tagged cells sit where a tap that leaves the map would alias them in flat indexing."""
    fx = R.stem_fixture(R.stem_two_maps_cells(ny, nx), ny, nx, seed=ny * nx)
    stem_exact(fx, layout, R.stem_params(ny + nx), f"{ny}x{nx}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("parity", ["even", "odd"])
def test_stem_active_pixel_counts(parity, layout):
    """Thirteen one-tile agents with 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64 active pixels.  even: every pillar is seen by
    one pixel through the centre tap (both convolutions); odd: every pillar by two or four pixels through the corner taps, and the
    groups of a tile see different tap sets."""
    fx = R.stem_fixture(R.stem_count_cells(parity), R.COUNT_NY, R.COUNT_NX, seed=7)
    stem_exact(fx, layout, R.stem_params(7), parity)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ci", R.SELECT_CI)
def test_stem_selector(ci, layout):
    """One one-hot pillar per agent at each cell parity; conv1's element is the weight 1 + co + 64 tap + 576 ci that was read."""
    fx, w1, wd = R.stem_selector(ci)
    main, ident, Tm, Ti = R.stem_ref(fx["pillars"], fx["cell_map"], w1, None, wd, None)
    assert R.stem_exact_units(Tm, Ti) < R.EXACT_LIMIT
    got_main, got_id = run_stem(fx, layout, w1, None, wd, None)
    g = got_main.cpu().numpy()
    bad = np.argwhere(g != main)
    if bad.size:
        b, co, oy, ox = (int(v) for v in bad[0])
        raise AssertionError(f"{len(bad)} elements; first at agent {b} co {co} pixel ({oy}, {ox}): read (co, tap, ci) = "
                             f"{R.stem_decode(g[b, co, oy, ox])}, want {R.stem_decode(main[b, co, oy, ox])}")
    assert_equal(got_main, main, "selector conv1")
    assert_equal(got_id, ident, "selector downsample")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stem_clamped_row_read(layout):
    """Row 0 (what `max(id, 0)` reads for an empty cell) and every row the map does not reference hold NaN: nothing of them may
    reach an output."""
    for (ny, nx), cells in (((5, 8), R.stem_two_maps_cells(5, 8)), ((R.COUNT_NY, R.COUNT_NX), R.stem_count_cells("odd"))):
        fx = R.stem_fixture(cells, ny, nx, seed=ny * nx, poison=True)
        assert np.isnan(fx["pillars"][0]).all()
        stem_exact(fx, layout, R.stem_params(3), f"poisoned {ny}x{nx}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stem_background_and_bias(layout):
    """An empty agent gives relu(b1) and bd exactly; with no biases the background is +0.0."""
    ny, nx = 5, 8
    cells = [R.stem_two_maps_cells(ny, nx)[0], [], R.stem_two_maps_cells(ny, nx)[1]]
    fx = R.stem_fixture(cells, ny, nx, seed=1)
    w1, b1, wd, bd = R.stem_params(2)
    assert (b1 < 0).any() and (b1 > 0).any()
    (got_main, got_id), _ = stem_exact(fx, layout, (w1, b1, wd, bd), "with biases")
    assert_equal(got_main[1], np.broadcast_to(np.maximum(b1, 0).astype(np.float64)[:, None, None], got_main[1].shape), "relu(b1)")
    assert_equal(got_id[1], np.broadcast_to(bd.astype(np.float64)[:, None, None], got_id[1].shape), "bd")
    (got_main, got_id), _ = stem_exact(fx, layout, (w1, None, wd, None), "no biases")
    assert not bits(got_main[1]).any() and not bits(got_id[1]).any()
    empty = R.stem_fixture([[], []], ny, nx, seed=2)
    (got_main, got_id), _ = stem_exact(empty, layout, (w1, None, wd, None), "empty maps")
    assert not bits(got_main).any() and not bits(got_id).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stem_random_floats_within_the_bound(layout):
    """Normal pillars, weights and biases on 17 x 24, two agents: the per-element bound with the derived k."""
    ny, nx = 17, 24
    fx = R.stem_fixture(R.stem_occupancy_cells(ny, nx, seed=4), ny, nx, seed=5, exact=False)
    w1, b1, wd, bd = R.stem_params(6, exact=False)
    main, ident, Tm, Ti = R.stem_ref(fx["pillars"], fx["cell_map"], w1, b1, wd, bd)
    got_main, got_id = run_stem(fx, layout, w1, b1, wd, bd)
    km, ki = R.stem_k()
    ok_m = within("pillar_stem_random:conv1", got_main, main, R.EPS * km * Tm, layout=layout)
    ok_i = within("pillar_stem_random:downsample", got_id, ident, R.EPS * ki * Ti, layout=layout)
    assert ok_m and ok_i
    again_main, again_id = run_stem(fx, layout, w1, b1, wd, bd)
    assert torch.equal(again_main, got_main) and torch.equal(again_id, got_id)          # two launches are bit-equal
