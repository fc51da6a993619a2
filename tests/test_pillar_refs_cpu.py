"""CPU proofs for tests/pillar_refs.py: the references of tests/test_gpu_pillar_conformance.py equal the oracle and float64 conv2d,
every exact fixture is exact, and every hand-built fixture has the properties its GPU test relies on.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests import backward_refs as B
from tests import pillar_refs as R
from tests.golden.detfill import det_values


def _pfn_oracle_params():
    pre = "pillar_vfe.pfn_layers.0."
    return dict(weight=det_values(pre + "linear.weight", (64, 10), "weight"), bn_gamma=det_values(pre + "norm.weight", (64,), "bn_weight"),
                bn_beta=det_values(pre + "norm.bias", (64,), "bn_bias"), bn_mean=det_values(pre + "norm.running_mean", (64,), "running_mean"),
                bn_var=det_values(pre + "norm.running_var", (64,), "running_var"))


# ------------------------------------------------------------------------------------------------ cell map + canvas
def test_cell_map_and_canvas_equal_the_oracle_on_the_golden(golden):
    g = golden("pointpillar_encoder")
    v, c, n = g["voxel_features"], g["voxel_coords"], g["voxel_num_points"]
    canvas, p = O.pfn_scatter(v, c, n, voxel_size=g["voxel_size"].tolist(), lidar_range=g["lidar_range"].tolist(), n_agents=2,
                              ny=128, nx=128, **_pfn_oracle_params())
    m = R.cell_map_ref(c, len(n), 2, 128, 128)
    assert int((m >= 0).sum()) > 100
    assert np.array_equal(R.canvas_ref(p, m), canvas.view(np.uint32))
    # ... and the golden's own pillar features, gathered through the map, are the golden's canvas bit for bit
    assert np.array_equal(R.canvas_ref(g["pillar_features"], m), g["spatial_features"].view(np.uint32))


def test_cell_map_and_canvas_equal_the_oracle_with_duplicates():
    """The oracle's fancy-index assignment keeps the LAST row of a duplicated cell; so does the loop."""
    M, P = 41, 5
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=3, n_agents=2, ny=3, nx=4)
    flat = coords[:, 0].astype(np.int64) * 12 + coords[:, 2] * 4 + coords[:, 3]
    assert len(np.unique(flat)) < M
    prm = B.k2_params(5)
    f, _ = B.k2_features64(vox, coords, nps)
    p = B.k2_forward(f, nps, prm)[0].astype(np.float32)
    m = R.cell_map_ref(coords, M, 2, 3, 4)
    want = O.scatter_to_canvas(p, coords, 2, 3, 4)
    assert np.array_equal(R.canvas_ref(p, m), want.view(np.uint32))
    for cell in np.unique(flat):
        assert m.reshape(-1)[cell] == np.nonzero(flat == cell)[0].max()
    # a live count below M: the later rows do not exist
    m5 = R.cell_map_ref(coords, 5, 2, 3, 4)
    assert set(m5[m5 >= 0].tolist()) <= set(range(5)) and np.array_equal(m5, R.cell_map_ref(coords[:5], 5, 2, 3, 4))


def test_cell_semantics_fixture_has_every_case():
    fx = R.cell_semantics()
    coords, n_agents, ny, nx = fx["coords"], fx["n_agents"], fx["ny"], fx["nx"]
    c = coords.astype(np.int64)
    idx = c[:, 1] + c[:, 2] * nx + c[:, 3]
    ok = (c[:, 0] >= 0) & (c[:, 0] < n_agents) & (idx >= 0) & (idx < ny * nx)
    assert (c[:, 0] == -1).any() and (c[:, 0] == n_agents).any()
    assert ((c[:, 2] == ny) & (c[:, 0] >= 0) & (c[:, 0] < n_agents) & ~ok).any()                 # y = ny: index past the grid
    assert ((c[:, 3] < 0) & (idx < 0)).any()                                                     # negative flat index
    assert ((c[:, 0] == 2) & (idx == ny * nx - 1)).any() and ((c[:, 0] == 0) & (idx == 0)).any()
    key = np.where(ok, c[:, 0] * ny * nx + idx, -1)
    dup = [np.nonzero(key == k)[0] for k in np.unique(key[key >= 0]) if (key == k).sum() > 1]
    same_slot_group = any((r // 4 == r[0] // 4).all() for r in dup)                              # one 4-pillar group of a k_pfn4 wave
    across_waves = any(len(set(r // 4)) > 1 and len(set(r // 16)) == 1 for r in dup)            # k_pfn4: 16 pillars per block
    across_blocks = any(len(set(r // 16)) > 1 for r in dup)
    assert same_slot_group and across_waves and across_blocks
    m = R.cell_map_ref(coords, len(coords), n_agents, ny, nx)
    assert int((m >= 0).sum()) == len(np.unique(key[key >= 0]))


# ------------------------------------------------------------------------------------------------ K2 forward fixtures
@pytest.mark.parametrize("P", [33, 47, 48, 49, 63, 64])
def test_k_pfn_fixtures_are_exact_and_cover_the_counts(P):
    M = 67
    nps = R.k2_cycle(M, R.k_pfn_counts(P))
    assert {1, 2, 31, 32, 33, P - 1, P} <= set(nps)
    vox, coords, npt = R.k2_grid_pillars(M, P, seed=P, n_agents=1, ny=4, nx=4, nps=nps)
    assert np.array_equal(npt, nps) and not vox[np.arange(P)[None, :] >= npt[:, None]].any()
    _, units = R.k2_forward_chunked(vox, coords, npt, B.k2_params(P))
    assert units < R.EXACT_LIMIT


def test_placing_pillars_keeps_the_relative_features():
    vox, coords, nps = B.k2_pillars(9, 6, seed=1)
    f0, _ = B.k2_features64(vox, coords, nps)
    cells = R.random_cells(9, 3, 256, 256, 2)
    v2, c2 = R.place_pillars(vox, coords, nps, cells)
    f1, _ = B.k2_features64(v2, c2, nps)
    assert np.array_equal(f0[:, :, 2:], f1[:, :, 2:]) and np.array_equal(c2[:, [0, 2, 3]], cells)
    assert not np.array_equal(f0[:, :, :2], f1[:, :, :2])


@pytest.mark.parametrize("P,M,stride", [(2, 65536 + 16 + 3, 65536), (33, 32768 + 5, 32768)])
def test_grid_stride_fixtures(P, M, stride):
    """Exact at 256 x 256; the pillar a wave meets in its second pass differs from the one of its first (the prefetch must not
    re-read pillar m); the map has duplicates."""
    vox, coords, nps = R.k2_grid_pillars(M, P, seed=P, n_agents=1, ny=256, nx=256, nps=R.k2_cycle(509, R.k_pfn_counts(P)), base=509)
    out, units = R.k2_forward_chunked(vox, coords, nps, B.k2_params(P))
    assert units < R.EXACT_LIMIT and out.shape == (M, 64)
    assert (out[stride:] != out[:M - stride]).any(1).all()
    m = R.cell_map_ref(coords, M, 1, 256, 256)
    assert 0 < int((m >= 0).sum()) < M
    assert vox.nbytes < 21e6


def test_k_pfn_random_fixture_has_no_near_ties():
    vox, coords, nps, prm = R.k_pfn_random()
    assert 33 <= vox.shape[1] <= 64
    f, fabs = B.k2_features64(vox, coords, nps)
    assert B.k2_argmax_margin(f, fabs, nps, prm, k=R.k_pfn_k()) > 0
    assert R.k_pfn_k() == B.k2_k()["out"] + 1           # the 6-level butterfly in place of pa + pb and the 4-level one


# ------------------------------------------------------------------------------------------------ canvas fixtures
@pytest.mark.parametrize("n_agents", [1, 3])
@pytest.mark.parametrize("ny,nx", R.CANVAS_SHAPES)
def test_canvas_fixture_properties(n_agents, ny, nx):
    fx = R.canvas_fixture(n_agents, ny, nx, seed=ny + nx)
    m, p = fx["cell_map"], fx["pillars"]
    M = p.shape[0]
    ids = m[m >= 0]
    assert np.array_equal(np.sort(ids), np.arange(M)) and 0 in ids and M - 1 in ids
    groups = (m.reshape(n_agents, -1, 4) >= 0)
    pat = (groups * (1 << np.arange(4))).sum(-1)
    assert np.array_equal(pat, fx["patterns"])
    if ny * nx // 4 >= 16:
        for b in range(n_agents):
            assert set(pat[b].tolist()) == set(range(16))
        assert pat[0, -1] not in (0, 15)                   # the last group (the ragged block's thread where there is one)
    if n_agents == 3:
        assert (pat == 0).any()                             # the all-empty fast path, also with one group per agent
    bits = R.canvas_ref(p, m)
    sp = set(R.special_values().view(np.uint32).tolist())
    assert sp <= set(bits.reshape(-1).tolist())             # every special value is in a referenced row
    assert not bits[np.broadcast_to((m < 0)[:, None], bits.shape)].any()


# ------------------------------------------------------------------------------------------------ stem reference + fixtures
def _conv64(dense, w1, b1, wd, bd):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    return (torch.relu(torch.nn.functional.conv2d(t(dense), t(w1), t(b1), 2, 1)).numpy(),
            torch.nn.functional.conv2d(t(dense), t(wd), t(bd), 2, 0).numpy())


def test_stem_ref_equals_conv2d_of_the_oracle_canvas():
    M = 41
    vox, coords, nps = R.k2_grid_pillars(M, 5, seed=3, n_agents=2, ny=5, nx=8)
    f, _ = B.k2_features64(vox, coords, nps)
    p = B.k2_forward(f, nps, B.k2_params(5))[0].astype(np.float32)
    canvas = O.scatter_to_canvas(p, coords, 2, 5, 8)
    w1, b1, wd, bd = R.stem_params(1, exact=False)
    main, ident, Tm, Ti = R.stem_ref(p, R.cell_map_ref(coords, M, 2, 5, 8), w1, b1, wd, bd)
    want_main, want_id = _conv64(canvas, w1, b1, wd, bd)
    assert np.array_equal(main, want_main) and np.array_equal(ident, want_id)
    assert (Tm + 1e-12 >= np.abs(main)).all() and (Ti + 1e-12 >= np.abs(ident)).all()


def _exact(fx, prm):
    main, ident, Tm, Ti = R.stem_ref(fx["pillars"], fx["cell_map"], *prm)
    assert R.stem_exact_units(Tm, Ti) < 3500 < R.EXACT_LIMIT
    assert np.array_equal(main, np.round(main)) and np.array_equal(ident, np.round(ident))
    return main, ident


def _unreferenced_row0(fx):
    m = fx["cell_map"]
    assert 0 in fx["unreferenced"] and len(fx["unreferenced"]) >= 2 and not (m == 0).any()
    assert set(m[m >= 0].tolist()) | set(fx["unreferenced"].tolist()) == set(range(fx["pillars"].shape[0]))


@pytest.mark.parametrize("ny,nx", R.STEM_SHAPES)
def test_stem_two_maps_fixture(ny, nx):
    cells = R.stem_two_maps_cells(ny, nx)
    fx = R.stem_fixture(cells, ny, nx, seed=ny * nx)
    _exact(fx, R.stem_params(ny + nx))
    _unreferenced_row0(fx)
    occ = fx["cell_map"] >= 0
    Wo = (nx - 1) // 2 + 1
    assert Wo % 4 == 0
    assert occ[0, ny - 1].any() and occ[1, 0].any()
    if ny >= 2:
        assert not occ[0, 0].any() and not occ[1, ny - 1].any()
    if ny >= 3:
        assert occ[0, 1, nx - 1]                                      # (nx - 1, 1): the flat predecessor of (0, 2)
    assert occ[0, :, 0].any()                                         # (0, y): the flat successor of (nx - 1, y - 1)
    # a kernel that indexed the map flat, without the row / column guards, would compute something else on this fixture
    flat = np.concatenate([np.full(nx + 1, -1), fx["cell_map"].reshape(-1), np.full(nx + 1, -1)])
    leaks = 0
    for b in range(2):
        for oy in range((ny - 1) // 2 + 1):
            for ox in range(Wo):
                for t in range(9):
                    iy, ix = 2 * oy + t // 3 - 1, 2 * ox + t % 3 - 1
                    inside = 0 <= iy < ny and 0 <= ix < nx
                    leaks += (not inside) and flat[nx + 1 + (b * ny + iy) * nx + ix] >= 0
    assert leaks > 0
    # a poisoned copy differs only in unreferenced rows
    fp = R.stem_fixture(cells, ny, nx, seed=ny * nx, poison=True)
    assert np.isnan(fp["pillars"][fp["unreferenced"]]).all() and not np.isnan(fp["pillars"][fx["cell_map"][occ]]).any()
    assert np.array_equal(fp["cell_map"], fx["cell_map"])
    a, b = _exact(fp, R.stem_params(ny + nx)), _exact(fx, R.stem_params(ny + nx))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_stem_shapes_cover_the_tile_edges():
    out = {(ny, nx): ((ny - 1) // 2 + 1, (nx - 1) // 2 + 1) for ny, nx in R.STEM_SHAPES}
    assert {w for _, w in out.values()} == {4, 12, 32, 36, 68}
    assert {h for h, _ in out.values()} >= {1, 3, 9, 5, 8}
    assert any(ny % 2 for ny, _ in R.STEM_SHAPES) and any(nx % 2 for _, nx in R.STEM_SHAPES)


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_stem_count_fixture(parity):
    cells = R.stem_count_cells(parity)
    fx = R.stem_fixture(cells, R.COUNT_NY, R.COUNT_NX, seed=7)
    _exact(fx, R.stem_params(7))
    _unreferenced_row0(fx)
    bits = R.stem_tap_bits(fx["cell_map"])
    assert bits.shape == (13, 2, 32)
    # `reach` as tests/test_gpu_kernels.py computes it: a 3x3 stride-2 max-pool of the padded occupancy
    occ = torch.from_numpy((fx["cell_map"] >= 0).astype(np.float32))[:, None]
    reach = torch.nn.functional.max_pool2d(torch.nn.functional.pad(occ, (1, 1, 1, 1)), 3, 2)[:, 0].numpy() > 0
    assert np.array_equal(reach, bits != 0)
    tiles = R.stem_tile_groups(bits)
    assert [t[3] for t in tiles] == list(R.COUNTS)
    assert [len(t[4]) for t in tiles] == [(c + 15) // 16 for c in R.COUNTS]
    if parity == "even":
        assert set(np.unique(bits).tolist()) == {0, 1 << 4}                 # the centre tap alone
        assert [len(c) for c in cells] == list(R.COUNTS)
    else:
        assert not (bits & (1 << 4)).any()
        for (b, _, _, n_act, groups), cs in zip(tiles, cells):
            if n_act <= 1:
                continue
            per_pillar = [int(sum(((2 * oy + ky - 1, 2 * ox + kx - 1) == cell) for oy in range(2) for ox in range(32)
                                  for ky in range(3) for kx in range(3))) for cell in cs]
            assert set(per_pillar) <= {2, 4}, (b, per_pillar)
            tile_bits = int(np.bitwise_or.reduce(groups))
            if n_act > 32:
                assert len(set(groups)) > 1 and any(gb != tile_bits for gb in groups), (b, groups)
        assert any(len(set(t[4])) > 1 for t in tiles)


@pytest.mark.parametrize("ci", R.SELECT_CI)
def test_stem_selector_fixture(ci):
    fx, w1, wd = R.stem_selector(ci)
    main, ident, Tm, Ti = R.stem_ref(fx["pillars"], fx["cell_map"], w1, None, wd, None)
    assert R.stem_exact_units(Tm, Ti) < R.EXACT_LIMIT
    _unreferenced_row0(fx)
    bits = R.stem_tap_bits(fx["cell_map"])
    assert (np.array([bin(int(v)).count("1") for v in bits.reshape(-1)]) <= 1).all()
    seen = set()
    for b, (py, px) in enumerate(R.PARITIES):
        for oy, ox in zip(*np.nonzero(bits[b])):
            tap = int(bits[b, oy, ox]).bit_length() - 1
            assert (2 * oy + tap // 3 - 1, 2 * ox + tap % 3 - 1) == (2 + py, 2 + px)
            for co in (0, 17, 63):
                assert R.stem_decode(main[b, co, oy, ox]) == (co, tap, ci)
            seen.add(tap)
        assert ident[b].any() == ((py, px) == (0, 0))
    assert seen == set(range(9))                             # the four parities together exercise every tap
    assert ident[0, 5, 1, 1] == -(1 + 5 + 64 * ci)


def test_stem_bounded_fixture_and_constants():
    ny, nx = 17, 24
    fx = R.stem_fixture(R.stem_occupancy_cells(ny, nx, seed=4), ny, nx, seed=5, exact=False)
    _unreferenced_row0(fx)
    occ = fx["cell_map"] >= 0
    assert 0.2 < occ.mean() < 0.4
    assert R.stem_k() == (579, 67)
