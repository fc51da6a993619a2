"""CPU proofs for tests/lss_refs.py: the float64 lift-splat reference equals the project's oracle, an fp32 replay of lss_cell_key
reproduces every fixture's cell table, every exact fixture is inside its exactness budget, the cell-edge fixture diverges where it
says, the per-element bounds separate the errors the GPU suite is after, and the run-length fixtures sit where intended against the
32-point tiles of the sorted pipeline."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import lss_refs as L


def fixtures():
    """name -> (fixture, D, C): every power-of-two-grid fixture the GPU suite uses, at its smallest member per builder."""
    out = {
        "depth_d4": (L.lss_depth_fixture(4, 5, 3), 4, 16),
        "depth_d20": (L.lss_depth_fixture(20, 17, 3, yden=64), 20, 16),
        "depth_d64_h64": (L.lss_depth_fixture(64, 64, 2), 64, 16),
        "runs_main": (L.lss_column_fixture(L.RUNS_MAIN_REENTERED), 4, 16),
        "runs_bab": (L.lss_column_fixture(L.RUNS_BAB), 4, 16),
        "runs_left": (L.lss_column_fixture(L.RUNS_LEFTOVER_REENTERED), 4, 16),
        "runs_diff": (L.lss_column_fixture(L.RUNS_ALL_DIFFERENT), 4, 16),
        "faces": (L.lss_face_fixture(), 4, 16),
        "agents": (L.lss_column_fixture([1.5, 1.75, 6.5], D=4, n_agents=3, n_cams=2,
                                        cam_cells=[(0, 0, 0), (1, -1, 0), (-2, 1, 0), (2, 0, 0), (0, -1, 0), (-1, 0, 0)]), 4, 16),
        "general_two_z": (L.lss_fixture(1, 2, [(0, 0, 0), (1, 0, -1)], fpos=L.B.k4_centres(4, 2, 3, 5), nz=2), 4, 16),
    }
    for nx, ny in ((8, 8), (136, 6), (7, 4), (8, 5)):
        out[f"stem_{nx}x{ny}"] = (L.lss_stem_fixture(nx, ny), 4, 32)
    out["stem_single"] = (L.lss_stem_fixture(8, 5, "single"), 4, 32)
    out["stem_empty"] = (L.lss_stem_fixture(8, 5, "empty"), 4, 32)
    out["depth_tail"] = (L.lss_depth_fixture(16, 20, 2, yden=64), 16, 256)
    out["depth_h1"] = (L.lss_depth_fixture(16, 1, 8, yden=64), 16, 32)
    out["depth_d6"] = (L.lss_depth_fixture(6, 5, 3, yden=64), 6, 16)
    for name, (fx, D, fH, C) in L.lss_bounded_cases().items():
        out["bounded_" + name] = (fx, D, C)
    for name, (fx, _) in L.lss_run_cases().items():
        out["run_" + name] = (fx, fx["cell"].shape[1], 16)
    return out


FIXTURES = fixtures()


def oracle_pool(fx, logit, feat):
    """oracle_np.bev_pool(lss_geometry(identity cameras), lift(...)): the project's restatement of the reference."""
    na, nc = fx["n_agents"], fx["n_cams"]
    BN, D, fH, fW = logit.shape
    C = feat.shape[1]
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (na, nc, 3, 3))
    geom = O.lss_geometry(fx["frustum"], eye, fx["trans"].reshape(na, nc, 3), eye, eye, np.zeros((na, nc, 3), np.float32))
    x = O.lift(logit, feat).reshape(na, nc, C, D, fH, fW).transpose(0, 1, 3, 4, 5, 2)
    return O.bev_pool(geom, x, fx["dx"], fx["bx"], fx["nx"])


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_equals_the_oracle(name):
    """Exact data: the oracle's fp32 lift and fp64 pooling make no rounding either -> equal.  Random data: the oracle's probabilities
    are fp32 -> 1e-5 of the output scale.  `faces` and `general_two_z` have nz = 2 and pin channel z * C + c."""
    fx, D, C = FIXTURES[name]
    logit, feat, _ = L.lss_exact_data(fx, C)
    ref = L.lss_forward_reference(fx, logit, feat)
    assert np.array_equal(oracle_pool(fx, logit, feat).astype(np.float64), ref["out"])
    logit, feat = L.lss_random_data(fx, C, 1)
    ref = L.lss_forward_reference(fx, logit, feat)
    want = oracle_pool(fx, logit, feat)
    assert float(np.abs(want - ref["out"]).max()) <= 1e-5 * max(float(np.abs(want).max()), 1.0)
    assert (np.abs(ref["out"]) <= ref["T"] * (1 + 1e-12)).all()
    assert np.array_equal(ref["npts"] > 0, ref["adds"] > 0) and (ref["adds"] <= ref["npts"]).all()


def test_two_z_slices_are_both_populated():
    for name in ("faces", "general_two_z"):
        fx, D, C = FIXTURES[name]
        assert int(fx["nx"][2]) == 2
        cells = int(fx["nx"][0] * fx["nx"][1])
        valid = fx["cell"][fx["cell"] >= 0]
        assert (valid < cells).any() and (valid >= cells).any()


@pytest.mark.parametrize("name", sorted(FIXTURES) + ["edges"])
def test_fp32_replay_of_lss_cell_key_reproduces_the_cell_table(name):
    fx = L.lss_edge_fixture() if name == "edges" else FIXTURES[name][0]
    assert np.array_equal(L.lss_key_replay(fx), fx["cell"])


@pytest.mark.parametrize("name", sorted(FIXTURES) + ["edges"])
def test_exact_fixtures_are_inside_their_budget(name):
    fx, D, C = (L.lss_edge_fixture(), 4, 16) if name == "edges" else FIXTURES[name]
    for hot in sorted({1, L.lss_hot(D), 1 << (D.bit_length() - 1)}):
        logit, feat, q = L.lss_exact_data(fx, C, hot=hot)
        ref = L.lss_forward_reference(fx, logit, feat)
        assert set(np.unique(ref["p"])) <= {0.0, q}
        assert L.lss_exact_units(ref, q) < L.EXACT_LIMIT
        assert np.array_equal(ref["out"] / q, np.round(ref["out"] / q))
        assert np.array_equal(ref["out"].astype(np.float32).astype(np.float64), ref["out"])


def test_hot_bins_rotate_over_every_bin():
    for D, fH, fW in ((4, 5, 3), (20, 17, 3), (52, 4, 3), (64, 3, 3)):
        fx = L.lss_depth_fixture(D, fH, fW)
        logit, _, _ = L.lss_exact_data(fx, 16)
        assert ((logit == 0).sum(1) == L.lss_hot(D)).all()
        assert (logit == 0).any(axis=(0, 2, 3)).all()


def test_depth_fixture_gives_every_bin_of_a_column_its_own_cells():
    fx = L.lss_depth_fixture(64, 64, 2)
    cell = fx["cell"][0]
    cells_xy = 64
    assert np.array_equal(cell[:, 0, 0] // cells_xy, np.arange(64))           # bin d lands in z slice d
    assert (fx["f"][0, 63, 63, :, 1] == 8.0).all() and (cell[63, 63] == -1).all()      # fy = n exactly: dropped
    assert len(np.unique(cell[63, :, 0])) >= 8                                  # the far bin's column: a run per cell
    assert len(np.unique(cell[0, :, 0])) == 1                                   # the near bin's column: one run


def test_column_runs_are_the_patterns_named():
    cell = L.lss_column_fixture(L.RUNS_MAIN_REENTERED)["cell"][0, 0, :, 0]
    a, b, c = 1 * 8 + 2, 4 * 8 + 2, 6 * 8 + 2                                  # rows 1, 4, 6 of the image column at x cell 2
    assert cell.tolist() == [-1, -1, a, a, b, a, -1, c]
    assert L.lss_column_fixture(L.RUNS_BAB)["cell"][0, 0, :, 0].tolist() == [b, a, b]
    assert L.lss_column_fixture(L.RUNS_LEFTOVER_REENTERED)["cell"][0, 0, :, 0].tolist() == [a, b, a, b, c, b]
    assert len(set(L.lss_column_fixture(L.RUNS_ALL_DIFFERENT)["cell"][0, 0, :, 0].tolist())) == 8
    # atomic adds of the fused kernel per cell: main cell once per (bin, column), a re-entered leftover cell once per run
    fx = L.lss_column_fixture(L.RUNS_LEFTOVER_REENTERED)
    adds = L.lss_atomic_adds(fx)
    assert adds[a] == 4 and adds[b] == 4 * 3 and adds[c] == 4


def test_face_fixture_lands_where_the_issue_says():
    fx = L.lss_face_fixture()
    cell, cells = fx["cell"], 64
    ok = cell >= 0
    assert not ok[2].any() and not ok[3].any()                                  # fz = -1 and fz = n: out
    assert ok[0].any() and (cell[0][ok[0]] >= cells).all()                      # fz = 1.5: bin 1
    assert ok[1].any() and (cell[1][ok[1]] < cells).all()                       # fz = -0.5: bin 0 by truncation
    assert not ok[:, :, :, 1].any() and not ok[:, :, :, 2].any()                # fx = -1 and fx = n
    assert not ok[:, :, 1].any() and not ok[:, :, 2].any()                      # fy = -1 and fy = n
    assert (cell[0, 0, 0, 0], cell[0, 0, 3, 3], cell[0, 0, 4, 0]) == (cells, cells + 3 * 8 + 3, cells + 7 * 8)


@pytest.mark.parametrize("nx,ny", [(8, 8), (136, 6), (7, 4), (8, 5)])
def test_stem_fixture_puts_tagged_cells_where_flat_indexing_aliases_them(nx, ny):
    cell = L.lss_stem_fixture(nx, ny)["cell"]
    assert (cell >= 0).all()
    y0, y1 = cell[0] // nx, cell[1] // nx
    assert (y0 == ny - 1).any() and not (y0 == 0).any()                         # agent 0: last row tagged, first row empty
    assert (y1 == 0).any() and not (y1 == ny - 1).any()                         # agent 1: first row tagged, last row empty
    assert (cell[0] == 1 * nx + nx - 1).any()                                   # (nx-1, 1): the flat predecessor of (0, 2)
    assert (cell[0] % nx == 0).any() and (cell[0] % nx >= nx - 1).any()
    assert int((L.lss_stem_fixture(nx, ny, "single")["cell"] >= 0).sum()) == 4
    assert not (L.lss_stem_fixture(nx, ny, "empty")["cell"] >= 0).any()


def test_edge_fixture_diverges_under_the_reciprocal_and_the_guard_catches_it():
    dx, bx, nx, lo = L.lss_production_grid()
    coords, div = L.lss_edge_coords()
    print(f"edge coordinates: {len(coords)}, diverging under a * fl(1/dx): {int(div.sum())}")
    assert len(coords) == 1285 and int(div.sum()) >= 32
    assert L.lss_guard_f32(coords[div], lo[0], dx[0]).all()                     # the guard sends every one of them to the division
    fx = L.lss_edge_fixture()
    nxd, nyd = int(fx["div_x"].sum()), int(fx["div_y"].sum())
    print(f"edge fixture: {nxd} diverging coordinates on x, {nyd} on y")
    assert nxd >= 16 and nyd >= 16 and int((~fx["div_x"]).sum()) >= 4 and int((~fx["div_y"]).sum()) >= 4
    assert L.lss_guard_f32(fx["xs"][fx["div_x"]], lo[0], dx[0]).all() and L.lss_guard_f32(fx["ys"][fx["div_y"]], lo[1], dx[1]).all()
    # identity cameras: the ego coordinate is the frustum value bit for bit, and a kernel without the guard gets another table
    wrong = np.where((L.lss_cell_reciprocal_f32(fx["ys"], lo[1], dx[1], nx[1])[:, None] >= 0)
                     & (L.lss_cell_reciprocal_f32(fx["xs"], lo[0], dx[0], nx[0])[None, :] >= 0),
                     L.lss_cell_reciprocal_f32(fx["ys"], lo[1], dx[1], nx[1])[:, None] * int(nx[0])
                     + L.lss_cell_reciprocal_f32(fx["xs"], lo[0], dx[0], nx[0])[None, :], -1)
    assert int((wrong != fx["cell"][0, 0]).sum()) >= 16 * len(fx["xs"])


# ---------------------------------------------------------------------------------------------------------------- the bound
def _exceeds(fx, ref, wrong_rows, D, fH, C):
    """A wrong pooled map exceeds BOTH paths' bounds at some element."""
    bf, bs = L.lss_bounds(fx, ref, D, fH, C)
    wrong = L.lss_dense(fx, wrong_rows)
    return L.max_ratio(wrong, ref["out"], bf) > 1 and L.max_ratio(wrong, ref["out"], bs) > 1


@pytest.mark.parametrize("name", sorted(L.lss_bounded_cases()))
def test_bound_separates_the_errors_the_suite_is_after(name):
    """Each wrong result, computed by the reference itself, exceeds the per-element bound somewhere: a dropped point, a doubled
    point (the valid point whose largest term p |f| is the MEDIAN of all valid points: a typical one, not the loudest), the
    probabilities of two neighbouring bins exchanged in one pixel, two image rows exchanged in one column, two z slices exchanged."""
    fx, D, fH, C = L.lss_bounded_cases()[name]
    logit, feat = L.lss_random_data(fx, C, 7)
    ref = L.lss_forward_reference(fx, logit, feat)
    bf, bs = L.lss_bounds(fx, ref, D, fH, C)
    assert L.max_ratio(ref["out"], ref["out"], bf) == 0.0
    p, cell = ref["p"], fx["cell"]
    BN, _, _, fW = cell.shape
    term = p * np.abs(feat).max(1)[:, None]
    valid = np.argwhere(cell >= 0)
    order = np.argsort(term[cell >= 0])
    i = tuple(valid[order[len(order) // 2]])
    dropped = dict(fx, cell=cell.copy())
    dropped["cell"][i] = -1
    assert _exceeds(fx, ref, L.lss_pool(dropped, p, feat), D, fH, C)
    p2 = p.copy()
    p2[i] *= 2
    assert _exceeds(fx, ref, L.lss_pool(fx, p2, feat), D, fH, C)
    v, u = fH // 2, fW // 2
    nz = int(fx["nx"][2])
    if nz > 1:       # not `collide`: there a pixel's bins share one cell, it contributes sum_d p_d f = f wherever its row and bins sit
        # image rows v and v + 1 exchanged in one column of one camera
        f2 = feat.copy()
        f2[0, :, [v, v + 1], u] = feat[0, :, [v + 1, v], u]
        assert _exceeds(fx, ref, L.lss_pool(fx, p, f2), D, fH, C)
        # two neighbouring bins of one pixel with different cells: their probabilities exchanged
        d = next(d for d in range(D - 1) if cell[0, d, v, u] >= 0 and cell[0, d + 1, v, u] >= 0 and cell[0, d, v, u] != cell[0, d + 1, v, u])
        p3 = p.copy()
        p3[0, [d, d + 1], v, u] = p[0, [d + 1, d], v, u]
        assert _exceeds(fx, ref, L.lss_pool(fx, p3, feat), D, fH, C)
        # z slices 0 and 1 exchanged
        cells_xy = int(fx["nx"][0] * fx["nx"][1])
        r = ref["rows"].reshape(fx["n_agents"], nz, cells_xy, C).copy()
        r[:, [0, 1]] = r[:, [1, 0]]
        assert _exceeds(fx, ref, r.reshape(-1, C), D, fH, C)


def test_bounded_cases_collide_as_described():
    fx, D, fH, C = L.lss_bounded_cases()["collide"]
    valid = fx["cell"][fx["cell"] >= 0]
    assert valid.size == fx["cell"].size == 768 and len(np.unique(valid)) == 1
    for name in ("d48_h12_c64", "d20_h17_c80"):
        fx, D, fH, C = L.lss_bounded_cases()[name]
        ref = L.lss_forward_reference(fx, *L.lss_random_data(fx, C, 0))
        assert int(ref["adds"].max()) >= 3 and int((fx["cell"] < 0).sum()) > 0      # shared cells, leftover runs, dropped points
        assert (fx["cell"].shape[1], fx["cell"].shape[2]) == (D, fH)


def test_k_values():
    """The derivations, evaluated: nothing here depends on a kernel's output."""
    assert L.k_probability_fused(48) == 63 and L.k_probability_fused(20) == 59
    assert float(L.k_fused(48, 12, 1)) == 63 + 1 + 12 + 1
    assert float(L.k_sorted(48, 1)) == 19 + 12 + 1 + 1 + 1 and float(L.k_sorted(20, 330)) == 19 + 5 + 1 + 32 + 11


# ---------------------------------------------------------------------------------------------------------------- sorted runs
@pytest.mark.parametrize("name", sorted(L.lss_run_cases()))
def test_run_fixtures_sit_where_intended_against_the_tiles(name):
    fx, want = L.lss_run_cases()[name]
    sk, seg_start, seg_end, invalid = L.lss_sorted_layout(fx)
    got = [(int(c), int(seg_start[c]), int(seg_end[c])) for c in range(invalid) if seg_start[c] >= 0]
    assert got == want
    n_valid = want[-1][2] if want else 0
    assert (sk[:n_valid] < invalid).all() and (sk[n_valid:] == invalid).all()
    T = L.LSS_TILE
    if name == "tiles":
        (_, s0, e0), (_, s1, e1), (_, s2, e2), (_, s3, e3), (_, s4, e4) = want
        assert (s0 % T, e0 - s0) == (0, T)                                      # one aligned tile
        assert e1 - s1 == T + 1                                                  # 33
        assert s2 % T != 0 and e2 % T == 0 and e2 - s2 < T                       # starts mid-tile, ends on a boundary
        assert (e3 - 1) // T - s3 // T >= 10 and ((e3 - 1) // T - s3 // T) % 8 != 0      # the combine's 8-wide loop twice, ragged
        assert e4 % T == 0 and len(sk) > e4 and len(sk) % T != 0                 # last valid run ends on a boundary; invalid tail
    if name == "full":
        assert len(sk) % T == 0 and want[-1][2] == len(sk)
    if name == "tiny":
        assert len(sk) < T
    if name == "none":
        assert not want and (sk == invalid).all()
