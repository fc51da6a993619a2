"""The lift-splat FORWARD kernels of csrc/bev_pool.hip, element by element at their edges: k_lss_scatter<1..4> + k_lss_canvas (the
fused path, ops.bev_pool_pm on a hand-built pixel-major head), k_bev_stem<32|64>, the sorted pipeline (k_lss_keys, k_lss_segments,
k_lss_transpose, k_lss_reduce_tiles<1|2|4>, k_lss_combine<1|2|4>: ops.bev_pool under HEAL_LSS_PATH=sorted or by routing) and
heal_camera_matrices.

Every assertion is one of: torch.equal with the float64 reference on a fixture that fp32 computes without rounding; an exact
zero; or the per-element bound |got - ref| <= k * 2^-24 * T with k derived in tests/lss_refs.py (k_fused, k_sorted) from the
kernels' operation sequences.  Nothing is normalised by a tensor-wide maximum and no cell may be wrong.  The references and the
fixture properties relied on here are proven on the CPU in tests/test_lss_refs_cpu.py.

Instantiations: k_lss_scatter<1> D = 4, 16; <2> D = 20, 32; <3> D = 36, 48; <4> D = 52, 64 (test_fused_depth_instantiations).
k_lss_reduce_tiles / k_lss_combine <1> C = 16, 64; <2> C = 80, 128; <4> C = 144, 256 (test_sorted_run_lengths).  k_bev_stem<32>
C = 32, 96; <64> C = 64, 128 (test_bev_stem_exact)."""
import numpy as np
import pytest
import torch

from heal_amd import ops
from tests import lss_refs as L
from tests.report import note

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_equal(got, ref64, what=""):
    """Bit for bit: the float64 reference is representable in fp32 on an exact fixture (checked), and equals the kernel's output."""
    ref64 = torch.from_numpy(np.ascontiguousarray(np.asarray(ref64, np.float64)))
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64), "the reference is not representable in fp32"
    got = got.detach().cpu().float()
    assert got.shape == ref32.shape, (what, tuple(got.shape), tuple(ref32.shape))
    if not torch.equal(got, ref32):
        bad = torch.nonzero((got != ref32) | torch.isnan(got))
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; first at {i}: got {float(got[i])!r}, "
                             f"want {float(ref32[i])!r}")


def within(name, got, ref, bound, **tags):
    """The per-element bound; the largest err / bound goes on record before the assertion."""
    ratio = L.max_ratio(got.detach().cpu().double().numpy(), ref, bound)
    print(f"{name} {tags}: largest err / bound = {ratio:.4f}")
    note(name, ratio=ratio, **tags)
    return ratio <= 1.0


def cam_mats(fx):
    """Camera matrices from the project's own entry point: identity rotations, intrinsics and post-rotation, zero post-translation,
    the fixture's translations -- and they come out as exactly that."""
    na, nc = fx["n_agents"], fx["n_cams"]
    eye = torch.eye(3, device=DEV).expand(na, nc, 3, 3).contiguous()
    cam = ops.camera_matrices(eye, dev(fx["trans"]).view(na, nc, 3), eye, eye, torch.zeros((na, nc, 3), device=DEV))
    i9 = torch.eye(3).reshape(1, 9).expand(na * nc, 9)
    want = torch.cat([i9, i9, torch.zeros((na * nc, 3)), torch.from_numpy(fx["trans"]), torch.zeros((na * nc, 3))], 1)
    assert torch.equal(cam.cpu(), want)
    return cam


def grid_args(fx):
    return [float(v) for v in fx["dx"]], [float(v) for v in fx["bx"]], [int(v) for v in fx["nx"]]


def run_fused(fx, logit, feat, pad=0, pooled=False):
    """ops.bev_pool_pm (k_lss_scatter + k_lss_canvas) on the pixel-major head [BN, fH*fW, C + D + pad]."""
    BN, D, fH, fW = logit.shape
    return ops.bev_pool_pm(dev(L.lss_head(logit, feat, pad)), feat.shape[1], D, fH, fW, dev(fx["frustum"]), cam_mats(fx),
                           fx["n_agents"], fx["n_cams"], *grid_args(fx), pooled=pooled)


def run_pool(fx, logit, feat):
    """ops.bev_pool on the reference's NCHW tensors: fused or sorted by routing / HEAL_LSS_PATH."""
    return ops.bev_pool(dev(logit), dev(feat), dev(fx["frustum"]), cam_mats(fx), fx["n_agents"], fx["n_cams"], *grid_args(fx))


def pm_workspace(fx, C):
    """(generation consumed, tag published, flags[2], rows[2]) of the fused path's workspace for this problem shape (carve_pm,
    csrc/bev_pool.hip: 64 state words, two flag arrays, two row arrays, each 256-B aligned)."""
    nx = [int(v) for v in fx["nx"]]
    ws = ops._WS[(("bev_pool_pm", fx["n_agents"], C, nx[0], nx[1], nx[2]), 0, torch.cuda.current_stream().cuda_stream)]
    n_cells = fx["n_agents"] * nx[0] * nx[1] * nx[2]
    al = lambda n: (n + 255) // 256 * 256
    words = ws.view(torch.int32)
    off, flags, rows = 256, [], []
    for _ in range(2):
        flags.append(ws[off:off + n_cells * 4].view(torch.int32)); off += al(n_cells * 4)
    for _ in range(2):
        rows.append(ws[off:off + n_cells * C * 4].view(torch.float32).view(n_cells, C)); off += al(n_cells * C * 4)
    return int(words[0].item()), int(words[1].item()), flags, rows


def check_workspace(fx, C, ref, rows_exact=True):
    """After a consumed call of generation g: half g & 1 holds exactly the pooled rows, tagged are exactly the cells that hold a
    point, and the other half is all zero.  -> g"""
    gen, tag, flags, rows = pm_workspace(fx, C)
    assert gen >= 1 and tag == gen
    tagged = (flags[gen & 1] == gen).cpu()
    assert torch.equal(tagged, torch.from_numpy(ref["npts"] > 0)), "tagged cells != cells that hold a point"
    if rows_exact:
        assert_equal(rows[gen & 1], ref["rows"], "workspace rows")
    assert int(torch.count_nonzero(rows[gen & 1][~tagged.to(DEV)])) == 0, "an untagged row is not zero"
    assert int(torch.count_nonzero(rows[(gen & 1) ^ 1])) == 0, "the other half is not all zero"
    return gen


def fused_exact(fx, C, hot=None, pad=0, fmax=125, what=""):
    logit, feat, q = L.lss_exact_data(fx, C, hot=hot, fmax=fmax)
    ref = L.lss_forward_reference(fx, logit, feat)
    assert L.lss_exact_units(ref, q) < L.EXACT_LIMIT and int(ref["npts"].sum()) > 0
    out = run_fused(fx, logit, feat, pad)
    assert_equal(out, ref["out"], what)
    check_workspace(fx, C, ref)
    return out, ref


# ============================================================================================================ fused, exact
@pytest.mark.parametrize("D,fH", [(4, 5), (16, 64), (20, 17), (32, 12), (36, 7), (48, 12), (52, 9), (64, 64)])
def test_fused_depth_instantiations(D, fH):
    """k_lss_scatter<1..4>, full and ragged last m-tiles, D / 4 not a multiple of 4; D * fH = 4 * blockDim at (16, 64) and (64, 64).
    Bin d of every column has its own z slice: a bin <-> cell mix-up is a wrong value."""
    if fH == 64:
        assert D * fH == 4 * 256 * ((D + 15) // 16)
    fx = L.lss_depth_fixture(D, fH, 3, yden=1 << ((D * fH // 4).bit_length() - 1))       # the farthest point at fy >= 8: dropped
    assert (fx["cell"] < 0).any() and int(L.lss_atomic_adds(fx).max()) > 1                  # dropped points, shared cells
    fused_exact(fx, 32, what=f"D={D} fH={fH}")


@pytest.mark.parametrize("fH", [1, 3, 4, 15, 16, 17, 33, 64])
def test_fused_image_heights(fH):
    """Zero-padded rows up to fH4, one to four softmax waves, k-steps clamped to fH4 / 4 - 1."""
    fx = L.lss_depth_fixture(16, fH, 8, yden=64)
    fused_exact(fx, 32, what=f"fH={fH}")


@pytest.mark.parametrize("C", [16, 48, 80, 256])
def test_fused_channels(C):
    """Channel tiles that do not divide by the four tile waves; the leftover walk's 64-channel passes under c < Cb."""
    fx = L.lss_depth_fixture(20, 17, 3, yden=64)
    assert int((L.lss_atomic_adds(fx) > 0).sum()) > 20
    fused_exact(fx, C, what=f"C={C}")


@pytest.mark.parametrize("D,fH,C", [(16, 20, 256), (32, 64, 256)])
def test_fused_staging_tail_loop(D, fH, C):
    """Feature rows beyond 4 * blockDim float4s: the loop after the four unconditional staging loads."""
    assert (fH + 3) // 4 * 4 * C // 4 > 1024 * ((D + 15) // 16)
    fx = L.lss_depth_fixture(D, fH, 2, yden=1024 if fH == 64 else 64)
    fused_exact(fx, C, what=f"tail D={D} fH={fH}")


def test_fused_head_row_stride_with_nan_padding():
    """CT > C + D with NaN in the padding words: nothing past C + D may be read."""
    fx = L.lss_depth_fixture(20, 5, 3, yden=64)
    fused_exact(fx, 48, pad=12, what="padded head")


@pytest.mark.parametrize("rows", [L.RUNS_MAIN_REENTERED, L.RUNS_BAB, L.RUNS_LEFTOVER_REENTERED, L.RUNS_ALL_DIFFERENT],
                         ids=["main_reentered", "bab", "leftover_reentered", "all_different"])
def test_fused_runs_along_an_image_column(rows):
    """The main cell is the first VALID point's cell and is re-entered after a leftover; leftover cells are re-entered; fH
    different cells.  The middle image column is entirely out of the grid: nothing is written for it and no cell is tagged
    (check_workspace compares the tagged set with the cells that hold a point, and every row with the reference)."""
    fx = L.lss_column_fixture(rows, xcells=(2.5, 9.5, 5.5))
    assert (fx["cell"][:, :, :, 1] == -1).all() and (fx["cell"][:, :, :, 0] >= 0).any()
    fused_exact(fx, 80, hot=2, what="runs")


def test_fused_truncation_rule_and_grid_faces_with_two_z_bins():
    """f = -0.5 is cell 0, f = -1 and f = n are out, on x, y and z; nz = 2 with points in both bins: channel z * C + c of the dense
    layout (k_lss_canvas)."""
    fused_exact(L.lss_face_fixture(), 16, hot=2, what="faces")


def test_fused_agents_and_cameras():
    """Three agents x two cameras, each translated to other cells, features different per camera: b = bn / n_cams."""
    fx = L.lss_column_fixture([1.5, 1.75, 6.5], D=4, n_agents=3, n_cams=2,
                              cam_cells=[(0, 0, 0), (1, -1, 0), (-2, 1, 0), (2, 0, 0), (0, -1, 0), (-1, 0, 0)])
    fused_exact(fx, 32, hot=2, what="agents")


def test_fused_collisions_add_up_exactly():
    """Every bin of every pixel of both cameras lands in one cell (768 points, 96 atomic adds per channel): a lost or doubled
    atomic is a wrong integer."""
    fx, D, fH, C = L.lss_bounded_cases()["collide"]
    _, ref = fused_exact(fx, C, what="collisions")
    assert int(ref["npts"].max()) == 768 and int(ref["adds"].max()) == 96


def test_fused_cell_edges_on_the_production_grid():
    """Ego coordinates within 2 ulp of cell edges of the dx = 0.4 grid: the output equals the reference built from the IEEE division
    (lss_cell_f32) bit for bit -- a * fl(1 / dx) without the near-integer guard puts `diverging` of these points elsewhere."""
    fx = L.lss_edge_fixture()
    n_div = 4 * int((fx["div_y"][:, None] | fx["div_x"][None, :]).sum())
    print(f"cell-edge fixture: {n_div} of {fx['cell'].size} points diverge under the reciprocal")
    note("lss_cell_edges", diverging_points=n_div, points=int(fx["cell"].size), div_x=int(fx["div_x"].sum()), div_y=int(fx["div_y"].sum()))
    assert int(fx["div_x"].sum()) >= 16 and int(fx["div_y"].sum()) >= 16
    fused_exact(fx, 16, hot=2, what="cell edges")


@pytest.mark.parametrize("C", [16, 32, 64])
def test_fused_channel_split_equals_the_default(C, monkeypatch):
    """HEAL_K4_CSPLIT=2 (grid.z channel slices): bit equal to the default at C = 32 and 64; falls back to one slice at C = 16."""
    fx = L.lss_depth_fixture(20, 17, 3, yden=64)
    one, _ = fused_exact(fx, C, what=f"csplit default C={C}")
    monkeypatch.setenv("HEAL_K4_CSPLIT", "2")
    two, _ = fused_exact(fx, C, what=f"csplit 2 C={C}")
    assert torch.equal(one, two)


# ========================================================================================================== sorted, exact
def sorted_exact(fx, C, hot=None, what=""):
    logit, feat, q = L.lss_exact_data(fx, C, hot=hot)
    ref = L.lss_forward_reference(fx, logit, feat)
    assert L.lss_exact_units(ref, q) < L.EXACT_LIMIT
    out = run_pool(fx, logit, feat)
    assert_equal(out, ref["out"], what)
    return out, ref


_RUN_CASES = [("tiles", C) for C in (16, 64, 80, 128, 144, 256)] + [("full", 64), ("tiny", 144), ("none", 16)]


@pytest.mark.parametrize("name,C", _RUN_CASES)
def test_sorted_run_lengths(name, C, monkeypatch):
    """Runs against the 32-point tiles (lss_run_cases: positions proven in tests/test_lss_refs_cpu.py), CPL = 1, 2, 4 with ragged
    lane rows."""
    monkeypatch.setenv("HEAL_LSS_PATH", "sorted")
    fx, _ = L.lss_run_cases()[name]
    D = fx["cell"].shape[1]
    out, _ = sorted_exact(fx, C, hot=min(4, 1 << (D.bit_length() - 1)), what=f"{name} C={C}")
    if name == "none":
        assert int(torch.count_nonzero(out)) == 0


def test_sorted_truncation_rule_agents_and_two_z_bins(monkeypatch):
    """k_lss_keys' own float comparison -1 < f < n before the conversion, on x, y and z; nz = 2; b = bn / n_cams."""
    monkeypatch.setenv("HEAL_LSS_PATH", "sorted")
    sorted_exact(L.lss_face_fixture(), 16, hot=2, what="sorted faces")
    sorted_exact(L.lss_fixture(1, 1, [(0, 0, 0)], fpos=L.B.k4_edge_positions()), 16, hot=2, what="sorted edges")
    sorted_exact(L.lss_fixture(1, 2, [(0, 0, 0), (1, 0, -1)], fpos=L.B.k4_centres(4, 2, 3, 5), nz=2), 80, hot=2, what="sorted two z")
    fx = L.lss_column_fixture([1.5, 1.75, 6.5], D=4, n_agents=3, n_cams=2,
                              cam_cells=[(0, 0, 0), (1, -1, 0), (-2, 1, 0), (2, 0, 0), (0, -1, 0), (-1, 0, 0)])
    sorted_exact(fx, 32, hot=2, what="sorted agents")


def test_routing_to_the_sorted_pipeline():
    """ops.bev_pool takes the sorted pipeline by itself for a non-separable frustum, D % 4 != 0 and fH > 64 -- shapes the fused
    entry point refuses -- and the result is exact there too."""
    cases = [("non-separable", L.lss_run_cases()["full"][0]),
             ("D=6", L.lss_depth_fixture(6, 5, 3, yden=64)),
             ("fH=65", L.lss_depth_fixture(4, 65, 2, yden=64))]
    for what, fx in cases:
        logit, feat, _ = L.lss_exact_data(fx, 16, hot=2)
        with pytest.raises(Exception):
            run_fused(fx, logit, feat)
        nx = [int(v) for v in fx["nx"]]
        key = (("bev_pool_pm", fx["n_agents"], 16, nx[0], nx[1], nx[2]), 0, torch.cuda.current_stream().cuda_stream)
        before = int(ops._WS[key].view(torch.int32)[1].item()) if key in ops._WS else None
        sorted_exact(fx, 16, hot=2, what=what)
        after = int(ops._WS[key].view(torch.int32)[1].item()) if key in ops._WS else None
        assert before == after, "the fused path's workspace was used"


def test_sorted_is_bit_reproducible(monkeypatch):
    """Two calls on random data give identical bits (fixed summation order), as the file header of bev_pool.hip claims."""
    monkeypatch.setenv("HEAL_LSS_PATH", "sorted")
    fx, D, fH, C = L.lss_bounded_cases()["d20_h17_c80"]
    logit, feat = L.lss_random_data(fx, C, 3)
    a = run_pool(fx, logit, feat)
    b = run_pool(fx, logit, feat)
    assert torch.equal(a, b) and int(torch.count_nonzero(a)) > 0


# ========================================================================================================== both, bounded
@pytest.mark.parametrize("name", sorted(L.lss_bounded_cases()))
def test_both_paths_within_their_bounds(name, monkeypatch):
    """Random logits in [-4, 4] and normal features on exact geometry: each path within k * 2^-24 * T of the float64 reference
    with its own k, element by element, and the two paths within the sum of their bounds of each other."""
    fx, D, fH, C = L.lss_bounded_cases()[name]
    logit, feat = L.lss_random_data(fx, C, 11)
    ref = L.lss_forward_reference(fx, logit, feat)
    bf, bs = L.lss_bounds(fx, ref, D, fH, C)
    fused = run_fused(fx, logit, feat)
    check_workspace(fx, C, ref, rows_exact=False)
    monkeypatch.setenv("HEAL_LSS_PATH", "sorted")
    srt = run_pool(fx, logit, feat)
    ok_f = within("lss_fused", fused, ref["out"], bf, case=name)
    ok_s = within("lss_sorted", srt, ref["out"], bs, case=name)
    ok_x = within("lss_fused_vs_sorted", fused, srt.cpu().double().numpy(), bf + bs, case=name)
    empty = torch.from_numpy(ref["T"] == 0)
    assert int(torch.count_nonzero(fused.cpu()[empty])) == 0 and int(torch.count_nonzero(srt.cpu()[empty])) == 0
    assert ok_f and ok_s and ok_x, name


# ===================================================================================================== workspace protocol
def stem_weights(C, seed):
    """Nonzero multiples of 1/4 in [-2, 2] and integer biases: with an integer map every product and partial sum is a multiple of
    1/4."""
    g = np.random.default_rng(seed)
    pick = np.concatenate([np.arange(-8, 0), np.arange(1, 9)]) / 4.0
    return (g.choice(pick, (64, C, 3, 3)), g.integers(-3, 4, 64).astype(np.float64), g.choice(pick, (64, C, 1, 1)),
            g.integers(-3, 4, 64).astype(np.float64))


def stem_reference(dense64, w1, b1, wd, bd):
    """The first BasicBlock's two convolutions in float64 on the CPU + the exactness budget (quarter units < 2^24)."""
    F = torch.nn.functional
    x = torch.from_numpy(np.ascontiguousarray(dense64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    main = torch.relu(F.conv2d(x, t(w1), t(b1), stride=2, padding=1))
    ident = F.conv2d(x, t(wd), t(bd), stride=2)
    budget = F.conv2d(x.abs(), t(np.abs(w1)), t(np.abs(b1)), stride=2, padding=1).max() * 4
    assert float(budget) < L.EXACT_LIMIT
    return main.numpy(), ident.numpy()


def run_stem(fx, C, seed, fmax=15):
    """Exact scatter (one hot bin: an integer map) -> heal_bev_stem_block, against float64 conv2d of the reference map."""
    logit, feat, q = L.lss_exact_data(fx, C, hot=1, fmax=fmax, seed=seed)
    ref = L.lss_forward_reference(fx, logit, feat)
    assert q == 1.0 and L.lss_exact_units(ref, q) < L.EXACT_LIMIT
    w1, b1, wd, bd = stem_weights(C, seed)
    want_main, want_id = stem_reference(ref["out"], w1, b1, wd, bd)
    pooled = run_fused(fx, logit, feat, pooled=True)
    assert isinstance(pooled, ops.PooledBEV) and pooled.stem_supported(64, 64)
    wm, wdf = ops.stem_fragments(dev(w1.astype(np.float32)), dev(wd.astype(np.float32)))
    got_main, got_id = pooled.stem_block(wm, dev(b1.astype(np.float32)), wdf, dev(bd.astype(np.float32)))
    assert_equal(got_main, want_main, "stem conv1")
    assert_equal(got_id, want_id, "stem downsample")
    return ref, (b1, bd), (got_main, got_id)


def test_workspace_protocol_over_different_scenes_and_consumers():
    """Calls on DIFFERENT exact fixtures that share one workspace: dense consumer, empty scene, stem_block consumer, dense.  Every
    output is bit equal to its reference; after call g the half (g & 1) ^ 1 is all zero, untagged rows of half g & 1 are zero, and
    the generation advances by one.  80 cells: no multiple of the 12 blocks of the dense emit nor of the 6 of the stem."""
    C, nx, ny = 96, 8, 5
    assert (2 * nx * ny) % (2 * C // 16) != 0 and (2 * nx * ny) % (2 * ((ny - 1) // 2 + 1)) != 0
    scenes = [("dense", L.lss_stem_fixture(nx, ny)), ("dense", L.lss_stem_fixture(nx, ny, "empty")),
              ("stem", L.lss_stem_fixture(nx, ny, "single")), ("dense", L.lss_stem_fixture(nx, ny))]
    gen0 = None
    for step, (consumer, fx) in enumerate(scenes):
        if consumer == "dense":
            logit, feat, q = L.lss_exact_data(fx, C, hot=2, seed=step)
            ref = L.lss_forward_reference(fx, logit, feat)
            out = run_fused(fx, logit, feat)
            assert_equal(out, ref["out"], f"protocol step {step}")
            if int(ref["npts"].sum()) == 0:
                assert int(torch.count_nonzero(out)) == 0
        else:
            ref, _, _ = run_stem(fx, C, step)
        gen = check_workspace(fx, C, ref)
        gen0 = gen - step if gen0 is None else gen0
        assert gen == gen0 + step, (gen, gen0, step)


# ============================================================================================================= k_bev_stem
@pytest.mark.parametrize("C", [32, 96, 64, 128])
@pytest.mark.parametrize("nx,ny", [(8, 8), (136, 6), (7, 4), (8, 5)])
def test_bev_stem_exact(C, nx, ny):
    """k_bev_stem<32> (C = 32, 96: one and three chunks) and <64> (C = 64, 128) on an integer map: both outputs equal float64
    conv2d bit for bit.  (136, 6): Wo = 68, the second x tile holds 4 pixels; (7, 4): odd nx, the right tap is off the map; (8, 5):
    odd ny, the bottom tap is off the map.  Two agents with different maps whose tagged cells sit in agent 0's last row and agent
    1's first row, and at x = nx - 1 in the row above an output pixel at x = 0 (lss_stem_fixture): nothing may leak through the
    clamped flag reads or flat cell indexing."""
    fx = L.lss_stem_fixture(nx, ny)
    cell = fx["cell"]
    assert (cell[0] // nx == ny - 1).any() and not (cell[0] // nx == 0).any()
    assert (cell[1] // nx == 0).any() and not (cell[1] // nx == ny - 1).any()
    assert (cell[0] == 1 * nx + nx - 1).any() and (cell[0] % nx == 0).any()
    ref, _, _ = run_stem(fx, C, C + nx)
    check_workspace(fx, C, ref)


@pytest.mark.parametrize("C", [32, 64])
def test_bev_stem_sparse_maps(C):
    """A single tagged cell (most taps skipped through the tap mask) and an empty map: relu(b1) and bd exactly."""
    ref, _, _ = run_stem(L.lss_stem_fixture(8, 8, "single"), C, 1)
    assert int((ref["npts"] > 0).sum()) == 1
    ref, (b1, bd), (got_main, got_id) = run_stem(L.lss_stem_fixture(8, 8, "empty"), C, 2)
    assert int(ref["npts"].sum()) == 0
    assert_equal(got_main, np.broadcast_to(np.maximum(b1, 0)[None, :, None, None], got_main.shape), "relu(b1)")
    assert_equal(got_id, np.broadcast_to(bd[None, :, None, None], got_id.shape), "bd")


# ==================================================================================================== heal_camera_matrices
def _signed_perms():
    perms = [(0, 1, 2), (1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0), (2, 0, 1)]
    signs = [(1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, 1)]
    out = []
    for p in perms:
        for s in signs:
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, p[r]] = s[r]
            out.append(m)
    return out


def _cam_call(rots, trans, intr, post, ptrans):
    t = lambda a: dev(np.asarray(a, np.float32))
    n = len(rots)
    return ops.camera_matrices(t(rots).view(1, n, 3, 3), t(trans).view(1, n, 3), t(intr).view(1, n, 3, 3), t(post).view(1, n, 3, 3),
                               t(ptrans).view(1, n, 3))


def test_camera_matrices_exact_on_permutations_and_power_of_two_scales():
    """Identity, axis permutations and 90-degree rotations (signed permutation matrices) as rotation and as post-rotation,
    power-of-two diagonal intrinsics and post-rotation scales: rots @ inv(intrins) and inv(post_rots) come out exactly."""
    S = _signed_perms()
    n = len(S)
    rots = np.stack(S)
    intr = np.stack([np.diag([2.0 ** (k % 5 - 2), 2.0 ** ((k + 1) % 4), 2.0 ** (-(k % 3))]) for k in range(n)])
    post = np.stack([S[(k * 7 + 3) % n] @ np.diag([2.0 ** (k % 3), 2.0 ** (-(k % 4)), 2.0 ** ((k + 2) % 5 - 2)]) for k in range(n)])
    post[0], rots[0], intr[0] = np.eye(3), np.eye(3), np.eye(3)
    inv_intr = np.stack([np.diag(1.0 / np.diag(m)) for m in intr])
    inv_post = np.stack([np.diag(1.0 / np.abs(m).sum(0)) @ np.sign(m).T for m in post])
    assert np.array_equal(np.einsum("nij,njk->nik", post, inv_post), np.broadcast_to(np.eye(3), (n, 3, 3)))
    trans = np.arange(3 * n).reshape(n, 3) * 0.25 - 4
    ptrans = -np.arange(3 * n).reshape(n, 3) * 0.5 + 7
    got = _cam_call(rots, trans, intr, post, ptrans)
    want = np.concatenate([(rots @ inv_intr).reshape(n, 9), inv_post.reshape(n, 9), ptrans, trans, np.zeros((n, 3))], 1)
    assert_equal(got, want, "camera matrices")


def test_camera_matrices_layout_with_distinct_values_per_slot():
    """The 27-float layout (combine 9 | inv post-rot 9 | post-trans 3 | trans 3 | 0 0 0) for 70 cameras (two blocks of 64 threads):
    integer matrices with determinant 1 (products of unit triangular matrices), so that the adjugate inverse is exact and every
    slot of every camera holds its own integer."""
    n = 70
    rots, intr, post, inv_intr, inv_post = [], [], [], [], []
    for t in range(n):
        a, b, c = 2 + t % 3, 6 + t % 5, 12 + t % 7
        U = np.array([[1.0, a, b], [0, 1, c], [0, 0, 1]])
        Lo = np.array([[1.0, 0, 0], [c, 1, 0], [a, b + 1, 1]])
        Ui = np.array([[1.0, -a, a * c - b], [0, 1, -c], [0, 0, 1]])
        Li = np.array([[1.0, 0, 0], [-c, 1, 0], [c * (b + 1) - a, -(b + 1), 1]])
        assert np.array_equal(U @ Ui, np.eye(3)) and np.array_equal(Lo @ Li, np.eye(3))
        # the rotation slot holds any matrix (it is not inverted): the first shift of a fixed one that leaves the 18 matrix slots distinct
        base = np.array([[11.0, 31, 5], [19, 2, 43], [9, 53, 3]])
        R = next(base + s for s in range(64) if len(set(np.concatenate([((base + s) @ Ui).ravel(), (Ui @ Li).ravel()]))) == 18)
        rots.append(R)
        intr.append(U); inv_intr.append(Ui)
        post.append(Lo @ U); inv_post.append(Ui @ Li)
    rots, intr, post, inv_intr, inv_post = (np.stack(v) for v in (rots, intr, post, inv_intr, inv_post))
    trans = 100.25 + np.arange(3 * n).reshape(n, 3)                # quarters: different from every integer matrix slot
    ptrans = -(500.75 + np.arange(3 * n).reshape(n, 3))
    want = np.concatenate([(rots @ inv_intr).reshape(n, 9), inv_post.reshape(n, 9), ptrans, trans, np.zeros((n, 3))], 1)
    assert float(np.abs(want).max()) < 2 ** 20 and all(len(set(row[:24])) == 24 for row in want)
    got = _cam_call(rots, trans, intr, post, ptrans)
    assert_equal(got, want, "camera matrix layout")
