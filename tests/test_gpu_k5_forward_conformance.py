"""The K5 forward kernels of heal_amd/csrc/warp_fuse.hip, element by element at their edges: k_warp_fuse<1..8> (heal_warp_fuse),
k_warp_fuse_lds<1..8> (heal_warp_fuse_levels, heal_warp_fuse_levels_src), k_warp_agent<16> (heal_warp_agent), k_fuse_warped
(heal_fuse_warped, heal_fuse_warped_rows) and k_warp_agents_pm (heal_warp_agents_pm).

Every assertion is one of: torch.equal with a reference that fp32 computes without rounding (the float64 reference on an exact
fixture, or sample_f32 where the kernel only samples); an exact +0.0 where every agent is masked; or the per-element bound
|got - ref| <= k * 2^-24 * T with k derived in tests/k5_forward_refs.py (k5_forward_k) from the kernel's operation sequence.
Nothing is normalised by a tensor-wide maximum and no element may be wrong.  The reference, the fixtures' properties and the
staging path each fixture takes are proven on the CPU in tests/test_k5_forward_refs_cpu.py.  The launch layouts restated there
assume the library's default block target: with HEAL_K5_BLOCKS set this module skips."""
import os

import numpy as np
import pytest
import torch

from heal_amd import ops
from tests import k5_forward_refs as R
from tests.report import note

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_REF = {}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _default_layout_and_summary():
    if os.environ.get("HEAL_K5_BLOCKS"):
        pytest.skip("HEAL_K5_BLOCKS is set: the fixtures prove their staging paths for the library's default block target only")
    yield
    for entry, ratio in sorted(_WORST.items()):
        print(f"k5 forward, largest err / bound of {entry}: {ratio:.4f}")
        note("k5_forward:largest", entry=entry, ratio=ratio)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ref_of(key, fx, grid_f64=True):
    """One float64 reference per (fixture, grid dtype), shared by the tests that need it and never modified."""
    if (key, grid_f64) not in _REF:
        _REF[key, grid_f64] = R.reference(fx, grid_f64)
    return _REF[key, grid_f64]


def equal(got, ref64):
    """Bit for bit: the float64 reference is representable in fp32 on an exact fixture (checked), and equals the kernel's output."""
    ref64 = torch.from_numpy(np.asarray(ref64, np.float64))
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64)
    return torch.equal(got.detach().cpu().float(), ref32)


def within(entry, got, ref, bound, **tags):
    """The per-element bound; the largest err / bound goes on record before the assertion."""
    ratio = R.max_ratio(got.detach().cpu().double().numpy(), ref, bound)
    print(f"{entry} {tags}: largest err / bound = {ratio:.4f}")
    note("k5_forward:" + entry, ratio=ratio, **tags)
    _WORST[entry] = max(_WORST.get(entry, 0.0), ratio)
    return ratio <= 1.0


def plus_zero_where_all_masked(got, count):
    z = got.detach().cpu()[:, torch.from_numpy(count == 0)]
    return bool((z == 0).all()) and not bool(torch.signbit(z).any())


def crop_arg(crop):
    return None if crop is None else [c if c is not None else (0, 0, 0, 0) for c in crop]       # (0,0,0,0): keep everything


def rows_arg(rows, dev_rows):
    return torch.from_numpy(np.asarray(rows, np.float64)).to(DEV) if dev_rows else rows


def run_fused(fx, grid_f64=True, dev_rows=False):
    return ops.warp_fuse(dev(fx["feats"]), dev(fx["occ"]), rows_arg(fx["rows"], dev_rows), grid_f64, crop_arg(fx["crop"]))


def run_levels(fxs, grid_f64=True, dev_rows=False):
    crops = [fx["crop"] for fx in fxs]
    return ops.warp_fuse_levels([dev(fx["feats"]) for fx in fxs], [dev(fx["occ"]) for fx in fxs], rows_arg(fxs[0]["rows"], dev_rows),
                                grid_f64, crops if any(c is not None for c in crops) else None)


def both_kernels_bounded(key, fx, grid_f64=True, dev_rows=False, **tags):
    """heal_warp_fuse and heal_warp_fuse_levels on one fixture, each against the float64 reference -> (fused, levels, reference)."""
    n = fx["feats"].shape[0]
    ref = ref_of(key, fx, grid_f64)
    b = R.bound(R.k5_forward_k(n)["out"], ref["T"])
    fused = run_fused(fx, grid_f64, dev_rows)
    (levels,) = run_levels([fx], grid_f64, dev_rows)
    ok_f = within("heal_warp_fuse", fused, ref["out"], b, fixture=key, grid_f64=grid_f64, dev_rows=dev_rows, **tags)
    ok_l = within("heal_warp_fuse_levels", levels, ref["out"], b, fixture=key, grid_f64=grid_f64, dev_rows=dev_rows, **tags)
    assert ok_f and ok_l, (key, tags)
    assert plus_zero_where_all_masked(fused, ref["count"]) and plus_zero_where_all_masked(levels, ref["count"])
    return fused, levels, ref


# ======================================================================================================= fused: both kernels
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_instantiation_within_the_bound(n):
    """k_warp_fuse<n> (4 channels in flight for n <= 4, 2 for n <= 6, else 1; C = 5 leaves a tail in each) and k_warp_fuse_lds<n>
    on a 16 x 8 map under half- and whole-pixel shifts with taps off the map on every side; both grid dtypes, affine rows from the
    host and from the device.  One agent: prob is exactly 1 and the output is the sample, bit for bit."""
    fx = R.far(n)
    for grid_f64 in (True, False):
        for dev_rows in (False, True):
            fused, levels, ref = both_kernels_bounded(f"far{n}", fx, grid_f64, dev_rows, n=n)
            if n == 1:
                want = np.where(ref["count"][None] > 0, R.sample_f32(fx["feats"], fx["rows"], grid_f64)[0], np.float32(0))
                assert torch.equal(fused.cpu(), torch.from_numpy(want)) and torch.equal(levels.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("C", R.CHANNEL_TAILS)
def test_channel_tails(C):
    """The `c + u < C` tail of every unroll width (n = 3: four channels in flight, n = 6: two, n = 8: one) and the `nc < 8` tail of a
    staging round."""
    for n in (3, 6, 8):
        both_kernels_bounded(f"tail_n{n}_c{C}", R.far(n, C=C, seed=300 + 10 * n + C), n=n, C=C)


@pytest.mark.parametrize("which", ["SLICED", "BIG", "ROUNDS"])
def test_channel_slices(which):
    """SLICED: heal_warp_fuse runs channel slices of 8 with a last slice of 6 (blockIdx.z > 0), the levels launch slices of 16 with
    a last slice of 6.  BIG: 256 x 256, slices of 16 and 4.  ROUNDS: a last slice of 12 = a full staging round and a tail of 4."""
    shape = getattr(R, which)
    both_kernels_bounded(which, R.sliced(shape, seed=170 + shape[1]), shape=list(shape))


@pytest.mark.parametrize("name", ["counts", "rotations", "window", "saturated", "zoom", "shape_1xW", "shape_Hx1", "shape_5x7",
                                  "shape_1x1"])
@pytest.mark.parametrize("grid_f64", [True, False])
def test_bounded_fixtures(name, grid_f64):
    """Every count of unmasked agents from 0 to 8; rotations with an agent wholly and one partly off the map; a camera crop window,
    a window on the border and the empty window; saturated logits; zooms whose source boxes are 32 wide (staged, an even
    width), 36 wide (direct gather) and of odd widths; maps of one row, one column, less than a tile, one pixel."""
    both_kernels_bounded(name, R.bounded_fixtures()[name], grid_f64)


@pytest.mark.parametrize("name", ["translation", "collision"])
def test_exact_fixtures(name):
    """Probabilities 0 or 1 and dyadic tap weights on integer features: both kernels equal the float64 reference bit for bit, and
    the pixels no agent reaches hold +0.0."""
    fx = R.exact_fixture(name)
    ref = ref_of("exact_" + name, fx)
    assert float(ref["T"].max()) / fx["unit"] < R.EXACT_LIMIT
    fused, (levels,) = run_fused(fx), run_levels([fx])
    assert equal(fused, ref["out"]) and equal(levels, ref["out"])
    assert plus_zero_where_all_masked(fused, ref["count"]) and plus_zero_where_all_masked(levels, ref["count"])
    if name == "translation":
        assert int((ref["count"] == 0).sum()) > 0
        assert equal(run_fused(fx, dev_rows=True), ref["out"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_equal_agents(n):
    """n identical maps and logits under the identity: prob = fl(1 / n).  A power of two: the output is the map, bit for bit;
    otherwise wt, the product and n - 1 adds round: within (n + 2) EPS of the map."""
    fx = R.equal_agents(n)
    fused, (levels,) = run_fused(fx), run_levels([fx])
    if n & (n - 1) == 0:
        assert equal(fused, fx["want"]) and equal(levels, fx["want"])
    else:
        b = R.bound(n + 2, np.abs(fx["want"]))
        assert within("heal_warp_fuse:equal_agents", fused, fx["want"], b, fixture="equal_agents", n=n)
        assert within("heal_warp_fuse_levels:equal_agents", levels, fx["want"], b, fixture="equal_agents", n=n)
    assert torch.equal(fused, levels)


# ======================================================================================================= levels
@pytest.mark.parametrize("grid_f64", [True, False])
def test_four_levels_in_one_launch(grid_f64):
    """Four levels of different shapes and channel counts (one with C < 8, one of a single pixel) in one grid: a block that took the
    wrong level by its block0 range would read another level's shape."""
    fxs = R.four_levels()
    outs = run_levels(fxs, grid_f64, dev_rows=grid_f64)
    n = fxs[0]["feats"].shape[0]
    for i, (fx, got) in enumerate(zip(fxs, outs)):
        ref = ref_of(f"four_levels_{i}", fx, grid_f64)
        assert within("heal_warp_fuse_levels", got, ref["out"], R.bound(R.k5_forward_k(n)["out"], ref["T"]), fixture="four_levels",
                      level=i, grid_f64=grid_f64)
        assert plus_zero_where_all_masked(got, ref["count"])
        assert torch.equal(got, run_fused(fx, grid_f64))


def window_sources(form):
    """The window fixture as heal_warp_fuse_levels_src reads it -> (sources of one level, the zero-padded stack as a fixture).
    The source stack is non-zero outside the boxes: a kernel that read there would differ from the reference on the padded stack."""
    fx = R.window()
    n, C, H, W = fx["feats"].shape
    f, o = dev(fx["feats"]), dev(fx["occ"])
    padded = dict(fx, feats=np.zeros_like(fx["feats"]), occ=np.zeros_like(fx["occ"]))
    level = []
    for a, box in enumerate(R.WINDOW_BOXES):
        y0, y1, x0, x1 = box or (0, H, 0, W)
        padded["feats"][a, :, y0:y1, x0:x1] = fx["feats"][a, :, y0:y1, x0:x1]
        padded["occ"][a, :, y0:y1, x0:x1] = fx["occ"][a, :, y0:y1, x0:x1]
        fa, oa = f[a, :, y0:y1, x0:x1], o[a, 0, y0:y1, x0:x1]
        if form == "dense":
            fa, oa = fa.contiguous(), oa.contiguous()
        level.append((fa, oa, (y0, x0)))
    return level, padded, (H, W)


@pytest.mark.parametrize("form", ["dense", "slice"])
def test_levels_src_against_the_reference_on_the_padded_stack(form):
    level, padded, shape = window_sources(form)
    ref = ref_of("window_padded", padded)
    (got,) = ops.warp_fuse_levels_src([level], [shape], padded["rows"], True, [padded["crop"]])
    assert within("heal_warp_fuse_levels_src", got, ref["out"], R.bound(R.k5_forward_k(4)["out"], ref["T"]), form=form)
    assert plus_zero_where_all_masked(got, ref["count"]) and float(np.abs(ref["out"]).max()) > 0
    assert torch.equal(got, run_levels([padded])[0])
    for grid_f64 in (True, False):      # the rows as a CUDA tensor, read at run time: the bits of the rows passed by value
        host = got if grid_f64 else ops.warp_fuse_levels_src([level], [shape], padded["rows"], False, [padded["crop"]])[0]
        devr = ops.warp_fuse_levels_src([level], [shape], rows_arg(padded["rows"], True), grid_f64, [padded["crop"]])[0]
        assert torch.equal(devr, host), grid_f64


# ======================================================================================================= split form
@pytest.mark.parametrize("C", [1, 15, 16, 17, 33])
def test_warp_agent(C):
    """feat_ego is the sample, bit for bit (16 channels per block: one short, exact, one over, two blocks and one over); score_ego
    is within k_score of the warped score and exactly 0 where the reference is 0 -- off the map, outside the crop window -- and
    nowhere else."""
    H, W = 24, 40
    base = R.rotations()
    feats, occ = R.data(400 + C, 1, C, H, W)
    k = R.k5_forward_k(1)["score"]
    for a, crop, grid_f64 in ((2, None, True), (3, (5, 20, 9, 30), True), (3, (0, 1, 0, 0), True), (2, None, False)):
        row = base["rows"][a:a + 1]
        fe, se = ops.warp_agent(dev(feats[0]), dev(occ[0]), row, grid_f64, None if crop is None else [crop])
        assert torch.equal(fe.cpu(), torch.from_numpy(R.sample_f32(feats, row, grid_f64)[0]))
        S = R.k5_forward(feats, occ, row, [crop], grid_f64)["S"]
        assert within("heal_warp_agent:score_ego", se, S, R.bound(k, S), C=C, agent=a, crop=crop is not None, grid_f64=grid_f64)
        assert torch.equal(se.cpu() == 0, torch.from_numpy(S == 0)) and not bool(torch.signbit(se).any())
        if crop != (0, 1, 0, 0):
            assert (S == 0).any() and (S != 0).any()


def split_inputs(n, C, H=24, W=44, seed=500):
    """fp32 warped maps and scores in [0, 1] with exact zeros: about a third of the (agent, pixel) scores, and whole columns."""
    g = np.random.default_rng(seed + 10 * n + C)
    x = g.standard_normal((n, C, H, W)).astype(np.float32)
    s = g.uniform(1e-4, 1.0, (n, 1, H, W)).astype(np.float32)
    s[g.uniform(size=s.shape) < 0.3] = 0
    s[:, :, :2, :] = 0
    s[:, :, -1, -5:] = 0
    return x, s


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fuse_warped(n):
    """k_fuse_warped on 264 float4 columns (two blocks, the second ragged), one channel, one and two channel blocks; all-zero score
    columns give +0.0; heal_fuse_warped_rows on shuffled, non-contiguous offsets into one buffer equals the stacked call bit for bit."""
    for C in (1, 16, 17):
        x, s = split_inputs(n, C)
        H, W = x.shape[2:]
        want, T, prob = R.split_reference(x, s)
        got = ops.fuse_warped(dev(x), dev(s))
        assert within("heal_fuse_warped", got, want, R.bound(R.k5_forward_k(n)["split"], T), n=n, C=C)
        count = (s[:, 0] != 0).sum(0)
        assert int((count == 0).sum()) >= 2 * W and plus_zero_where_all_masked(got, count)
        # rows: the agents' maps and scores at shuffled places of one buffer, gaps of 4 and 8 floats between them
        g = np.random.default_rng(n)
        order = g.permutation(2 * n)
        sizes = [C * H * W if j < n else H * W for j in order]
        starts = np.concatenate([[4], 4 + np.cumsum([sz + 4 * (1 + j % 2) for j, sz in enumerate(sizes)])])[:-1]
        base = np.full(int(starts[-1] + sizes[-1] + 4), 7.0, np.float32)
        at = {}
        for j, st, sz in zip(order, starts, sizes):
            base[st:st + sz] = (x[j] if j < n else s[j - n]).reshape(-1)
            at[int(j)] = int(st)
        rows = ops.fuse_warped_rows(dev(base), [at[a] for a in range(n)], [at[n + a] for a in range(n)], C, H, W)
        assert torch.equal(rows, got)


def test_warp_agents_pm_ragged():
    """One 64-channel block that is mostly empty (C = 4) and two blocks with a 4-channel second one (C = 68), on a 5 x 7 map (less than
    a 16 x 4 tile on one axis, two ragged tiles on the other): the sample of every agent, token-major, bit for bit."""
    fx = R.shape("5x7")
    for C in (4, 68):
        feats, _ = R.data(600 + C, 4, C, 5, 7)
        for grid_f64 in (True, False):
            got = ops.warp_agents_pm(dev(feats), fx["rows"], grid_f64)
            want = R.sample_f32(feats, fx["rows"], grid_f64).transpose(0, 2, 3, 1)
            assert got.shape == want.shape and torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))
            assert torch.equal(ops.warp_agents_pm(dev(feats), rows_arg(fx["rows"], True), grid_f64), got)     # rows read on the device


# ======================================================================================================= repeatability
def test_two_launches_are_bit_equal():
    """No atomics in the forward: every entry point gives the same bits twice."""
    fx = R.rotations()
    level, padded, shape = window_sources("slice")
    x, s = split_inputs(4, 17)
    feats, occ = dev(fx["feats"]), dev(fx["occ"])
    calls = {
        "warp_fuse": lambda: run_fused(fx),
        "warp_fuse_levels": lambda: run_levels([fx])[0],
        "warp_fuse_levels_src": lambda: ops.warp_fuse_levels_src([level], [shape], padded["rows"], True, [padded["crop"]])[0],
        "warp_agent": lambda: torch.cat([t.reshape(-1) for t in ops.warp_agent(feats[2], occ[2], fx["rows"][2:3], True, None)]),
        "fuse_warped": lambda: ops.fuse_warped(dev(x), dev(s)),
        "warp_agents_pm": lambda: ops.warp_agents_pm(dev(np.ascontiguousarray(fx["feats"][:, :4])), fx["rows"], True),
    }
    for name, call in calls.items():
        a, b = call().clone(), call()
        torch.cuda.synchronize()
        assert torch.equal(a, b), name
