"""The references and bounds of tests/linear_refs.py have teeth (no GPU): the addressing reference of heal_linear equals a naive
triple loop and changes under every planted index mistake; the fp32 emulation of k_colsum + k_split_weights in the kernels'
summation order stays within the derived per-element bound on every fixture of the GPU file's bound test, and every planted
arithmetic mistake leaves it."""
import numpy as np
import pytest

from tests import linear_refs as R
from tests.report import note


# ================================================================================================ heal_linear addressing
def _small(seed, T, K, N, groups=1, cs_parts=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (T, K)).astype(np.float64)
    w = rng.integers(-2, 3, (N, K)).astype(np.float64)
    b = rng.integers(1, 9, (groups, N)).astype(np.float64)
    cs = rng.choice([0.25, 0.5, 1.0, 2.0], (groups, cs_parts, N)) if cs_parts else None
    st = np.stack([rng.integers(-2, 3, T), rng.choice([0.5, 1.0, 2.0], T)], 1).astype(np.float64)
    return x, w, b, cs, st


def _naive(x, w, b, cs, cs_part, group_rows, stats, act, res, inner, outer, ldo, pc, ps, size):
    T, K = x.shape
    N = w.shape[0]
    flat = np.full(size, np.nan)
    for t in range(T):
        g = t // group_rows if group_rows else 0
        row = (t % inner) * outer + t // inner if inner else t
        for c in range(N):
            acc = 0.0
            for k in range(K):
                xv = x[t, k] if stats is None else (x[t, k] - stats[t, 0]) * stats[t, 1]
                acc += xv * w[c, k] * (cs[g, k // cs_part, c] if cs is not None else 1.0)
            acc += b[g, c]
            if act == "relu":
                acc = max(acc, 0.0)
            if res is not None:
                acc += res[row, c]
            flat[(c // pc) * ps + row * ldo + c % pc] = acc
    return flat


@pytest.mark.parametrize("inner,outer,pc,gap,ldo_pad,stats,act", [(0, 0, 8, 0, 0, False, None), (3, 4, 4, 0, 0, False, "relu"),
                                                                  (4, 3, 8, 12, 4, True, None), (6, 2, 4, 8, 0, False, "relu")])
def test_addressing_reference_equals_a_triple_loop(inner, outer, pc, gap, ldo_pad, stats, act):
    T, K, N, group_rows, cs_part = 12, 8, 8, 4, 4
    x, w, b, cs, st = _small(inner * 10 + pc, T, K, N, groups=3, cs_parts=K // cs_part)
    st = st if stats else None
    res = np.random.default_rng(1).integers(-50, 51, (T, N)).astype(np.float64)
    ldo = pc + ldo_pad
    ps = T * ldo + gap
    size = (N // pc) * ps
    rows = R.out_rows(T, inner, outer)
    val = R.linear_values(x, w, b, stats=st, colscale=cs, cs_part=cs_part, group_rows=group_rows, bias_per_group=True, act=act)
    flat, mask = R.scatter(val + res[rows], rows, ldo, pc, ps, size)
    want = _naive(x, w, b, cs, cs_part, group_rows, st, act, res, inner, outer, ldo, pc, ps, size)
    assert np.array_equal(mask, ~np.isnan(want)) and np.array_equal(flat[mask], want[mask])
    mag = R.linear_values(x, w, b, stats=st, colscale=cs, cs_part=cs_part, group_rows=group_rows, bias_per_group=True,
                          absolute=True)
    assert (mag >= np.abs(val)).all()


def test_planted_index_mistakes_change_the_reference():
    T, K, N, group_rows = 512, 32, 16, 256
    x, w, b, cs, _ = _small(3, T, K, N, groups=4, cs_parts=1)      # two groups; four tiles for the planted index
    kw = dict(colscale=cs, cs_part=K, group_rows=group_rows, bias_per_group=True)
    val = R.linear_values(x, w, b, **kw)
    R.assert_distinct(val)
    # the group of a token is the group of its tile's first token (t0 // group_rows), not the tile's own index
    assert not np.array_equal(R.linear_values(x, w, b, plant="group_by_tile", **kw), val)
    inner, outer, pc, ldo = 128, 4, 8, 8
    ps, size = T * ldo + 16, 4 * (T * ldo + 16)
    rows = R.out_rows(T, inner, outer)
    assert sorted(rows) == list(range(T))
    # ... and it is the group of the TOKEN, whatever row the map sends the token to
    assert not np.array_equal(R.linear_values(x, w, b, plant="group_by_out_row", plant_rows=rows, **kw), val)
    flat, mask = R.scatter(val, rows, ldo, pc, ps, size)
    swapped, _ = R.scatter(val, R.out_rows(T, inner, outer, plant="swap_map"), ldo, pc, ps, size)
    assert not np.array_equal(np.nan_to_num(swapped), np.nan_to_num(flat)), "inner and outer swapped"
    dense, dmask = R.scatter(val, rows, ldo, pc, ps, size, plant="dense_parts")
    assert not np.array_equal(dmask, mask), "part_stride taken as T * N"


def test_distinctness_check_sees_equal_rows_and_pieces():
    val = np.arange(64, dtype=np.float64).reshape(4, 16)
    R.assert_distinct(val)
    rows = val.copy()
    rows[2] = rows[0]
    with pytest.raises(AssertionError):
        R.assert_distinct(rows)
    pieces = val.copy()
    pieces[1, 8:12] = pieces[1, 0:4]
    with pytest.raises(AssertionError):
        R.assert_distinct(pieces)
    with pytest.raises(AssertionError):
        R.scatter(val, [0, 1, 1, 2], 16, 16, 0, 64)


# ================================================================================================ LayerNorm statistics, column sums
@pytest.mark.parametrize("C", [4, 32, 252, 256, 260, 508, 512])
def test_ln_stats_emulation_within_the_bound(C):
    rng = np.random.default_rng(C)
    x = (50.0 + 0.5 * rng.standard_normal((9, C))).astype(np.float32)
    mean, r, e_m, e_r = R.ln_stats_bounds(x, 1e-5)
    st = R.ln_stats_f32(x, 1e-5).astype(np.float64)
    assert (np.abs(st[:, 0] - mean) <= e_m).all() and (np.abs(st[:, 1] - r) <= e_r).all()


@pytest.mark.parametrize("C", [64, 128, 192, 256])
@pytest.mark.parametrize("rows", [1, 19, 20, 21, 511, 512, 513, 1030])
def test_colsum_emulation_is_exact_on_integers(C, rows):
    br = np.random.default_rng(C + rows).integers(-8, 9, (3, 2 * rows, C))
    want = R.colsum_exact(br, 2, rows)
    assert want.shape == (2, 3, R.n_chunks(rows), C)
    assert np.array_equal(R.colsum_f32(br, 2, rows).astype(np.int64), want)
    if rows > 512:
        assert not np.array_equal(R.colsum_f32(br, 2, rows, plant="drop_last_chunk").astype(np.int64), want)


# ================================================================================================ split-attention weights
PLANTS = ["part_rows", "drop_last_chunk", "swap_branches", "no_eps", "no_ln_b", "bias_unscaled"]


@pytest.fixture(scope="module")
def bound_runs():
    """Every fixture of the bound test once: (case, branches, params, reference)."""
    return [(case,) + R.bound_fixture(case) for case in R.BOUND_CASES]


def _ratios(case, br, p, ref, plant=None):
    C, groups, n_parts, rpp, eps = case
    scale, bias = R.emulate(br, groups, n_parts, rpp, p, eps, plant)
    return R.max_ratio(scale, ref["scale"], ref["B_scale"]), R.max_ratio(bias, ref["bias"], ref["B_bias"])


def test_emulation_of_the_kernels_stays_within_the_bound(bound_runs):
    worst = {}
    for case, br, p, ref in bound_runs:
        rs, rb = _ratios(case, br, p, ref)
        worst[case[0]] = max(worst.get(case[0], 0.0), rs, rb)
        assert rs <= 1.0 and rb <= 1.0, f"{case}: emulation at {rs:.3f} (scale) / {rb:.3f} (bias) x the bound"
        assert np.allclose(ref["scale"].sum(1), 1.0)
    note("linear_refs_cpu.split_weights_emulation", worst_ratio={str(k): v for k, v in worst.items()})


@pytest.mark.parametrize("plant", PLANTS)
def test_planted_mistake_leaves_the_bound(plant, bound_runs):
    hit = [case for case, br, p, ref in bound_runs if max(_ratios(case, br, p, ref, plant)) > 1.0]
    assert hit, f"{plant}: within the bound on every fixture"


def test_float64_reference_is_the_module_of_split_attn():
    """split_weights_reference against the reference's own sequence: to_out per token, sum, mean, fc1, LayerNorm, ReLU, fc2,
    softmax over the three branches (RadixSoftmax(3, 1))."""
    torch = pytest.importorskip("torch")
    C, groups, rows = 64, 2, 40
    br, p = R.split_branches(C, groups, rows, 1), R.split_params(C, 2)
    ref = R.split_weights_reference(br, groups, 1, rows, p, 1e-5)
    t = {k: torch.from_numpy(v).double() for k, v in p.items()}
    x = torch.from_numpy(br).double()
    outs = [x[i] @ t["w_out"][i].t() + t["b_out"][i] for i in range(3)]
    gap = sum(outs).reshape(groups, rows, C).mean(1)
    h = torch.nn.functional.layer_norm(gap @ t["fc1"].t(), (C,), t["ln_g"], t["ln_b"], 1e-5)
    a = torch.softmax((torch.relu(h) @ t["fc2"].t()).reshape(groups, 3, C), 1)
    assert np.allclose(ref["scale"], a.numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(ref["bias"], (a * t["b_out"][None]).sum(1).numpy(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_exact_fixtures_on_the_emulation(C):
    """The uniform and the one-hot gate of the GPU file, on the emulation: 1 / 3 everywhere, and exactly the winner."""
    groups, rows = 3, 37
    br = R.split_branches(C, groups, rows, C)
    p = R.split_params(C, C + 1, fc2_zero=True)
    scale, bias = R.emulate(br, groups, 1, rows, p, 1e-5)
    third = np.float32(1.0) / np.float32(3.0)
    assert (scale == third).all()
    b = p["b_out"]
    assert np.array_equal(bias, np.broadcast_to((third * b[0] + third * b[1]) + third * b[2], bias.shape))
    br, p, winner = R.onehot_fixture(C, groups, rows, C)
    lg = np.sort(R.split_weights_reference(br, groups, 1, rows, p, 1e-5)["logits"], 1)
    assert (lg[:, 2] - lg[:, 1] > 200.0).all(), "the winner's margin"
    assert len({tuple(w) for w in winner}) == groups and all(len(set(w)) == 3 for w in winner)
    scale, bias = R.emulate(br, groups, 1, rows, p, 1e-5)
    want = (np.arange(3)[None, :, None] == winner[:, None, :]).astype(np.float32)
    assert np.array_equal(scale, want)
    assert np.array_equal(bias, np.take_along_axis(p["b_out"], winner, 0))
    s2, b2 = R.emulate(br, groups, 1, rows, p, 1e-5, "bias_unscaled")
    assert np.array_equal(s2, want) and not np.array_equal(b2, bias)
