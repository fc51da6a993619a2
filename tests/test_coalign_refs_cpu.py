"""The references of tests/coalign_refs.py against the reference's float64 torch composition (reference_level of
tests/test_gpu_coalign.py), sample_f32 against the float64 sample, the layout rule, the properties of the exact fixtures, and the
TEETH of the per-element bound and of the bit-exact `max` comparison: seeded defects of the kind k_warp_att_fuse can have,
applied to the fp32-rounded reference, must show on the fixtures tests/test_gpu_coalign_conformance.py uses.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import coalign_refs as R
from tests.backward_refs import k5_taps
from tests.test_gpu_coalign import reference_level

RTOL = 1e-12


def close(a, b, tol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(np.abs(b), 1.0)).all())


# ---------------------------------------------------------------------------------------------------------------- (a)
def test_layout_rule_and_block_ranges():
    assert R.coalign_layout(256, 256) == (64, 4) and R.coalign_layout(252, 256) == (16, 16)
    assert R.coalign_layout(*R.PIX64[1:]) == (64, 4) and R.coalign_layout(64, 64) == (16, 16) and R.coalign_layout(1, 1) == (16, 16)
    assert [R.coalign_layout(H, W)[0] for _, H, W in R.MIXED] == [16, 64, 16, 16]
    assert [R.coalign_layout(H, W)[0] for _, H, W in R.THRESHOLD] == [16, 64]
    assert all(R.coalign_layout(H, W)[0] == 16 for _, H, W in R.SMALL)
    assert R.coalign_blocks(R.MIXED) == [(0, 2 * 13, 16), (26, 17 * 64, 64), (26 + 1088, 5, 16), (26 + 1088 + 5, 1, 16)]
    k = R.coalign_k(5, 17, 16)
    assert k["s"] == 8 + 1 + 2 + 15 + 1 and k["p"] == 13 and k["out"] == 22
    assert R.coalign_k(8, 5, 4)["s"] == 8 + 1 + 2 + 3 + 1


@pytest.mark.parametrize("mode", ["att", "max"])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_references_equal_the_float64_composition_on_exact_poses(n, mode):
    """Half-pixel translations on a power-of-two map: torch's float64 grid_sample and the kernel's fp32 tap arithmetic form the
    same coordinates and weights, so the float64 composition is the reference to 1e-12 on random float features (C = 16: sqrt(C) is
    the same number in fp32, which the kernel divides by, and in float64)."""
    C, H, W = 16, 8, 16
    feats = R.random_feats(n, C, H, W, seed=n)
    rows = R.half_rows(n, H, W)
    want = reference_level(torch.from_numpy(feats), rows, mode, torch.float64).numpy()
    if mode == "att":
        ref = R.att_reference(feats, rows)
        assert close(ref["out"], want)
        assert (np.abs(ref["out"]) <= ref["T"] * (1 + 1e-12) + 1e-300).all() and np.isfinite(ref["B"]).all()
        assert close(ref["p"].sum(0), 1.0)
    else:
        got = R.max_reference(feats, rows).astype(np.float64)
        x, xa = R.sample_f64(feats, rows)
        assert (np.abs(got - want) <= 4 * R.EPS * xa.max(0) * (1 + 1e-6)).all()
        assert np.array_equal(x.max(0), want) or close(x.max(0), want)


@pytest.mark.parametrize("grid_f64", [True, False])
def test_sample_f32_is_within_its_roundings_of_the_float64_sample(grid_f64):
    """tap4 is 4 products and 3 adds, 7 roundings, of which a tap's term passes at most 4: |f32 - f64| <= 4 EPS |x| per element, on
    rotations with taps off every border; and the float64 sample is torch's grid_sample up to the fp32 rounding of the pixel coordinate."""
    n, C, H, W = 6, 5, 19, 27
    feats = R.random_feats(n, C, H, W, seed=3)
    rows = R.poses("ego", n, 3)
    x, xa = R.sample_f64(feats, rows, grid_f64)
    s = R.sample_f32(feats, rows, grid_f64)
    assert s.dtype == np.float32 and (np.abs(s.astype(np.float64) - x) <= R.coalign_k(n, C, 16)["x"] * R.EPS * xa * (1 + 1e-6)).all()
    _, tw, ok = k5_taps(rows, H, W, grid_f64)
    assert not ok.all() and ok.any() and not R.reached(rows, H, W, grid_f64)[0].all()       # the ego's own sample leaves the map
    if grid_f64:
        M = torch.from_numpy(rows)
        grid = torch.nn.functional.affine_grid(M, [n, C, H, W], align_corners=False).float().double()
        t = torch.nn.functional.grid_sample(torch.from_numpy(feats).double(), grid, align_corners=False).numpy()
        assert float(np.abs(t - x).max()) <= 16 * R.EPS * max(H, W) * float(np.abs(feats).max())


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("n,C,H,W", R.EQUAL_CASES)
def test_equal_agents_fixture(n, C, H, W):
    fx = R.equal_agents(n, C, H, W, seed=n)
    assert fx["units"] < R.EXACT_LIMIT and np.array_equal(fx["feats"], np.round(fx["feats"]))
    assert np.array_equal(R.sample_f32(fx["feats"], fx["rows"]), fx["feats"])                 # the identity samples the pixel itself
    ref = R.att_reference(fx["feats"], fx["rows"], fx["sqrt_dim"])
    assert np.array_equal(ref["out"], fx["want"].astype(np.float64))
    assert np.array_equal(ref["p"], np.full_like(ref["p"], 1.0 / n))
    assert np.array_equal(R.max_reference(fx["feats"], fx["rows"]), fx["want"])


@pytest.mark.parametrize("n,C,H,W", R.SELECTOR_CASES)
def test_selector_fixture(n, C, H, W):
    fx = R.selector(n, C, H, W, seed=n)
    assert fx["units"] < R.EXACT_LIMIT and np.array_equal(fx["feats"], np.round(fx["feats"]))
    nz, zero, gap = R.selector_masks(fx)
    assert nz.sum() >= H * W // 4 and zero.sum() >= H                      # both kinds of pixel
    assert gap > R.UNDERFLOW_GAP
    assert float(np.exp(np.float32(-R.UNDERFLOW_GAP))) < 2.0 ** -149 / 2
    x, _ = R.sample_f64(fx["feats"], fx["rows"])
    assert np.array_equal(x * 16, np.round(x * 16))                        # samples on the quarter grid (sixteenths would do)
    assert np.array_equal(R.sample_f32(fx["feats"], fx["rows"]).astype(np.float64), x)
    ref = R.att_reference(fx["feats"], fx["rows"], fx["sqrt_dim"])
    assert float(np.abs(ref["out"] - x[fx["chosen"]])[:, nz].max()) < 1e-30 * R.SELECTOR_SCALE
    assert close(ref["out"][:, zero], x.mean(0)[:, zero]) and not x[fx["chosen"]][:, zero].any()
    assert np.abs(ref["logit"][:, zero]).max() == 0


# ---------------------------------------------------------------------------------------------------------------- (c)
def att_plain(x, sd, logit=None, mask=None):
    """The `att` reduction on samples x [n, C, H, W] in float64; logit overrides the logits, mask [n, H, W] False drops an agent."""
    lg = (x[:1] * x).sum(1) / sd if logit is None else logit
    if mask is not None:
        lg = np.where(mask, lg, -np.inf)
    e = np.exp(lg - lg.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    return (p[:, None] * x).sum(0)


def swapped_taps_sample(feats, rows):
    """sample_f64 with the north-east and south-west taps read from each other's address (weights kept)."""
    n, C, H, W = feats.shape
    off, tw, _ = k5_taps(rows, H, W)
    off = off[..., [0, 2, 1, 3]]
    v = R._gather(np.asarray(feats, np.float64).reshape(n, C, H * W), off)
    return (v * tw[:, None]).sum(-1).reshape(n, C, H, W)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


TEETH = [(3, R.MIXED, "rot", 0), (8, R.MIXED, "rot", 3), (5, R.SMALL, "ego", 1), (4, R.SMALL, "offmap", 2), (2, R.THRESHOLD, "rot", 2)]


@functools.lru_cache(maxsize=None)
def teeth_case(i):
    n, levels, pose, seed = TEETH[i]
    return R.bound_fixture(n, levels, pose, seed)


@pytest.mark.parametrize("i", range(len(TEETH)))
def test_att_bound_and_max_equality_have_teeth(i):
    n, levels, pose, _ = TEETH[i]
    fx = teeth_case(i)
    rows = fx["rows"]
    seen = set()
    for l, (C, H, W) in enumerate(levels):
        feats, sd = fx["feats"][l], fx["sqrt_dims"][l]
        ref = R.att_reference(feats, rows, sd)
        ratio = lambda got: R.max_ratio(f32(got), ref["out"], ref["B"])      # noqa: E731
        assert ratio(ref["out"]) <= 1.0                                  # rounding the reference to fp32 stays inside
        x, _ = R.sample_f64(feats, rows)
        assert ratio(att_plain(x, sd)) <= 1.0
        assert ratio(att_plain(R.sample_f32(feats, rows).astype(np.float64), sd)) <= 1.0      # the fp32 samples: c_x covers them
        pix, n_slices = ref["layout"]
        cper = -(-C // n_slices)
        last = min(cper, C) - 1                                            # the last channel of slice 0
        mut = {}
        if n > 1:
            mut["dot_misses_the_last_channel_of_a_slice"] = att_plain(x, sd, logit=((x[:1] * x).sum(1) - x[0, last] * x[:, last]) / sd)
            mut["logits_divided_by_sqrt_C"] = att_plain(x, R.f32_sqrt_dim(C))
            rc = R.reached(rows, H, W)
            if not rc.all():
                mut["out_of_reach_agent_dropped_from_the_softmax"] = att_plain(x, sd, mask=rc)
        if H > 1 and W > 1:
            mut["ne_and_sw_taps_swapped"] = att_plain(swapped_taps_sample(feats, rows), sd)
        hole = ref["out"].copy()
        hole[last] = 0.0
        mut["last_output_channel_of_a_slice_not_written"] = hole
        for name, got in mut.items():
            r = ratio(got)
            print(i, (C, H, W), name, round(r, 2))
            assert r > 1.0, (name, (C, H, W), r)
            seen.add(name)
        # max mode: bit equality is the check
        want = R.max_reference(feats, rows)
        s32 = R.sample_f32(feats, rows)
        rc = R.reached(rows, H, W)
        if not rc.all():
            skipped = np.where(rc[:, None], s32, -np.inf).max(0)
            skipped = np.where(np.isfinite(skipped), skipped, 0.0).astype(np.float32)
            if not np.array_equal(skipped, want):        # shows where every agent in reach is negative: on some level of each case
                seen.add("max_skips_out_of_reach")
        if H > 1 and W > 1 and n > 1:
            assert not np.array_equal(f32(swapped_taps_sample(feats, rows)).max(0), want)
    need = {"last_output_channel_of_a_slice_not_written", "ne_and_sw_taps_swapped"}
    if n > 1:
        need |= {"dot_misses_the_last_channel_of_a_slice", "logits_divided_by_sqrt_C"}
    if pose in ("offmap", "rot", "ego") and n > 1:
        need |= {"out_of_reach_agent_dropped_from_the_softmax", "max_skips_out_of_reach"}
    assert need <= seen, need - seen
