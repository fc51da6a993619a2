"""The float64 K5 forward reference of tests/k5_forward_refs.py against the oracle and against a float64 torch restatement of the
reference composition, the properties of the fixtures that tests/test_gpu_k5_forward_conformance.py relies on, an fp32 emulation
of k_warp_fuse held to the derived bound, and the sensitivity of that bound to the errors the suite is after.  No GPU: this must
pass before a kernel is compared with the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_np as O
from tests import k5_forward_refs as R

FIX = R.bounded_fixtures()
NAMES = sorted(FIX)
_REF = {}


def ref_of(name, grid_f64=True):
    """One reference per (fixture, grid dtype), shared by the tests and never modified."""
    if (name, grid_f64) not in _REF:
        _REF[name, grid_f64] = R.reference(FIX[name], grid_f64)
    return _REF[name, grid_f64]


def k_out(fx):
    return R.k5_forward_k(fx["feats"].shape[0])["out"]


# ----------------------------------------------------------------------------------------------------- reference agreement
@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_oracle(name):
    """oracle_np.weighted_fuse on oracle_np.occ_to_score: the same operator in fp32 numpy, with as many roundings per term as the
    kernel (sample 4, prob 56 + n, product 1, n - 1 adds), so it is held to the kernel's own bound.  The oracle's affine_grid
    handles one-row and one-column maps (its base grid is then the single coordinate 0, as torch's)."""
    fx = FIX[name]
    n, _, H, W = fx["feats"].shape
    ref = ref_of(name)
    mask = R.k5_keep(fx["crop"], n, H, W).reshape(n, 1, H, W).astype(np.float32)
    with np.errstate(over="ignore"):
        got = O.weighted_fuse(fx["feats"], O.occ_to_score(fx["occ"], mask), fx["rows"])
    ratio = R.max_ratio(got, ref["out"], R.bound(k_out(fx), ref["T"]))
    print(f"{name}: oracle err / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert (np.abs(ref["out"]) <= ref["T"] * (1 + 1e-12) + 1e-300).all()


def torch_forward(fx):
    """F.affine_grid + F.grid_sample (bilinear, zeros, align_corners=False) in float64, then the masked softmax of pyramid_fuse.py:
    score == 0 -> -inf, softmax over the agents, NaN -> 0 -> (out [C,H,W], S [n,H,W]).  Its taps are float64 taps."""
    x = torch.from_numpy(np.asarray(fx["feats"], np.float64))
    n, C, H, W = x.shape
    keep = torch.from_numpy(R.k5_keep(fx["crop"], n, H, W).reshape(n, 1, H, W))
    score = (torch.sigmoid(torch.from_numpy(np.asarray(fx["occ"], np.float64))) + R.OFFSET) * keep
    grid = F.affine_grid(torch.from_numpy(fx["rows"]), [n, C, H, W], align_corners=False)
    X = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    S = F.grid_sample(score, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    Sm = S.masked_fill(S == 0, -float("inf"))
    p = torch.softmax(Sm, dim=0)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    return (X * p).sum(0).numpy(), S[:, 0].numpy()


def coordinate_gap(fx):
    """Largest distance, in source pixels, between the fp32 sampling coordinate the kernel (and k5_taps) uses and the float64 one
    torch uses -> (dx, dy)."""
    n, _, H, W = fx["feats"].shape
    g64 = O.affine_grid(fx["rows"], H, W)
    g32 = g64.astype(np.float32)
    f = np.float32
    ix32 = ((g32[..., 0] + f(1)) * f(W) - f(1)) / f(2)
    iy32 = ((g32[..., 1] + f(1)) * f(H) - f(1)) / f(2)
    ix64, iy64 = ((g64[..., 0] + 1) * W - 1) / 2, ((g64[..., 1] + 1) * H - 1) / 2
    return float(np.abs(ix32 - ix64).max()), float(np.abs(iy32 - iy64).max())


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_float64_torch(name):
    """Masking is the one discontinuity of the operator: a sample that lies on the map's border to fp32 (weight exactly 0, agent
    masked) may lie 1e-16 inside it to float64 (agent unmasked).  Such pixels -- the two references disagree about WHO is masked
    -- are left out, and must be few.  Everywhere else bilinear sampling with zero padding is continuous in the coordinate: on
    fixtures whose grid is exact the two agree to float64 rounding, elsewhere within the tap-weight difference, which is at most
    (dx + dy) per tap pair: |dX| <= 2 (dx + dy) max|x|, |dS| <= 2 (dx + dy) 1.0001, |dprob| <= |dS| summed over the agents."""
    fx = FIX[name]
    n = fx["feats"].shape[0]
    ref = ref_of(name)
    out, S = torch_forward(fx)
    same = ((S != 0) == (ref["S"] != 0)).all(0)
    assert same.mean() >= 0.8 and same.sum() > 0
    dx, dy = coordinate_gap(fx)
    xmax = float(np.abs(fx["feats"]).max())
    tol = 1e-12 * max(xmax, 1.0) if fx["grid_exact"] else 2.0 * (dx + dy) * xmax * (1 + 2.0002 * n)
    if fx["grid_exact"]:
        assert dx + dy < 1e-12
    err = float(np.abs(out - ref["out"])[:, same].max())
    print(f"{name}: torch float64 err = {err:.3e} (tolerance {tol:.3e}, {int((~same).sum())} pixels of disputed masking)")
    assert err <= tol
    assert tol < 2e-3          # the tap-weight difference is small: the comparison means something


# ----------------------------------------------------------------------------------------------------- conditions on the fixtures
def test_unmasked_agent_counts():
    """Pixels with 0, 1, 2, ... unmasked agents exist, and `counts` has every count from 0 to n."""
    cnt = ref_of("counts")["count"]
    n = FIX["counts"]["feats"].shape[0]
    assert set(np.unique(cnt)) == set(range(n + 1))
    for name in ("far8", "rotations", "window", "saturated"):
        c = ref_of(name)["count"]
        assert len(np.unique(c)) >= 3, name
    assert int((ref_of("rotations")["count"] == 0).sum()) > 0
    for name in NAMES:
        ref = ref_of(name)
        assert np.array_equal(ref["prob"].sum(0) > 0.5, ref["count"] > 0) and (ref["out"][:, ref["count"] == 0] == 0).all()
        assert R.tiny_weights(FIX[name]) > 2.0 ** -60, name


def test_translation_fixtures_have_off_map_and_zero_weight_taps():
    fx = FIX["far8"]
    H, W = fx["feats"].shape[2:]
    off, tw, ok = R.k5_taps(fx["rows"], H, W)
    assert (ok & (tw == 0)).any()                       # a tap inside the map that carries weight 0 (whole-pixel shifts)
    x0 = np.arange(H * W) % W
    y0 = np.arange(H * W) // W
    bad = ~ok
    assert bad[:, x0 == 0].any() and bad[:, x0 == W - 1].any() and bad[:, y0 == 0].any() and bad[:, y0 == H - 1].any()
    rot = ref_of("rotations")
    assert (rot["count"] < 4).all() and not (rot["S"][1] != 0).any()             # agent 1 wholly off the map
    assert (rot["S"][2] != 0).any() and (rot["S"][2] == 0).any()                 # agent 2 partly
    win = ref_of("window")
    assert not (win["S"][3] != 0).any() and (win["S"][1] != 0).any()             # the empty window masks its agent everywhere


@pytest.mark.parametrize("name", ["translation", "collision"])
def test_exact_fixtures_are_exact(name):
    fx = R.exact_fixture(name)
    ref = R.reference(fx)
    assert set(np.unique(ref["prob"])) <= {0.0, 1.0}
    assert float(ref["T"].max()) / fx["unit"] < R.EXACT_LIMIT
    assert np.array_equal(ref["out"] / fx["unit"], np.round(ref["out"] / fx["unit"])) and float(np.abs(ref["out"]).max()) > 0
    assert np.array_equal(R.emulate_f32(fx["feats"], fx["occ"], fx["rows"], fx["crop"]).astype(np.float64), ref["out"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_equal_agents(n):
    fx = R.equal_agents(n)
    ref = R.reference(fx)
    assert np.allclose(ref["prob"], 1.0 / n, rtol=1e-15) and float(np.abs(fx["want"]).max()) * n < R.EXACT_LIMIT
    assert R.max_ratio(ref["out"], fx["want"], 1e-15 * np.abs(fx["want"])) <= 1
    emu = R.emulate_f32(fx["feats"], fx["occ"], fx["rows"])
    if n & (n - 1) == 0:
        assert np.array_equal(emu, fx["want"])
    else:
        assert R.max_ratio(emu, fx["want"], R.bound(n + 2, np.abs(fx["want"]))) <= 1


def test_one_agent_is_the_sample():
    """n = 1: prob is exactly 1 where the agent is unmasked, and the tap chain is that of sample_f32: bit for bit."""
    fx = FIX["far1"]
    want = np.where(ref_of("far1")["count"][None] > 0, R.sample_f32(fx["feats"], fx["rows"])[0], np.float32(0))
    assert np.array_equal(R.emulate_f32(fx["feats"], fx["occ"], fx["rows"]), want)


def test_lds_layouts():
    n, C, H, W = R.SLICED
    (lv,) = R.lds_layout([(C, H, W)])
    assert lv["cpb"] >= 16 and lv["last"] % 8 != 0 and lv["cgroups"] > 1
    assert R.fused_layout(C, H, W) == (8, 9) and C % 8 == 6                          # heal_warp_fuse: cch > 4, C % cch != 0
    (lv,) = R.lds_layout([R.BIG[1:]])
    assert lv["cpb"] >= 16 and lv["last"] % 8 != 0
    (lv,) = R.lds_layout([R.ROUNDS[1:]])
    assert lv["cpb"] >= 16 and lv["last"] > 8 and lv["last"] % 8 != 0                # two rounds in one slice, the second a tail
    lvs = R.lds_layout(R.FOUR_LEVELS)
    assert any(C < 8 for C, _, _ in R.FOUR_LEVELS) and len(lvs) == 4
    for a, b, la, lb in zip(R.FOUR_LEVELS, R.FOUR_LEVELS[1:], lvs, lvs[1:]):
        assert a[1:] != b[1:] and a[0] != b[0] and lb["block0"] == la["block0"] + la["blocks"] > la["block0"]
    (lv,) = R.lds_layout([FIX["zoom"]["feats"].shape[1:]])
    assert lv["cpb"] == 8 and lv["last"] == 3


def test_lds_boxes_of_the_zoom_fixture():
    """Zoom 2: a tile's box is 32 x 32 exactly (staged); zoom 2.25: 33 or more (fallback); even and odd widths occur."""
    fx = FIX["zoom"]
    H, W = fx["feats"].shape[2:]
    boxes = R.lds_boxes(fx["rows"], ref_of("zoom")["prob"], H, W)
    assert boxes.shape == (16, 4, 4)
    z2, z225 = boxes[:, 2], boxes[:, 3]
    assert any(b[2] == 32 and b[3] == 32 and R.staged(b) for b in z2)
    assert any(b[2] >= 33 and not R.staged(b) for b in z225) and any(R.staged(b) for b in z225)
    widths = {int(b[2]) for a in range(4) for b in boxes[:, a] if R.staged(b)}
    assert any(w % 2 == 0 for w in widths) and any(w % 2 == 1 for w in widths)
    assert (boxes[:, :, 2] <= W).all() and (boxes[:, :, 0] >= 0).all() and (boxes[:, :, 0] + boxes[:, :, 2] <= W).all()
    assert any(b[2] == 0 for b in z2)                                                # tiles that do not see the zoomed agent
    assert (boxes[:, 0, 2] >= 16).all()                                              # the identity: 16 or 17 wide


# ----------------------------------------------------------------------------------------------------- emulation
@pytest.mark.parametrize("grid_f64", [True, False])
def test_fp32_emulation_stays_within_the_bound(grid_f64):
    worst = 0.0
    for name in NAMES:
        fx = FIX[name]
        ref = ref_of(name, grid_f64)
        emu = R.emulate_f32(fx["feats"], fx["occ"], fx["rows"], fx["crop"], grid_f64)
        ratio = R.max_ratio(emu, ref["out"], R.bound(k_out(fx), ref["T"]))
        print(f"{name} grid_f64={grid_f64}: emulation err / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert (emu[:, ref["count"] == 0] == 0).all() and not np.signbit(emu[:, ref["count"] == 0]).any()
    print(f"largest emulation err / bound = {worst:.4f}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------- sensitivity
def _mutant_taps(fx, kind):
    n, _, H, W = fx["feats"].shape
    off, tw, ok = R.k5_taps(fx["rows"], H, W)
    if kind == "swap":           # the ne and sw taps swapped: each weight goes to the other's source pixel
        tw = tw[..., [0, 2, 1, 3]]
    else:                        # `<= W - 1` read as `< W - 1`: the last column and the last row are never sampled
        edge = (off % W == W - 1) | (off // W == H - 1)
        tw = np.where(ok & edge, 0.0, tw)
    return off, tw, ok


def _ratio(name, **kw):
    fx, ref = FIX[name], ref_of(name)
    crop = kw.pop("crop", fx["crop"])
    wrong = R.k5_forward(fx["feats"], fx["occ"], fx["rows"], crop, **kw)["out"]
    return R.max_ratio(wrong, ref["out"], R.bound(k_out(fx), ref["T"])), wrong


def test_bound_separates_the_errors_the_suite_is_after():
    sat = FIX["saturated"]
    got = {}
    got["offset dropped"], dropped = _ratio("saturated", offset=0.0)
    got["offset doubled"], doubled = _ratio("saturated", offset=2 * R.OFFSET)
    got["zero mask removed"], _ = _ratio("saturated", mask_zero=False)
    h0, h1, w0, w1 = sat["crop"][1]
    got["crop h1 off by one"], _ = _ratio("saturated", crop=[None, (h0, h1 - 1, w0, w1)] + sat["crop"][2:])
    got["ne and sw swapped"], _ = _ratio("rotations", taps=_mutant_taps(FIX["rotations"], "swap"))
    got["border < W - 1"], _ = _ratio("far8", taps=_mutant_taps(FIX["far8"], "border"))
    got["border < W - 1, rotations"], _ = _ratio("rotations", taps=_mutant_taps(FIX["rotations"], "border"))
    for k, v in got.items():
        print(f"mutant `{k}`: err / bound = {v:.3g}")
    assert all(v >= 4.0 for v in got.values()), got
    # the gap this suite closes: both offset mutants pass the tolerance the fused kernel was held to so far
    want = ref_of("saturated")["out"]
    assert np.allclose(dropped, want, rtol=1e-3, atol=2e-5) and np.allclose(doubled, want, rtol=1e-3, atol=2e-5)


def test_split_reference_is_the_fused_reference():
    """k_fuse_warped's reference on float64 warped maps and scores is the fused reference: the split form computes the same thing."""
    for name in ("far5", "window"):
        ref = ref_of(name)
        out, T, prob = R.split_reference(ref["X"], ref["S"][:, None])
        assert np.allclose(out, ref["out"], rtol=1e-13, atol=1e-15) and np.array_equal(prob[:, 0], ref["prob"])
        assert (T <= ref["T"] * (1 + 1e-12)).all()           # |sample of x| <= sample of |x|
