"""The float64 numpy references of tests/backward_refs.py against float64 torch autograd of the reference compositions, and the
properties of the fixtures that tests/test_gpu_backward_conformance.py relies on.  No GPU: this must pass before a kernel is
compared with any of these references."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests import backward_refs as R

pytestmark = pytest.mark.grad         # float64 torch autograd is the witness here: the tests record graphs (on the CPU)

RTOL = 1e-12


def close(a, b):
    """1e-12 relative per element (the data are of order one: an element whose reference is 0 is held to 1e-12 absolute)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= RTOL * np.maximum(np.abs(b), 1.0)).all())


# ---------------------------------------------------------------------------------------------------------------- K5
def k5_autograd(feats, occ, rows, gout, crop):
    from heal_amd.opencood.models.fuse_modules.pyramid_fuse import weighted_fuse_autograd
    n = feats.shape[0]
    x = torch.from_numpy(np.asarray(feats, np.float64)).requires_grad_(True)
    o = torch.from_numpy(np.asarray(occ, np.float64)).requires_grad_(True)
    aff = np.zeros((1, n, n, 2, 3))
    aff[0, 0] = rows
    out = weighted_fuse_autograd(x, o, [n], aff, crop)
    (out * torch.from_numpy(np.asarray(gout, np.float64))[None]).sum().backward()
    return x.grad.numpy(), o.grad.numpy()


K5_CASES = {
    "far8": lambda: (*R.k5_ints(1, 8, 5, 16, 8), R.shift_rows(R.FAR, 16, 8), None),
    "far3": lambda: (*R.k5_ints(2, 3, 5, 16, 8), R.shift_rows(R.FAR[:3], 16, 8), None),
    "crop": lambda: (*R.k5_ints(3, 3, 3, 8, 16), R.shift_rows([(0.0, 0.0), (0.5, 0.5), (-0.5, 1.0)], 8, 16),
                     [(2, 3, 5, 6), (0, 6, 0, 12), (3, 8, 6, 16)]),
    "1x1": lambda: (*R.k5_ints(4, 3, 3, 1, 1), R.shift_rows([(0.0, 0.0)] * 3, 1, 1), None),
    "exact": lambda: (lambda f: (f["feats"], f["occ"], f["grad_out"], f["rows"], f["crop"]))(R.k5_exact_translation()),
    "collision": lambda: (lambda f: (f["feats"], f["occ"], f["grad_out"], f["rows"], f["crop"]))(R.k5_collision()),
}


@pytest.mark.parametrize("name", sorted(K5_CASES))
def test_k5_reference_equals_float64_autograd(name):
    """Against weighted_fuse_autograd in float64.  Its score offset is the double 1e-4, the kernel's (and the reference's default)
    the float32 constant 1e-4f, 4.7e-9 away in relative terms: the reference is given the double here so that 1e-12 can be asked."""
    feats, occ, gout, rows, crop = K5_CASES[name]()
    ref = R.k5_reference(feats, occ, rows, gout, crop, offset=1e-4)
    gx, go = k5_autograd(feats, occ, rows, gout, crop)
    assert close(ref["g_feats"], gx), float(np.abs(ref["g_feats"] - gx).max())
    assert close(ref["g_occ"], go), float(np.abs(ref["g_occ"] - go).max())
    assert (np.abs(ref["g_feats"]) <= ref["T_feats"] * (1 + 1e-12) + 1e-300).all()
    assert (np.abs(ref["g_occ"]) <= ref["T1_occ"] * (1 + 1e-12) + 1e-300).all()
    if name in ("far3", "far8", "crop"):
        # a real softmax: the occupancy gradient is exercised
        assert float(np.abs(go).max()) > 0 and bool(((ref["prob"] > 0) & (ref["prob"] < 1)).any())


def test_k5_fp32_grid_is_torchs_fp32_affine_grid():
    """grid_f32 restates grid_point<float>; torch builds the same numbers (linspace * (n - 1) / n, then base @ theta^T) in fp32 for
    pure translations on the maps used, so the fp32-grid GPU case has a second witness."""
    import torch.nn.functional as F
    for H, W, shifts in ((16, 8, R.FAR[:3]), (4, 4, R.FAR[:3])):
        rows = R.shift_rows(shifts, H, W)
        want = F.affine_grid(torch.from_numpy(rows).float(), [len(shifts), 1, H, W], align_corners=False).numpy()
        got = R.grid_f32(rows, H, W)
        assert float(np.abs(got - want).max()) <= 2.0 ** -22


def test_k5_translations_give_exact_tap_weights():
    for H, W in ((16, 8), (8, 32), (16, 64), (4, 4), (2, 32), (1, 1), (8, 16)):
        _, tw, _ = R.k5_taps(R.shift_rows(R.FAR, H, W), H, W)
        assert set(np.unique(tw)) <= {0.0, 0.25, 0.5, 1.0}
    _, tw, _ = R.k5_taps(R.k5_collision()["rows"], 16, 16)
    assert np.array_equal(tw * 64, np.round(tw * 64))


@pytest.mark.parametrize("make", [R.k5_exact_translation, R.k5_collision])
def test_k5_exact_fixtures_have_one_unmasked_agent_per_pixel(make):
    fx = make()
    cnt = R.k5_unmasked_count(fx)
    assert set(np.unique(cnt)) <= {0, 1} and int((cnt == 1).sum()) > 0
    ref = R.k5_reference(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    assert set(np.unique(ref["prob"])) <= {0.0, 1.0}
    assert np.array_equal(ref["prob"].sum(0), (cnt == 1).astype(np.float64))
    assert R.k5_exact_units(ref, fx["unit"]) < R.EXACT_LIMIT
    assert np.array_equal(ref["g_feats"] / fx["unit"], np.round(ref["g_feats"] / fx["unit"]))
    assert float(np.abs(ref["g_occ"]).max()) == 0.0
    if make is R.k5_exact_translation:
        assert int((cnt == 0).sum()) > 0                                 # pixels where every agent is masked
    else:
        assert float(ref["n_feats"].max()) >= 16                         # about sixteen ego pixels per source pixel


def test_k5_bound_separates_the_errors_the_suite_is_after():
    """The per-element bound is tight enough to see a crop window that is off by one, a dropped border tap and a lost term of a
    shared source pixel: each of these wrong results, computed by the reference itself, exceeds the bound somewhere."""
    feats, occ, gout, rows, crop = K5_CASES["crop"]()
    n, C = feats.shape[:2]
    ref = R.k5_reference(feats, occ, rows, gout, crop)
    bf, bo = R.k5_bounds(ref, n, C)
    assert R.max_ratio(ref["g_feats"], ref["g_feats"], bf) == 0.0
    off_by_one = R.k5_reference(feats, occ, rows, gout, [crop[0], (0, 6, 0, 11), crop[2]])
    assert R.max_ratio(off_by_one["g_occ"], ref["g_occ"], bo) > 1 and R.max_ratio(off_by_one["g_feats"], ref["g_feats"], bf) > 1
    feats, occ, gout, rows, crop = K5_CASES["far8"]()
    ref = R.k5_reference(feats, occ, rows, gout, crop)
    bf, bo = R.k5_bounds(ref, 8, 5)
    # one term lost at the element with the SMALLEST non-zero sum of terms: the quietest place such an error can hide
    t = np.where(ref["T_feats"] > 0, ref["T_feats"], np.inf)
    i = np.unravel_index(np.argmin(t), t.shape)
    wrong = ref["g_feats"].copy()
    wrong[i] -= ref["T_feats"][i] / max(ref["n_feats"][i], 1.0)
    assert R.max_ratio(wrong, ref["g_feats"], bf) > 1


# ---------------------------------------------------------------------------------------------------------------- K4
def k4_cases():
    """name -> (fixture, D, C, exact).  The same builders the GPU tests use, at their smallest members."""
    out = {}
    out["exact_d4"] = (R.k4_fixture(R.k4_centres(4, 2, 3, 1), [(0, 0, 0)], 1, 1), 4, 5, True)
    out["exact_d64"] = (R.k4_fixture(R.k4_centres(64, 2, 3, 2), [(0, 0, 0)], 1, 1), 64, 5, True)
    out["c256"] = (R.k4_fixture(R.k4_centres(4, 2, 3, 3), [(0, 0, 0)], 1, 1), 4, 256, True)
    out["agents"] = (R.k4_fixture(R.k4_centres(4, 2, 3, 4, 2, 6), [(0, 0, 0), (1, -2, 0), (-2, 1, 0), (2, 2, 0), (0, -1, 0), (-1, 0, 0)],
                                  3, 2), 4, 5, True)
    out["two_z"] = (R.k4_fixture(R.k4_centres(4, 2, 3, 5), [(0, 0, 0), (1, 0, -1)], 1, 2, nz=2), 4, 3, True)
    out["edges"] = (R.k4_fixture(R.k4_edge_positions(), [(0, 0, 0)], 1, 1), 4, 5, True)
    out["random_d3"] = (R.k4_fixture(R.k4_centres(3, 2, 3, 6), [(0, 0, 0)], 1, 1), 3, 5, False)
    out["random_d63"] = (R.k4_fixture(R.k4_centres(63, 2, 3, 7), [(0, 0, 0)], 1, 1), 63, 5, False)
    return out


def test_k4_edge_fixture_lands_where_the_issue_says():
    fx = R.k4_fixture(R.k4_edge_positions(), [(0, 0, 0)], 1, 1)
    cell = fx["cell"][0]
    assert (cell[:, 0, 0] == -1).all()
    assert cell[0, 0, 1] % 8 == 0 and cell[0, 0, 1] >= 0 and cell[1, 0, 1] == -1 and cell[2, 0, 1] == -1 and cell[3, 0, 1] % 8 == 3
    assert (cell[0, 1, 2] // 8) % 8 == 0 and cell[1, 1, 2] == -1 and cell[2, 1, 2] == -1
    # the four points that sit on an integer (f = -1 and f = n, on x and on y) are exactly the ones named; all others are at k + 0.5
    frac = fx["f"] - np.floor(fx["f"])
    on_int = (frac == 0.0)
    assert int(on_int.sum()) == 4
    assert on_int[0, 1, 0, 1, 0] and on_int[0, 2, 0, 1, 0] and on_int[0, 1, 1, 2, 1] and on_int[0, 2, 1, 2, 1]
    assert (frac[~on_int] == 0.5).all()


@pytest.mark.parametrize("name", sorted(k4_cases()))
def test_k4_fixture_points_sit_at_half_cells_and_values_are_exact(name):
    fx, D, C, exact = k4_cases()[name]
    if name != "edges":
        frac = fx["f"] - np.floor(fx["f"])
        assert (frac == 0.5).all()
    if exact:
        assert D & (D - 1) == 0 and R.k4_exact_units(D, C, 2) < R.EXACT_LIMIT
        logit, feat, gout = R.k4_data(fx, D, C, 0, True)
        ref = R.k4_reference(fx, logit, feat, gout)
        assert (ref["p"] == 1.0 / D).all()
        for v in (ref["g_feat"], ref["g_logit"]):
            assert np.array_equal(v * D * D, np.round(v * D * D))


@pytest.mark.parametrize("name", sorted(k4_cases()))
def test_k4_reference_equals_float64_index_add_autograd(name):
    fx, D, C, exact = k4_cases()[name]
    logit, feat, gout = R.k4_data(fx, D, C, 3, exact)
    ref = R.k4_reference(fx, logit, feat, gout)
    lg = torch.from_numpy(logit.astype(np.float64)).requires_grad_(True)
    ft = torch.from_numpy(feat.astype(np.float64)).requires_grad_(True)
    nx = [int(v) for v in fx["nx"]]
    cells = nx[0] * nx[1] * nx[2]
    BN, n_agents, n_cams = logit.shape[0], fx["n_agents"], fx["n_cams"]
    vals = (lg.softmax(1)[:, :, None] * ft[:, None]).permute(0, 1, 3, 4, 2).reshape(-1, C)       # [BN*D*fH*fW, C]
    cell = torch.from_numpy(fx["cell"])
    row = (torch.arange(BN)[:, None, None, None] // n_cams) * cells + cell
    ok = (cell >= 0).reshape(-1)
    pooled = torch.zeros((n_agents * cells, C), dtype=torch.float64).index_add(0, row.reshape(-1)[ok], vals[ok])
    # [agent, iz, iy, ix, C] -> [agent, nz*C, ny, nx] with channel z * C + c
    out = pooled.view(n_agents, nx[2], nx[1], nx[0], C).permute(0, 1, 4, 2, 3).reshape(n_agents, nx[2] * C, nx[1], nx[0])
    (out * torch.from_numpy(gout.astype(np.float64))).sum().backward()
    assert close(ref["g_feat"], ft.grad.numpy()) and close(ref["g_logit"], lg.grad.numpy())
    assert (np.abs(ref["g_feat"]) <= ref["T_feat"] + 1e-300).all()
    assert (np.abs(ref["g_logit"]) <= ref["T_logit"] * (1 + 1e-12) + 1e-300).all()
    # the forward oracle puts z bin iz of channel c at output channel iz * C + c: the same pooled map from oracle_np.bev_pool
    geom = fx["frustum"][None] + fx["trans"][:, None, None, None, :]      # fr.z = 1: (x z, y z, z) + trans, exact in fp32
    x6 = vals.detach().numpy().reshape(n_agents, n_cams, D, *feat.shape[2:], C)
    want = O.bev_pool(geom.reshape(n_agents, n_cams, D, *feat.shape[2:], 3), x6, fx["dx"], fx["bx"], fx["nx"])
    assert float(np.abs(want - out.detach().numpy()).max()) <= 1e-5 * max(float(np.abs(want).max()), 1.0)
    if name == "two_z":
        per_bin = np.abs(want).reshape(n_agents, 2, C, -1).sum((0, 2, 3))
        assert per_bin[0] > 0 and per_bin[1] > 0                          # points in both z bins


# ---------------------------------------------------------------------------------------------------------------- K2
K2_M = (1, 3, 4, 5, 16, 17, 67)
K2_P = (1, 16, 17, 31, 32)


def k2_autograd(vox, coords, nps, prm, grad):
    """PillarVFE.pillar_features in float64, eval mode: A = dW / (gamma rstd), B = d beta, Cx = d gamma."""
    from heal_amd.opencood.models.sub_modules.pillar_vfe import PillarVFE
    vfe = PillarVFE({"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]}, 4,
                    list(R.K2_VOXEL), list(R.K2_RANGE)).double().eval()
    pfn = vfe.pfn_layers[0]
    t = lambda k: torch.from_numpy(np.asarray(prm[k], np.float64))      # noqa: E731
    scale, rstd, mean, shift = t("scale"), t("rstd"), t("mean"), t("shift")
    gamma = scale / rstd
    with torch.no_grad():
        pfn.linear.weight.copy_(t("weight"))
        pfn.norm.weight.copy_(gamma)
        pfn.norm.bias.copy_(shift + mean * scale)
        pfn.norm.running_mean.copy_(mean)
        pfn.norm.running_var.copy_(1.0 / (rstd * rstd) - pfn.norm.eps)
    out = vfe.pillar_features(torch.from_numpy(vox.astype(np.float64)), torch.from_numpy(coords).long(),
                              torch.from_numpy(nps).long())
    (out * torch.from_numpy(np.asarray(grad, np.float64))).sum().backward()
    return (out.detach().numpy(), (pfn.linear.weight.grad / scale[:, None]).numpy(), pfn.norm.bias.grad.numpy(),
            pfn.norm.weight.grad.numpy())


def k2_close(a, b, scale):
    return bool((np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), scale)).all())


@pytest.mark.parametrize("M,P", [(1, 1), (3, 16), (5, 17), (17, 31), (67, 32), (16, 1), (4, 32)])
def test_k2_reference_equals_float64_autograd_and_fixture_is_exact(M, P):
    vox, coords, nps = R.k2_pillars(M, P, seed=100 * M + P)
    prm = R.k2_params(7 * M + P)
    f, fabs = R.k2_features64(vox, coords, nps)
    assert np.array_equal(f, O.pillar_features(vox, coords, nps, R.K2_VOXEL, R.K2_RANGE).astype(np.float64))
    assert np.array_equal(f * 4, np.round(f * 4)) and R.k2_exact_units(f, prm) < R.EXACT_LIMIT
    grad = np.random.default_rng(M + P).integers(-2, 3, (M, 64)).astype(np.float64)
    out, A, B, Cx = k2_autograd(vox, coords, nps, prm, grad)
    ref = R.k2_backward(f, nps, prm, grad, tie="torch", fabs=fabs)
    assert k2_close(R.k2_forward(f, nps, prm)[0], out, 1.0)
    s = max(float(np.abs(A).max()), 1.0)
    assert k2_close(ref["A"], A, s) and k2_close(ref["B"], B, s) and k2_close(ref["Cx"], Cx, s)
    assert (np.abs(ref["A"]) <= ref["T_A"] + 1e-300).all() and (np.abs(ref["Cx"]) <= ref["T_Cx"] + 1e-300).all()


def test_k2_tie_rules_differ_only_in_A_and_only_on_real_versus_padding_ties():
    """The finding recorded in k2_backward's docstring, measured on an integer fixture where such ties do occur: a real row with
    y == relu(shift) > 0 and np < P.  The kernel's rule gives that gradient to the padding row (A gets nothing), torch's to the real
    row; B and Cx are the same under both rules."""
    vox, coords, nps = R.k2_pillars(67, 17, seed=3)
    prm = R.k2_params(5)
    f, _ = R.k2_features64(vox, coords, nps)
    grad = np.random.default_rng(2).integers(-2, 3, (67, 64)).astype(np.float64)
    a, b = R.k2_backward(f, nps, prm, grad, tie="kernel"), R.k2_backward(f, nps, prm, grad, tie="torch")
    out, z, y, pad = R.k2_forward(f, nps, prm)
    differ = (a["pad_wins"] != b["pad_wins"]) & (out > 0)      # (at y* = 0 the rules pick different rows too, but dy = 0 there)
    assert int(differ.sum()) > 0 and not np.array_equal(a["A"], b["A"])
    assert np.array_equal(a["B"], b["B"]) and np.array_equal(a["Cx"], b["Cx"])
    m, c = np.nonzero(differ)
    assert (z[m, b["p_star"][m, c], c] == 0).all() and (pad[c] > 0).all()


def test_k2_random_fixture_has_no_near_ties():
    vox, coords, nps, prm = R.k2_random()
    f, fabs = R.k2_features64(vox, coords, nps)
    assert R.k2_argmax_margin(f, fabs, nps, prm) > 0
    grad = np.random.default_rng(1).standard_normal((vox.shape[0], 64))
    out, A, B, Cx = k2_autograd(vox, coords, nps, prm, grad)
    ref = R.k2_backward(f, nps, prm, grad, tie="kernel", fabs=fabs)      # no ties: both rules agree
    s = max(float(np.abs(A).max()), 1.0)
    assert k2_close(ref["A"], A, s) and k2_close(ref["B"], B, s) and k2_close(ref["Cx"], Cx, s)
    assert k2_close(R.k2_forward(f, nps, prm)[0], out, 1.0)
