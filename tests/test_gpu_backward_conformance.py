"""The three scatter / gather BACKWARD kernels of the training path, element by element at their edges:
heal_warp_fuse_backward (K5), heal_bev_pool_backward (K4), heal_pfn_moments / heal_pfn_features / heal_pfn_backward (K2).

Every assertion is one of: torch.equal with the float64 reference on a fixture that fp32 computes without rounding; an exact
zero; or the per-element bound |got - ref| <= k * 2^-24 * T with k derived in tests/backward_refs.py (k5_k, k4_k, k2_k) from the
kernel's operation sequence.  Nothing is normalised by a tensor-wide maximum and no element may be wrong.  The references and the
fixture properties relied on here are proven on the CPU in tests/test_backward_refs_cpu.py.  The operators are called directly:
no autograd graph is recorded."""
import numpy as np
import pytest
import torch

from heal_amd import ops
from tests import backward_refs as R
from tests.report import note

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def equal(got, ref64):
    """Bit-for-bit: the float64 reference is representable in fp32 on an exact fixture (checked), and equals the kernel's output."""
    ref32 = torch.from_numpy(np.asarray(ref64, np.float64)).float()
    assert torch.equal(ref32.double(), torch.from_numpy(np.asarray(ref64, np.float64)))
    return torch.equal(got.detach().cpu().float(), ref32)


def within(name, got, ref, bound, **tags):
    """The per-element bound; the largest err / bound goes on record before the assertion."""
    ratio = R.max_ratio(got.detach().cpu().double().numpy(), ref, bound)
    print(f"{name} {tags}: largest err / bound = {ratio:.4f}")
    note(name, ratio=ratio, **tags)
    return ratio <= 1.0


# =================================================================================================================== K5
def run_k5(feats, occ, rows, gout, crop=None, grid_f64=True, dev_rows=False):
    crop_arg = None if crop is None else [c if c is not None else (0, 0, 0, 0) for c in crop]       # (0,0,0,0): keep everything
    rows_arg = torch.from_numpy(np.asarray(rows, np.float64)).to(DEV) if dev_rows else rows
    return ops.warp_fuse_backward(dev(feats), dev(occ), rows_arg, dev(gout), grid_f64, crop_arg)


def k5_bounded(name, feats, occ, rows, gout, crop=None, grid_f64=True, dev_rows=False, **tags):
    n, C = feats.shape[:2]
    gf, go = run_k5(feats, occ, rows, gout, crop, grid_f64, dev_rows)
    ref = R.k5_reference(feats, occ, rows, gout, crop, grid_f64)
    bf, bo = R.k5_bounds(ref, n, C)
    ok_f = within(name + ":grad_feats", gf, ref["g_feats"], bf, **tags)
    ok_o = within(name + ":grad_occ", go, ref["g_occ"], bo, **tags)
    assert ok_f and ok_o, (name, tags)
    return gf, go, ref


def test_k5_exact_feature_gradient_through_zero_one_probabilities():
    """One unmasked agent per ego pixel (or none): the softmax weight is expf(0) / 1 = 1, grad_feats is a dyadic scatter of
    grad_out through tap weights 0, 1/4, 1/2, 1 -- bit for bit -- and grad_occ is exactly zero (q_a - 1 * q_a).  Ego columns 4, 10,
    11 and 15 are reached by no agent: nothing may be written from them."""
    fx = R.k5_exact_translation()
    ref = R.k5_reference(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    assert R.k5_exact_units(ref, fx["unit"]) < R.EXACT_LIMIT
    gf, go = run_k5(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    assert equal(gf, ref["g_feats"])
    assert int(torch.count_nonzero(go)) == 0
    assert float(np.abs(ref["g_feats"]).max()) > 0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_k5_every_instantiation_within_the_bound(n):
    """k_warp_fuse_backward<1> ... <8> (8 holds off[8][4] and tw[8][4] per thread) on one 16 x 8 map with half- and whole-pixel
    shifts that put taps of several agents off the map on each side; random occupancy logits: a real softmax."""
    H, W, C = 16, 8, 5
    feats, occ, gout = R.k5_ints(20 + n, n, C, H, W)
    _, _, ref = k5_bounded("k5_instantiation", feats, occ, R.shift_rows(R.FAR[:n], H, W), gout, n=n)
    if n > 1:
        assert float(np.abs(ref["g_occ"]).max()) > 0


@pytest.mark.parametrize("H,W", [(8, 32), (16, 64), (4, 4), (2, 32), (1, 1)])
def test_k5_tile_edges(H, W):
    """Exactly one 32 x 8 tile, four tiles, partial tiles, and the single pixel (base_coord with n <= 1)."""
    n, C = 3, 3
    feats, occ, gout = R.k5_ints(40 + H + W, n, C, H, W)
    k5_bounded("k5_tiles", feats, occ, R.shift_rows(R.FAR[:n], H, W), gout, H=H, W=W)


def test_k5_crop_window_edges():
    """A 1 x 1 window, a window touching row 0 / column 0, one touching H / W; half-pixel shifts make the taps straddle the window
    borders.  Outside its window an agent's grad_occ is exactly 0.0; inside, the bound holds."""
    n, C, H, W = 3, 3, 8, 16
    crop = [(2, 3, 5, 6), (0, 6, 0, 12), (3, 8, 6, 16)]
    feats, occ, gout = R.k5_ints(60, n, C, H, W)
    _, go, ref = k5_bounded("k5_crop", feats, occ, R.shift_rows([(0.0, 0.0), (0.5, 0.5), (-0.5, 1.0)], H, W), gout, crop)
    keep = torch.from_numpy(R.k5_keep(crop, n, H, W).reshape(n, 1, H, W))
    outside = go.cpu()[keep == 0]
    assert outside.numel() > 0 and int(torch.count_nonzero(outside)) == 0
    inside = ref["g_occ"][keep.numpy() == 1]
    assert float(np.abs(inside).max()) > 0 and all(float(np.abs(ref["g_occ"][a]).max()) > 0 for a in range(n))


def test_k5_collisions_add_up_exactly():
    """Scale 1/4: about sixteen ego pixels add into each source pixel.  Probabilities are 1 (the second agent's window is empty),
    the tap weights multiples of 1/64: a lost or doubled atomic is a wrong multiple, and the comparison is bit for bit."""
    fx = R.k5_collision()
    ref = R.k5_reference(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    assert R.k5_exact_units(ref, fx["unit"]) < R.EXACT_LIMIT and float(ref["n_feats"].max()) >= 16
    gf, go = run_k5(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    assert equal(gf, ref["g_feats"])
    assert int(torch.count_nonzero(gf[1])) == 0 and int(torch.count_nonzero(go)) == 0


def test_k5_device_poses():
    """The affine rows as a CUDA float64 tensor (the device branch of affine_row, warp_taps.h): within the bound on the n = 5 data of the
    instantiation test, and on the exact fixture bit-equal to the host-rows result (atomic order cannot matter there)."""
    n, H, W, C = 5, 16, 8, 5
    feats, occ, gout = R.k5_ints(20 + n, n, C, H, W)
    k5_bounded("k5_device_poses", feats, occ, R.shift_rows(R.FAR[:n], H, W), gout, dev_rows=True, n=n)
    fx = R.k5_exact_translation()
    host = run_k5(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])
    devp = run_k5(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"], dev_rows=True)
    assert torch.equal(host[0], devp[0]) and torch.equal(host[1], devp[1])
    assert equal(devp[0], R.k5_reference(fx["feats"], fx["occ"], fx["rows"], fx["grad_out"], fx["crop"])["g_feats"])


def test_k5_fp32_grid():
    """grid_f64=False: the reference builds its grid in float32 operation for operation as grid_point<float> does."""
    n, H, W, C = 3, 16, 8, 5
    feats, occ, gout = R.k5_ints(23, n, C, H, W)
    k5_bounded("k5_fp32_grid", feats, occ, R.shift_rows(R.FAR[:n], H, W), gout, grid_f64=False, n=n)


# =================================================================================================================== K4
def run_k4(fx, logit, feat, gout):
    """Camera matrices from the project's own entry point: identity rotations, intrinsics and post-rotation, zero post-translation,
    whole-cell translations -- and they come out as exactly that."""
    na, nc = fx["n_agents"], fx["n_cams"]
    eye = torch.eye(3, device=DEV).expand(na, nc, 3, 3).contiguous()
    trans = dev(fx["trans"]).view(na, nc, 3)
    cam = ops.camera_matrices(eye, trans, eye, eye, torch.zeros((na, nc, 3), device=DEV))
    want = torch.cat([torch.eye(3).reshape(1, 9).expand(na * nc, 9), torch.eye(3).reshape(1, 9).expand(na * nc, 9),
                      torch.zeros((na * nc, 3)), torch.from_numpy(fx["trans"]), torch.zeros((na * nc, 3))], 1)
    assert torch.equal(cam.cpu(), want)
    return ops.bev_pool_backward(dev(gout), dev(logit), dev(feat), dev(fx["frustum"]), cam, na, nc,
                                 [float(v) for v in fx["dx"]], [float(v) for v in fx["bx"]], [int(v) for v in fx["nx"]])


def k4_exact(fx, D, C, seed):
    assert D & (D - 1) == 0 and R.k4_exact_units(D, C, 2) < R.EXACT_LIMIT
    logit, feat, gout = R.k4_data(fx, D, C, seed, True)
    ref = R.k4_reference(fx, logit, feat, gout)
    gl, gf = run_k4(fx, logit, feat, gout)
    assert equal(gf, ref["g_feat"]), float(np.abs(gf.cpu().double().numpy() - ref["g_feat"]).max())
    assert equal(gl, ref["g_logit"]), float(np.abs(gl.cpu().double().numpy() - ref["g_logit"]).max())
    return gl, gf, ref


@pytest.mark.parametrize("D", [4, 64])
def test_k4_exact(D):
    """Equal logits: p = 1 / D exactly; integer features and gradients: both outputs bit for bit."""
    fx = R.k4_fixture(R.k4_centres(D, 2, 3, D), [(0, 0, 0)], 1, 1)
    _, _, ref = k4_exact(fx, D, 5, 1)
    assert float(np.abs(ref["g_logit"]).max()) > 0 and float(np.abs(ref["g_feat"]).max()) > 0


@pytest.mark.parametrize("C", [1, 63, 64, 65, 256])
def test_k4_channel_guards(C):
    """Lane l owns channels l + 64 k, k < 4, under c < C guards: one channel, one short of a lane row, exactly one, one over, all four."""
    fx = R.k4_fixture(R.k4_centres(4, 2, 3, C), [(0, 0, 0)], 1, 1)
    k4_exact(fx, 4, C, 2)


@pytest.mark.parametrize("D", [1, 3, 63, 64])
def test_k4_depth_lanes_within_the_bound(D):
    """Lanes >= D take -inf and must drop out of the softmax and of both reductions; random logits."""
    C = 5
    fx = R.k4_fixture(R.k4_centres(D, 2, 3, 10 + D), [(0, 0, 0)], 1, 1)
    logit, feat, gout = R.k4_data(fx, D, C, 3, False)
    ref = R.k4_reference(fx, logit, feat, gout)
    gl, gf = run_k4(fx, logit, feat, gout)
    kf, kl = R.k4_k(D)
    ok_f = within("k4_depth:grad_feat", gf, ref["g_feat"], R.EPS * kf * ref["T_feat"], D=D)
    ok_l = within("k4_depth:grad_logit", gl, ref["g_logit"], R.EPS * kl * ref["T_logit"], D=D)
    assert ok_f and ok_l
    if D == 1:
        assert int(torch.count_nonzero(gl)) == 0           # p = expf(0) / 1 = 1 and s - 1 * s = 0: exactly


def test_k4_agents_and_cameras():
    """Three agents of two cameras, every camera translated to other cells, grad_out different per agent: a kernel that read another
    agent's rows (b = bn / n_cams, b * cells in the key) would be exactly wrong."""
    cams = [(0, 0, 0), (1, -2, 0), (-2, 1, 0), (2, 2, 0), (0, -1, 0), (-1, 0, 0)]
    fx = R.k4_fixture(R.k4_centres(4, 2, 3, 4, 2, 6), cams, 3, 2)
    assert len({fx["cell"][b].tobytes() for b in range(6)}) == 6
    k4_exact(fx, 4, 5, 4)


def test_k4_two_z_bins():
    """nx[2] = 2 with points in both bins: pins the channel order z * C + c of grad_out's re-layout in ops.bev_pool_backward, the
    layout oracle_np.bev_pool produces (final[b, :, z, y, x], z slices concatenated along the channels; checked on the forward
    oracle in tests/test_backward_refs_cpu.py::test_k4_reference_equals_float64_index_add_autograd[two_z])."""
    fx = R.k4_fixture(R.k4_centres(4, 2, 3, 5), [(0, 0, 0), (1, 0, -1)], 1, 2, nz=2)
    iz = [fx["cell"][b][fx["cell"][b] >= 0] // 64 for b in range(2)]
    assert set(np.unique(iz[0])) == {1} and set(np.unique(iz[1])) == {0}
    k4_exact(fx, 4, 3, 5)


def test_k4_out_of_the_grid_and_the_truncation_rule():
    """A pixel with every bin outside gets exactly zero gradients; a point half a cell below the grid (lo - dx / 2) is cell 0 by the
    reference's truncation toward zero, lo - dx is out, and the far edge fx = nx is out -- on x and on y."""
    fx = R.k4_fixture(R.k4_edge_positions(), [(0, 0, 0)], 1, 1)
    cell = fx["cell"][0]
    assert (cell[:, 0, 0] == -1).all() and cell[0, 0, 1] % 8 == 0 and cell[0, 0, 1] >= 0 and (cell[1:3, 0, 1] == -1).all()
    assert cell[0, 1, 2] >= 0 and (cell[0, 1, 2] // 8) % 8 == 0 and (cell[1:3, 1, 2] == -1).all()
    gl, gf, ref = k4_exact(fx, 4, 5, 6)
    assert int(torch.count_nonzero(gl[0, :, 0, 0])) == 0 and int(torch.count_nonzero(gf[0, :, 0, 0])) == 0
    assert float(np.abs(ref["g_feat"][0, :, 0, 1]).max()) > 0


def test_k4_collisions():
    """All D bins of a pixel in one cell, and all six pixels of two cameras in that same cell."""
    fpos = np.full((4, 2, 3, 2), 3.5)
    fpos[..., 1] = 5.5
    fx = R.k4_fixture(fpos, [(0, 0, 0), (0, 0, 0)], 1, 2)
    assert len(np.unique(fx["cell"])) == 1 and fx["cell"].min() >= 0
    gl, _, ref = k4_exact(fx, 4, 5, 7)
    assert int(torch.count_nonzero(gl)) == 0 and float(np.abs(ref["g_feat"]).max()) > 0      # every s_d equal: s - sum p s = 0


@pytest.mark.parametrize("fH,fW", [(1, 1), (1, 5), (7, 1)])
def test_k4_ragged_launch(fH, fW):
    """1, 5 and 7 pixels: not multiples of the four waves of a block."""
    fx = R.k4_fixture(R.k4_centres(4, fH, fW, fH + fW), [(0, 0, 0)], 1, 1)
    k4_exact(fx, 4, 5, 8)


# =================================================================================================================== K2
K2_M = (1, 3, 4, 5, 16, 17, 67)
K2_P = (1, 16, 17, 31, 32)


def run_k2(vox, coords, nps, prm, grad):
    v, c, n = dev(vox), dev(coords), dev(nps)
    w, sc, sh, mu, rs = (dev(prm[k]) for k in ("weight", "scale", "shift", "mean", "rstd"))
    s1, S = ops.pfn_moments(v, c, n, R.K2_VOXEL, R.K2_RANGE)
    out = ops.pfn_features(v, c, n, w, sc, sh, R.K2_VOXEL, R.K2_RANGE)
    A, B, Cx = ops.pfn_backward(v, c, n, w, sc, sh, mu, rs, R.K2_VOXEL, R.K2_RANGE, dev(np.asarray(grad, np.float32)))
    return dict(s1=s1, S=S, out=out, A=A, B=B, Cx=Cx)


def k2_exact(vox, coords, nps, prm, grad):
    """Moments, features and the three backward sums bit for bit on a dyadic fixture -> (kernel results, reference)."""
    f, _ = R.k2_features64(vox, coords, nps)
    assert np.array_equal(f * 4, np.round(f * 4)) and R.k2_exact_units(f, prm, float(np.abs(grad).max())) < R.EXACT_LIMIT
    got = run_k2(vox, coords, nps, prm, grad)
    s1, S = R.k2_moments(f)
    ref = R.k2_backward(f, nps, prm, grad, tie="kernel")
    ref.update(s1=s1, S=S, out=R.k2_forward(f, nps, prm)[0])
    for k in ("s1", "S", "out", "A", "B", "Cx"):
        g, r = got[k].cpu().double(), torch.from_numpy(ref[k])
        assert torch.equal(g, r), (k, float((g - r).abs().max()))
    return got, ref


@pytest.mark.parametrize("P", K2_P)
@pytest.mark.parametrize("M", K2_M)
def test_k2_exact_moments_features_and_backward_sums(M, P):
    """Partial waves and partial blocks (four pillars per wave, sixteen per block: M = 1, 3, 5, 17, 67), both sides of `i + 16 < P`,
    point counts from 1 to P; integer grad_pillar, power-of-two rstd and integer mean make Cx exact too."""
    vox, coords, nps = R.k2_pillars(M, P, seed=100 * M + P)
    grad = np.random.default_rng(M + P).integers(-2, 3, (M, 64)).astype(np.float64)
    k2_exact(vox, coords, nps, R.k2_params(7 * M + P), grad)


def _k2_intensity_only(P, nps, shift, w3):
    """Pillars whose z depends on the (positive) intensity alone: weight[c] = w3 on feature 3, 0 elsewhere; scale 1."""
    M = len(nps)
    vox, coords, nps = R.k2_pillars(M, P, seed=9, nps=nps)
    g = np.random.default_rng(4)
    vox[:, :, 3] = g.integers(1, 3, (M, P)) * (np.arange(P)[None, :] < nps[:, None])
    prm = R.k2_params(3)
    prm["weight"] = np.zeros((64, 10), np.float32)
    prm["weight"][:, 3] = w3
    prm["scale"] = np.ones(64, np.float32)
    prm["shift"] = np.full(64, shift, np.float32)
    grad = g.integers(1, 3, (M, 64)).astype(np.float64) * np.where(g.integers(0, 2, (M, 64)) > 0, 1, -1)
    return vox, coords, nps, prm, grad


def test_k2_padding_row_wins():
    """np < P and every real row below relu(shift) = 3: the arg-max is a padding row.  A gets nothing from it, B gets dy, Cx gets
    dy * (0 - mean) * rstd."""
    vox, coords, nps, prm, grad = _k2_intensity_only(8, [1, 3, 7, 4, 2], 3.0, -1.0)
    got, ref = k2_exact(vox, coords, nps, prm, grad)
    assert ref["pad_wins"].all() and (ref["out"] == 3.0).all()
    assert int(torch.count_nonzero(got["A"])) == 0
    assert torch.equal(got["B"].cpu(), torch.from_numpy(grad.sum(0)))
    want_cx = (grad * (0.0 - prm["mean"].astype(np.float64)) * prm["rstd"].astype(np.float64)).sum(0)
    assert torch.equal(got["Cx"].cpu(), torch.from_numpy(want_cx)) and float(np.abs(want_cx).max()) > 0


def test_k2_padding_row_absent():
    """np == P, shift = 3 > 0, every real y = relu(3 - 8 I) = 0: there is no padding row to take relu(shift); a real row wins with
    y = 0 and dy = 0: no gradient at all, and the feature is 0, not 3."""
    vox, coords, nps, prm, grad = _k2_intensity_only(8, [8, 8, 8, 8, 8], 3.0, -8.0)
    got, ref = k2_exact(vox, coords, nps, prm, grad)
    assert not ref["pad_wins"].any()
    for k in ("out", "A", "B", "Cx"):
        assert int(torch.count_nonzero(got[k])) == 0, k


def test_k2_all_negative_pillar():
    """np < P, shift = -1: every row, real or padding, has y = 0: no gradient anywhere."""
    vox, coords, nps, prm, grad = _k2_intensity_only(8, [1, 3, 7, 4, 2], -1.0, -1.0)
    got, _ = k2_exact(vox, coords, nps, prm, grad)
    for k in ("out", "A", "B", "Cx"):
        assert int(torch.count_nonzero(got[k])) == 0, k


@pytest.mark.parametrize("P", [1, 8, 32])
def test_k2_single_point_pillars(P):
    """np = 1: the mean is the point, the three point - mean features are exactly zero."""
    M = 5
    vox, coords, nps = R.k2_pillars(M, P, seed=12, nps=[1] * M)
    f, _ = R.k2_features64(vox, coords, nps)
    assert float(np.abs(f[:, :, 4:7]).max()) == 0.0 and float(np.abs(f[:, 0, :4]).max()) > 0
    grad = np.random.default_rng(P).integers(-2, 3, (M, 64)).astype(np.float64)
    got, _ = k2_exact(vox, coords, nps, R.k2_params(13), grad)
    assert int(torch.count_nonzero(got["S"][4:7])) == 0 and int(torch.count_nonzero(got["A"][:, 4:7])) == 0


def test_k2_random_floats_within_the_bound():
    """Normal data, M = 67, P = 20: guards against an exact fixture being blind to something.  The fixture has no near-ties between
    the two best rows of any (pillar, channel) (asserted here and on the CPU), so the arg-max rows agree with the reference."""
    vox, coords, nps, prm = R.k2_random()
    f, fabs = R.k2_features64(vox, coords, nps)
    assert R.k2_argmax_margin(f, fabs, nps, prm) > 0
    grad = np.random.default_rng(1).standard_normal((vox.shape[0], 64)).astype(np.float32)
    got = run_k2(vox, coords, nps, prm, grad)
    ref = R.k2_backward(f, nps, prm, grad, tie="kernel", fabs=fabs)
    s1, S = R.k2_moments(f)
    ref.update(s1=s1, S=S, out=R.k2_forward(f, nps, prm)[0], T_s1=fabs.sum((0, 1)), T_S=np.einsum("mpj,mpk->jk", fabs, fabs),
               T_out=R.k2_out_T(fabs, nps, prm))
    k = R.k2_k()
    oks = [within("k2_random:" + name, got[name], ref[name], R.EPS * k[name] * ref["T_" + name])
           for name in ("s1", "S", "out", "A", "B", "Cx")]
    assert all(oks), oks
