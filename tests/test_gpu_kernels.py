"""Parity of the gfx950 kernels (through the C ABI) against the oracle and the reference's golden
vectors.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from oracle import cref
from oracle import oracle_np as O
from tests.golden.detfill import det_values

pytestmark = pytest.mark.gpu

PP_RANGE = [-102.4, -102.4, -3, 102.4, 102.4, 1]


def _need_experimental():
    """The measured-negative kernels (include/heal_amd_experimental.h) exist only in a HEAL_BUILD_EXPERIMENTAL=1 library."""
    from heal_amd import ops
    if not ops.experimental_build():
        pytest.skip("libheal_amd.so was built without HEAL_BUILD_EXPERIMENTAL=1 (measured-negative kernels are not shipped)")



def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def check_voxelize(pts, lidar_range, voxel_size, P, max_voxels):
    from heal_amd import ops
    v, c, n = ops.voxelize(dev(pts), lidar_range, voxel_size, P, max_voxels, batch_idx=3)
    ov, oc, on = cref.voxelize(pts, lidar_range, voxel_size, P, max_voxels, batch_idx=3)
    assert v.shape[0] == ov.shape[0], (v.shape, ov.shape)
    np.testing.assert_array_equal(c.cpu().numpy(), oc)
    np.testing.assert_array_equal(n.cpu().numpy(), on)
    # bit-exact copy of the points (compare as raw bits so that NaN payloads count too)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), ov.view(np.uint32))
    return ov.shape[0]


# ---------------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("seed", [1000, 1001])
def test_voxelize_pointpillars_full_frame(seed):
    from heal_amd import synth
    pts = synth.lidar_frame(seed)
    m = check_voxelize(pts, PP_RANGE, [0.4, 0.4, 4], 32, 70000)
    assert m > 3000


def test_voxelize_second_grid_and_voxel_cap():
    from heal_amd import synth
    pts = synth.lidar_frame(1002)
    check_voxelize(pts, PP_RANGE, [0.1, 0.1, 0.1], 5, 70000)      # 41 x 2048 x 2048 cells: hash path
    check_voxelize(pts, PP_RANGE, [0.1, 0.1, 0.1], 5, 3000)       # max_voxels cap reached
    check_voxelize(pts, PP_RANGE, [0.4, 0.4, 4], 3, 100)          # both caps


def test_voxelize_edge_cases():
    rng = np.random.default_rng(0)
    R = [-4.0, -4.0, -3.0, 4.0, 4.0, 1.0]
    V = [0.4, 0.4, 4.0]
    # every point outside
    pts = rng.uniform(5, 9, (257, 4)).astype(np.float32)
    assert check_voxelize(pts, R, V, 8, 100) == 0
    # exactly on the boundaries (lower inclusive, upper exclusive), negative zero, duplicates, NaN
    pts = np.array([[-4.0, -4.0, -3.0, 0.1], [4.0, 0.0, 0.0, 0.2], [0.0, 4.0, 0.0, 0.3], [0.0, 0.0, 1.0, 0.4],
                    [-0.0, -0.0, -0.0, 0.5], [0.0, 0.0, 0.0, 0.6], [3.9999998, 3.9999998, 0.9999999, 0.7],
                    [np.nan, 0.0, 0.0, 0.8], [0.0, np.inf, 0.0, 0.9], [0.4, 0.8, 0.0, 1.0],
                    [0.4, 0.8, 0.0, 1.0], [0.39999998, 0.8000001, 0.0, 1.1]], np.float32)
    assert check_voxelize(pts, R, V, 8, 100) > 0
    # many points in a single voxel (> max_points) and a single point
    pts = np.concatenate([rng.uniform(0.0, 0.39, (500, 4)), rng.uniform(-3.9, 3.9, (300, 4))]).astype(np.float32)
    check_voxelize(pts, R, V, 8, 100)
    check_voxelize(pts[:1], R, V, 8, 100)
    # ragged sizes around the tile boundaries of the scan / sort
    for n in (63, 64, 65, 2047, 2048, 2049, 4097):
        check_voxelize(rng.uniform(-4.5, 4.5, (n, 4)).astype(np.float32), R, V, 4, 50)


@pytest.mark.parametrize("P", [1, 2, 3, 12, 32, 48, 64, 80, 200])
def test_voxelize_every_group_size_and_long_segments(P):
    """The selection stage of K1 at every lane-group size (G = 1, 2, 4, 16, 32, 64 lanes per voxel for max_points <= 64) and on
    its max_points > 64 path (atomicMin cascade), with cells that hold far more points than max_points (the first P in INPUT
    order must survive whatever order the atomics ran in), cells with exactly P, P - 1 and one point, interleaved over the cloud
    so that a cell's points come from many different waves and blocks."""
    rng = np.random.default_rng(100 + P)
    R = [-4.0, -4.0, -3.0, 4.0, 4.0, 1.0]
    V = [0.4, 0.4, 4.0]
    dense = rng.uniform(0.0, 0.39, (5 * P + 700, 4))                                 # one cell, >> P points
    dense2 = rng.uniform(0.0, 0.39, (3 * P + 64, 4)) + np.array([0.8, 0.0, 0.0, 0.0])  # another, > P
    exact = rng.uniform(0.0, 0.39, (P, 4)) + np.array([-0.8, 0.4, 0.0, 0.0])          # exactly P
    short = rng.uniform(0.0, 0.39, (max(P - 1, 1), 4)) + np.array([-1.6, -0.8, 0.0, 0.0])
    spread = rng.uniform(-3.9, 3.9, (3000, 4))
    pts = np.concatenate([dense, dense2, exact, short, spread]).astype(np.float32)
    pts = pts[rng.permutation(pts.shape[0])]
    assert check_voxelize(pts, R, V, P, 1000) > 300
    check_voxelize(pts, R, V, P, 37)                                                  # voxel cap on top
    from heal_amd import ops
    got = ops.voxelize_collated([dev(pts), dev(pts[::2].copy())], R, V, P, 1000)       # the batched form shares the chain
    m = [int(v) for v in got[3].cpu()]
    for b, cloud in enumerate((pts, pts[::2].copy())):
        ov, oc, on = cref.voxelize(cloud, R, V, P, 1000, batch_idx=b)
        sl = slice(m[b], m[b + 1])
        assert m[b + 1] - m[b] == ov.shape[0]
        np.testing.assert_array_equal(got[0][sl].cpu().numpy().view(np.uint32), ov.view(np.uint32))
        np.testing.assert_array_equal(got[1][sl].cpu().numpy(), oc)
        np.testing.assert_array_equal(got[2][sl].cpu().numpy(), on)


def test_voxelize_round_trip_property():
    """Size-independent properties at full size: every in-range point lands in exactly the voxel of
    its cell, no voxel is empty, slots keep input order."""
    from heal_amd import ops, synth
    pts = synth.lidar_frame(1003)
    v, c, n = ops.voxelize(dev(pts), PP_RANGE, [0.4, 0.4, 4], 32, 70000)
    v, c, n = v.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy()
    assert n.min() >= 1 and n.max() <= 32
    cells = c[:, 1].astype(np.int64) * 512 * 512 + c[:, 2] * 512 + c[:, 3]
    assert len(np.unique(cells)) == len(cells)
    fx = np.floor((pts[:, 0] - np.float32(-102.4)) / np.float32(0.4))
    fy = np.floor((pts[:, 1] - np.float32(-102.4)) / np.float32(0.4))
    fz = np.floor((pts[:, 2] - np.float32(-3)) / np.float32(4))
    inr = (fx >= 0) & (fx < 512) & (fy >= 0) & (fy < 512) & (fz >= 0) & (fz < 1)
    pcell = (fz[inr] * 512 * 512 + fy[inr] * 512 + fx[inr]).astype(np.int64)
    ucell, cnt = np.unique(pcell, return_counts=True)
    assert np.array_equal(np.sort(cells), ucell)
    assert n.sum() == np.minimum(cnt, 32).sum()
    mask = np.arange(32)[None, :] < n[:, None]
    assert np.all(v[~mask] == 0)


# ---------------------------------------------------------------------------------------------- K2
def pfn_params():
    pre = "pillar_vfe.pfn_layers.0."
    w = det_values(pre + "linear.weight", (64, 10), "weight")
    g = det_values(pre + "norm.weight", (64,), "bn_weight")
    b = det_values(pre + "norm.bias", (64,), "bn_bias")
    mu = det_values(pre + "norm.running_mean", (64,), "running_mean")
    var = det_values(pre + "norm.running_var", (64,), "running_var")
    scale = (g / np.sqrt(var + np.float32(1e-3))).astype(np.float32)
    shift = (b - mu * scale).astype(np.float32)
    return dict(weight=w, bn_gamma=g, bn_beta=b, bn_mean=mu, bn_var=var), w, scale, shift


def test_pfn_scatter_matches_reference_golden(golden):
    from heal_amd import ops
    g = golden("pointpillar_encoder")
    _, w, scale, shift = pfn_params()
    canvas, pillars = ops.pfn_scatter(dev(g["voxel_features"]), dev(g["voxel_coords"], torch.int32),
                                      dev(g["voxel_num_points"], torch.int32), dev(w), dev(scale), dev(shift),
                                      g["voxel_size"].tolist(), g["lidar_range"].tolist(), 2, 128, 128,
                                      return_pillars=True)
    np.testing.assert_allclose(pillars.cpu().numpy(), g["pillar_features"], rtol=1e-3, atol=1e-5)
    c = canvas.cpu().numpy()
    np.testing.assert_allclose(c, g["spatial_features"], rtol=1e-3, atol=1e-5)
    assert np.array_equal(c != 0, g["spatial_features"] != 0)


def test_pfn_scatter_full_size_vs_oracle():
    from heal_amd import ops, synth
    params, w, scale, shift = pfn_params()
    vs, cs, ns = [], [], []
    for b, seed in enumerate((1000, 1001)):
        v, c, n = cref.voxelize(synth.lidar_frame(seed), PP_RANGE, [0.4, 0.4, 4], 32, 70000, batch_idx=b)
        vs.append(v); cs.append(c); ns.append(n)
    v, c, n = np.concatenate(vs), np.concatenate(cs), np.concatenate(ns)
    canvas = ops.pfn_scatter(dev(v), dev(c), dev(n), dev(w), dev(scale), dev(shift), [0.4, 0.4, 4], PP_RANGE,
                             2, 512, 512).cpu().numpy()
    ref, _ = O.pfn_scatter(v, c, n, voxel_size=[0.4, 0.4, 4], lidar_range=PP_RANGE, n_agents=2, ny=512, nx=512,
                           **params)
    np.testing.assert_allclose(canvas, ref, rtol=1e-3, atol=1e-5)
    assert np.array_equal(canvas != 0, ref != 0)
    # every pillar occupies exactly one canvas cell (some channels may be exactly 0 after ReLU)
    occupied = (canvas != 0).any(axis=1).sum()
    assert occupied <= len(n) and occupied >= 0.99 * len(n)


def test_pfn_pillars_equal_pfn_scatter(golden):
    """Round 6: heal_pfn_pillars (K2 without the canvas) returns the same pillar features, and heal_pillar_canvas of its
    (cell map, pillars) pair is heal_pfn_scatter's canvas bit for bit (and the reference's golden canvas)."""
    from heal_amd import ops
    g = golden("pointpillar_encoder")
    _, w, scale, shift = pfn_params()
    args = (dev(g["voxel_features"]), dev(g["voxel_coords"], torch.int32), dev(g["voxel_num_points"], torch.int32), dev(w),
            dev(scale), dev(shift), g["voxel_size"].tolist(), g["lidar_range"].tolist(), 2, 128, 128)
    canvas, pillars = ops.pfn_scatter(*args, return_pillars=True)
    pb = ops.pfn_pillars(*args)
    assert torch.equal(pb.pillars[:pillars.shape[0]], pillars)
    assert torch.equal(pb.dense(), canvas)
    m = pb.cell_map.cpu().numpy()
    c = g["voxel_coords"].astype(np.int64)
    idx = c[:, 1] + c[:, 2] * 128 + c[:, 3]
    ok = (c[:, 0] >= 0) & (c[:, 0] < 2) & (idx >= 0) & (idx < 128 * 128)
    key, rows = c[ok, 0] * 128 * 128 + idx[ok], np.nonzero(ok)[0]
    cells = np.unique(key)
    assert int((m >= 0).sum()) == len(cells) > 0              # one entry per distinct in-grid cell of the golden's coordinates
    last = np.full(2 * 128 * 128, -1, np.int64)
    np.maximum.at(last, key, rows)
    assert np.array_equal(m.reshape(-1)[cells], last[cells])   # ... and it is the largest row with that cell
    np.testing.assert_allclose(pb.dense().cpu().numpy(), g["spatial_features"], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("layout", ["lanes", "tiles"])
@pytest.mark.parametrize("n_agents,ny,nx,rng_,seeds", [(2, 512, 512, PP_RANGE, (1000, 1001)),
                                                        (1, 240, 480, [-96, -48, -3, 96, 48, 1], (1002,)),
                                                        (3, 128, 128, [-25.6, -25.6, -3, 25.6, 25.6, 1], (1003, 1004, 1005)),
                                                        (1, 40, 24, [-4.8, -8.0, -3, 4.8, 8.0, 1], (1006,))])
def test_pillar_stem_block_equals_dense_path(n_agents, ny, nx, rng_, seeds, layout):
    """heal_pillar_stem_block (first BasicBlock convolutions of the PointPillars backbone read from the pillar rows through the
    cell map; the canvas is never written) against the dense path it replaces -- the canvas + torch's fp64 3x3 / stride 2 and 1x1 /
    stride 2 convolutions: 1e-5 of the output scale (summation order), background pixels exactly relu(bias) / bias.  Full 512 x 512
    and native 480 x 240 grids, a small one, and a map smaller than the tile raster (40 x 24 -> 20 x 12 outputs: ragged tiles)."""
    from heal_amd import ops, synth
    _, w, scale, shift = pfn_params()
    vs, cs, ns = [], [], []
    for b, seed in enumerate(seeds):
        v, c, n = cref.voxelize(synth.lidar_frame(seed), rng_, [0.4, 0.4, 4], 32, 70000, batch_idx=b)
        vs.append(v); cs.append(c); ns.append(n)
    args = (dev(np.concatenate(vs)), dev(np.concatenate(cs)), dev(np.concatenate(ns)), dev(w), dev(scale), dev(shift),
            [0.4, 0.4, 4], rng_, n_agents, ny, nx)
    canvas = ops.pfn_scatter(*args)
    pb = ops.pfn_pillars(*args)
    g = torch.Generator().manual_seed(ny * 7 + nx)
    w1 = (torch.randn((64, 64, 3, 3), generator=g) / 24.0).cuda()
    wd = (torch.randn((64, 64, 1, 1), generator=g) / 8.0).cuda()
    b1, bd = torch.randn((64,), generator=g).cuda(), torch.randn((64,), generator=g).cuda()
    assert pb.stem_supported(64, 64)
    pb.weight_layout = layout       # "lanes": the pixel-compacted production kernel; "tiles": the round's first version (A/B)
    wm, wdf = pb.fragments(w1, wd)
    got_main, got_id = pb.stem_block(wm, b1, wdf, bd)
    ref_main = torch.relu(torch.nn.functional.conv2d(canvas.double(), w1.double(), b1.double(), 2, 1))
    ref_id = torch.nn.functional.conv2d(canvas.double(), wd.double(), bd.double(), 2, 0)
    assert got_main.shape == ref_main.shape and got_id.shape == ref_id.shape
    for got, ref in ((got_main, ref_main), (got_id, ref_id)):
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        assert err < 1e-5, err
    # pixels no pillar reaches: exactly the bias (ReLU on the conv1 half)
    occ = (canvas != 0).any(1, keepdim=True).float()
    reach = torch.nn.functional.max_pool2d(torch.nn.functional.pad(occ, (1, 1, 1, 1)), 3, 2) == 0
    bg_main = torch.relu(b1)[None, :, None, None].expand_as(got_main)
    assert torch.equal(got_main[reach.expand_as(got_main)], bg_main[reach.expand_as(got_main)])
    # no bias
    got2, _ = pb.stem_block(wm, None, wdf, None)
    ref2 = torch.relu(torch.nn.functional.conv2d(canvas.double(), w1.double(), None, 2, 1))
    assert float((got2.double() - ref2).abs().max() / ref2.abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------- K5
@pytest.mark.parametrize("tag", ["sq", "rect", "f32"])
def test_warp_fuse_matches_reference_golden(golden, tag):
    from heal_amd import ops
    g = golden("warp_fuse")
    x, score = g[f"{tag}_x"], g[f"{tag}_score"]
    n = x.shape[0]
    rows = g[f"{tag}_affine"][0, :n]
    f64 = rows.dtype == np.float64
    # the kernel builds the score from occupancy logits; feed logit(score - 1e-4) ... except that the
    # fixture also contains exact zeros, which a sigmoid cannot produce -> use the split API whose
    # second half takes scores directly, and the fused kernel on a zero-free variant below
    feats_ego, scores_ego = [], []
    for a in range(n):
        fe, _ = ops.warp_agent(dev(x[a]), dev(np.zeros_like(score[a])), rows[a], grid_f64=f64)
        se, _ = ops.warp_agent(dev(score[a]), dev(np.zeros_like(score[a])), rows[a], grid_f64=f64)
        feats_ego.append(fe); scores_ego.append(se)
    fe = torch.stack(feats_ego); se = torch.stack(scores_ego)
    np.testing.assert_allclose(fe.cpu().numpy(), g[f"{tag}_warped"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(se.cpu().numpy(), g[f"{tag}_wscore"], rtol=1e-4, atol=2e-5)
    assert np.array_equal(se.cpu().numpy() == 0, g[f"{tag}_wscore"] == 0)
    fused = ops.fuse_warped(fe, se)
    np.testing.assert_allclose(fused.cpu().numpy(), g[f"{tag}_fused"], rtol=1e-3, atol=2e-5)


@pytest.mark.parametrize("n,C,H,W,f64", [(3, 64, 64, 64, True), (5, 128, 128, 128, True), (2, 16, 24, 40, False),
                                         (1, 8, 32, 32, True), (8, 8, 16, 16, True)])
def test_warp_fuse_fused_vs_oracle(n, C, H, W, f64):
    from heal_amd import ops, synth
    rng = np.random.default_rng(n * 100 + C)
    x = rng.standard_normal((n, C, H, W)).astype(np.float32)
    occ = (rng.standard_normal((n, 1, H, W)) * 2).astype(np.float32)
    Hm, Wm = 0.8 * H, 0.8 * W
    poses = synth.agent_poses(7 + n, n, r_min=2.0, r_max=0.3 * min(Hm, Wm))
    pw = synth.pairwise_t_matrix(poses, 8)[None].astype(np.float64 if f64 else np.float32)
    rows = O.normalize_pairwise_tfm(pw, Hm, Wm, 1)[0][0, :n]
    mods = ["m1"] * n
    crop_info = {}
    crops = None
    if n >= 3:  # make agent 1 a camera agent with a crop window
        mods[1] = "m2"
        crop_info = {"m2": {"crop_ratio_H_m2": 2.0, "crop_ratio_W_m2": 2.0}}
        from heal_amd.opencood.models.fuse_modules.pyramid_fuse import crop_window
        crops = [crop_window(H, W, 2.0, 2.0) if m == "m2" else (0, 0, 0, 0) for m in mods]
    out = ops.warp_fuse(dev(x), dev(occ), rows, grid_f64=f64, crop=crops).cpu().numpy()
    score = O.occ_to_score(occ, O.camera_crop_mask(n, H, W, mods, crop_info))
    ref = O.weighted_fuse(x, score, rows)
    np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5)
    # split form == fused form
    fe, se = zip(*[ops.warp_agent(dev(x[a]), dev(occ[a]), rows[a], grid_f64=f64,
                                  crop=None if crops is None else [crops[a]]) for a in range(n)])
    out2 = ops.fuse_warped(torch.stack(fe), torch.stack(se)).cpu().numpy()
    np.testing.assert_allclose(out2, out, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("tag", ["sq", "rect", "f32"])
def test_warp_agents_token_major_matches_reference_golden(golden, tag):
    """heal_warp_agents_pm (all agents of a scene, written [n,H,W,C]) against the reference's warp_affine_simple output, and
    bit-equal to the per-agent kernel it replaces at V2X-ViT's entry; channel counts that do not fill a 64-channel block,
    maps that do not fill a 16 x 4 tile, device-resident affine rows."""
    from heal_amd import ops
    g = golden("warp_fuse")
    x = g[f"{tag}_x"]
    n = x.shape[0]
    rows = g[f"{tag}_affine"][0, :n]
    f64 = rows.dtype == np.float64
    pm = ops.warp_agents_pm(dev(x), rows, grid_f64=f64)
    assert pm.shape == (n, x.shape[2], x.shape[3], x.shape[1]) and pm.is_contiguous()
    np.testing.assert_allclose(pm.permute(0, 3, 1, 2).cpu().numpy(), g[f"{tag}_warped"], rtol=1e-4, atol=2e-5)
    per_agent = torch.stack([ops.warp_agent(dev(x[a]), dev(np.zeros_like(x[a][:1])), rows[a], grid_f64=f64)[0] for a in range(n)])
    assert torch.equal(pm.permute(0, 3, 1, 2), per_agent)
    rng = np.random.default_rng(3)
    for (m, C, H, W) in ((8, 256, 128, 128), (3, 72, 30, 50), (1, 4, 5, 7)):
        y = torch.from_numpy(rng.standard_normal((m, C, H, W)).astype(np.float32)).cuda()
        r = np.tile(np.array([[1, 0, 0, 0, 1, 0]], dtype=np.float64), (m, 1)) + 0.2 * rng.standard_normal((m, 6))
        a = ops.warp_agents_pm(y, r)
        b = torch.stack([ops.warp_agent(y[i], y[i][:1], r[i])[0] for i in range(m)])
        assert torch.equal(a.permute(0, 3, 1, 2), b), (m, C, H, W)
        assert torch.equal(ops.warp_agents_pm(y, torch.from_numpy(r).cuda()), a)


def test_warp_fuse_identity_is_exact():
    """Linearity / idempotence property: one agent, identity transform -> output == input."""
    from heal_amd import ops
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 64, 256, 256)).astype(np.float32)
    occ = rng.standard_normal((1, 1, 256, 256)).astype(np.float32)
    rows = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    out = ops.warp_fuse(dev(x), dev(occ), rows, grid_f64=True).cpu().numpy()
    np.testing.assert_allclose(out, x[0], rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------- K8
def _survivor_anchor_indices(cand_corners, cand_anchor_idx, boxes, tol=1e-4):
    """Anchor index of every output box: the candidate (oracle decode, anchor order) whose 8 corners it reproduces."""
    flat = cand_corners.reshape(len(cand_corners), -1).astype(np.float64)
    out = np.empty(len(boxes), np.int64)
    for i, b in enumerate(boxes.reshape(len(boxes), -1).astype(np.float64)):
        d = np.abs(flat - b).max(1)
        j = int(np.argmin(d))
        assert d[j] < tol, (i, d[j])
        out[i] = cand_anchor_idx[j]
    return out


def test_quad_iou_bit_exact_vs_oracle(golden):
    from heal_amd import ops
    g = golden("decode")
    q = np.ascontiguousarray(g["cmp_proj"][:, :4, :2])
    rng = np.random.default_rng(2)
    extra = q[rng.integers(0, len(q), 64)] + rng.normal(0, 0.5, (64, 1, 2)).astype(np.float32)
    allq = np.concatenate([q, extra.astype(np.float32), np.zeros((1, 4, 2), np.float32), q[:3][:, ::-1]])
    got = ops.quad_iou(dev(allq), dev(allq)).cpu().numpy()
    want = cref.quad_iou(allq, allq)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))  # bit exact incl. NaN


@pytest.mark.parametrize("tag", ["id", "tf"])
def test_decode_nms_matches_reference_golden(golden, tag):
    from heal_amd import ops
    g = golden("decode")
    anchors = dev(g["anchors"].astype(np.float32))
    pred, score = ops.decode_nms(dev(g[f"{tag}_cls"]), dev(g[f"{tag}_reg"]), dev(g[f"{tag}_dir"]), anchors,
                                 0.2, 0.7853, 2, 0.15, g[f"{tag}_tfm"], g["gt_range"].tolist())
    assert pred.shape == g[f"{tag}_pred"].shape
    np.testing.assert_allclose(score.cpu().numpy(), g[f"{tag}_score"], rtol=1e-5, atol=1e-6)
    # against the REFERENCE's boxes (torch CPU transcendental functions vs the device's: a few ulps of +-100 m coordinates)
    np.testing.assert_allclose(pred.cpu().numpy(), g[f"{tag}_pred"], rtol=1e-5, atol=1e-4)


def test_decode_nms_full_size_vs_oracle():
    """131 072 anchors (256x256x2), many candidates, more than nms_top survivors of the filters."""
    from heal_amd import ops
    rng = np.random.default_rng(4)
    H = W = 256
    anchors = O.generate_anchor_box(PP_RANGE, 0.4, 0.4, 512, 512, 3.9, 1.6, 1.56, [0, 90])
    cls = (rng.standard_normal((1, 2, H, W)) * 1.5 - 2.5).astype(np.float32)
    reg = (rng.standard_normal((1, 14, H, W)) * 0.2).astype(np.float32)
    dirp = rng.standard_normal((1, 4, H, W)).astype(np.float32)
    tfm = np.eye(4, dtype=np.float32)
    pred, score = ops.decode_nms(dev(cls), dev(reg), dev(dirp), dev(anchors.astype(np.float32)), 0.2, 0.7853, 2,
                                 0.15, tfm, PP_RANGE)
    rp, rs = O.post_process(cls, reg, dirp, anchors, 0.2, 0.7853, 2, 0.15, tfm, PP_RANGE)
    assert pred.shape == rp.shape
    np.testing.assert_allclose(score.cpu().numpy(), rs, rtol=1e-5, atol=1e-6)
    # box coordinates up to +-140 m: relative 2e-6 (a few fp32 ulps of the decode's exp / sin / cos), no absolute slack beyond
    # what a coordinate near zero needs
    np.testing.assert_allclose(pred.cpu().numpy(), rp, rtol=2e-6, atol=2e-5)
    # the survivor INDEX LIST: every device box is matched to the oracle's candidate table (anchor index per candidate) and the
    # resulting anchor indices, in output order, must be the oracle's survivors in its order (shape + scores alone
    # do not identify the survivors)
    cand, _, cand_idx = O.decode_candidates(cls, reg, dirp, anchors, 0.2, 0.7853, 2, tfm)
    want_idx = _survivor_anchor_indices(cand, cand_idx, rp)
    got_idx = _survivor_anchor_indices(cand, cand_idx, pred.cpu().numpy())
    assert len(set(got_idx.tolist())) == len(got_idx) and np.array_equal(got_idx, want_idx)
    # idempotence: NMS survivors do not suppress each other
    q = pred[:, :4, :2].contiguous()
    iou = ops.quad_iou(q, q).cpu().numpy()
    np.fill_diagonal(iou, 0)
    assert not (iou > 0.15).any()


@pytest.mark.parametrize("n_equal", [600, 9000])
def test_decode_nms_ties_and_many_candidates_vs_oracle(n_equal):
    """Exactly tied scores (a saturated head) below and above the single-block top-k capacity (4096): the order among equal
    scores is 'larger anchor index first' on both sides, and with 9000 tied candidates the radix select has to split a tie
    at the rank-1000 boundary by anchor index."""
    from heal_amd import ops
    rng = np.random.default_rng(n_equal)
    H = W = 128
    anchors = O.generate_anchor_box([-51.2, -51.2, -3, 51.2, 51.2, 1], 0.4, 0.4, 256, 256, 3.9, 1.6, 1.56, [0, 90])
    cls = np.full((1, 2, H, W), -9.0, np.float32)
    flat = cls.reshape(-1)
    flat[rng.choice(flat.size, n_equal, replace=False)] = 1.25            # one exactly repeated logit
    flat[rng.choice(flat.size, 200, replace=False)] = rng.uniform(1.0, 3.0, 200).astype(np.float32)
    reg = (rng.standard_normal((1, 14, H, W)) * 0.05).astype(np.float32)
    dirp = rng.standard_normal((1, 4, H, W)).astype(np.float32)
    tfm = np.eye(4, dtype=np.float32)
    rngb = [-51.2, -51.2, -3, 51.2, 51.2, 1]
    pred, score = ops.decode_nms(dev(cls), dev(reg), dev(dirp), dev(anchors.astype(np.float32)), 0.2, 0.7853, 2,
                                 0.15, tfm, rngb)
    rp, rs = O.post_process(cls, reg, dirp, anchors, 0.2, 0.7853, 2, 0.15, tfm, rngb)
    assert pred.shape == rp.shape, (pred.shape, rp.shape)
    np.testing.assert_allclose(score.cpu().numpy(), rs, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(pred.cpu().numpy(), rp, rtol=1e-3, atol=1e-3)


def test_decode_nms_nothing_above_threshold():
    from heal_amd import ops
    anchors = O.generate_anchor_box([-25.6, -25.6, -3, 25.6, 25.6, 1], 0.4, 0.4, 128, 128, 3.9, 1.6, 1.56, [0, 90])
    cls = np.full((1, 2, 64, 64), -9.0, np.float32)
    reg = np.zeros((1, 14, 64, 64), np.float32)
    pred, score = ops.decode_nms(dev(cls), dev(reg), None, dev(anchors.astype(np.float32)), 0.2, 0.7853, 2, 0.15,
                                 np.eye(4, dtype=np.float32), [-25.6, -25.6, -3, 25.6, 25.6, 1])
    assert pred is None and score is None


def test_ops_reject_cpu_tensors():
    from heal_amd import _capi, ops
    with pytest.raises(_capi.HealAmdError):
        ops.voxelize(torch.zeros(10, 4), PP_RANGE, [0.4, 0.4, 4], 32, 100)


# ---------------------------------------------------------------------------------------------- K4
def _cam_mats(cam):
    from heal_amd.opencood.models.heter_encoders import LiftSplatShoot
    t = {k: dev(v) for k, v in cam.items()}
    return LiftSplatShoot.camera_matrices(t["rots"], t["trans"], t["intrins"], t["post_rots"], t["post_trans"])


def _pool_close(got, want, rtol=1e-3, atol=1e-4, max_bad_cells=0, name="bev_pool"):
    """Per-cell sums must agree.  `max_bad_cells` is an ABSOLUTE number of BEV cells allowed to differ (0 against the
    reference's golden vector, whose geometry the kernel reproduces operation for operation; a stated handful against the
    numpy oracle, whose 3x3 products are evaluated in another order so that a point within one ulp of a cell edge may land
    in the neighbouring cell).  The count found is always recorded (tests/report.py) and printed on failure; the TOTAL per
    channel must be conserved either way."""
    from tests.report import note
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol)
    n_bad = int(bad.any(axis=1).sum())
    occupied = int((np.abs(want).sum(axis=1) > 0).sum())
    note(name, bad_cells=n_bad, occupied_cells=occupied, allowed=int(max_bad_cells),
         max_abs_err=float(np.abs(got - want).max()))
    assert n_bad <= max_bad_cells, f"{n_bad} of {occupied} occupied BEV cells differ (allowed: {max_bad_cells})"
    np.testing.assert_allclose(got.sum(axis=(2, 3)), want.sum(axis=(2, 3)), rtol=2e-3, atol=1e-2)


def test_bev_pool_matches_reference_golden(golden):
    from heal_amd import ops
    g = golden("lss")
    cam = {k[4:]: g[k] for k in g.files if k.startswith("cam_")}
    B, N = cam["trans"].shape[:2]
    out = ops.bev_pool(dev(g["depth_logit"]), dev(g["feat"]), dev(g["frustum"]), _cam_mats(cam), B, N,
                       g["dx"].tolist(), g["bx"].tolist(), g["nx"].tolist()).cpu().numpy()
    assert out.shape == g["pooled"].shape
    _pool_close(out, g["pooled"], max_bad_cells=0, name="bev_pool_reference_golden")


@pytest.mark.parametrize("n_agents,C,final_dim", [(2, 128, (384, 512)), (1, 128, (336, 448)), (1, 16, (64, 96))])
def test_bev_pool_full_size_vs_oracle(n_agents, C, final_dim):
    from heal_amd import ops, synth
    rng = np.random.default_rng(C + n_agents)
    fH, fW = final_dim[0] // 8, final_dim[1] // 8
    D, N = 48, 4
    frustum = O.create_frustum(list(final_dim), 8, [2, 50, 48], "LID")
    dx, bx, nx = O.gen_dx_bx([-51.2, 51.2, 0.4], [-51.2, 51.2, 0.4], [-10, 10, 20.0])
    rig = synth.camera_rig(0, N, final_dim[0], final_dim[1])
    cam = {k: np.tile(v[None], (n_agents,) + (1,) * v.ndim).astype(np.float32) for k, v in rig.items()}
    depth_logit = rng.standard_normal((n_agents * N, D, fH, fW)).astype(np.float32)
    feat = rng.standard_normal((n_agents * N, C, fH, fW)).astype(np.float32)
    out = ops.bev_pool(dev(depth_logit), dev(feat), dev(frustum), _cam_mats(cam), n_agents, N, dx.tolist(),
                       bx.tolist(), nx.tolist()).cpu().numpy()
    geom = O.lss_geometry(frustum, cam["rots"], cam["trans"], cam["intrins"], cam["post_rots"], cam["post_trans"])
    lifted = O.lift(depth_logit, feat)
    x = lifted.reshape(n_agents, N, C, D, fH, fW).transpose(0, 1, 3, 4, 5, 2)
    ref = O.bev_pool(geom, x, dx, bx, nx)
    assert out.shape == ref.shape == (n_agents, C, 256, 256)
    _pool_close(out, ref, max_bad_cells=0, name=f"bev_pool_full_size_{n_agents}_{C}_{final_dim[0]}")
    assert (out != 0).any(axis=1).sum() > 1000


def test_mask_points_then_voxelize_equals_reference_filters_then_oracle(golden):
    """heal_mask_points (pcd_utils.mask_ego_points + mask_points_by_range on the device, dropped points -> NaN) followed
    by K1 must equal the reference's host filters followed by the oracle voxeliser: bit exact, face-exact points and a
    NaN point included (tests/golden/pcd.npz, generated from the imported reference)."""
    from heal_amd import ops
    from heal_amd.opencood.utils import pcd_utils
    g = golden("pcd")
    rng = g["lidar_range"].tolist()
    pts = dev(g["points"])
    masked = pcd_utils.mask_points_by_range(pcd_utils.mask_ego_points(pts), rng)     # device path of the mirror
    assert masked.shape == pts.shape
    kept = ~torch.isnan(masked).any(dim=1)
    assert np.array_equal(masked[kept].cpu().numpy(), g["ego_range"])
    one = ops.mask_points(pts, rng, mask_ego=True)
    assert np.array_equal(one.cpu().numpy(), masked.cpu().numpy(), equal_nan=True)
    only = ops.mask_points(pts, rng, mask_ego=False)
    assert np.array_equal(only[~torch.isnan(only).any(dim=1)].cpu().numpy(), g["only_range"])
    inplace = pts.clone()
    ops.mask_points(inplace, rng, mask_ego=True, out=inplace)
    assert np.array_equal(inplace.cpu().numpy(), one.cpu().numpy(), equal_nan=True)
    for vs, P in (([0.4, 0.4, 4], 32), ([0.1, 0.1, 0.1], 5)):
        v, c, n = ops.voxelize(one, rng, vs, P, 70000)
        ov, oc, on = cref.voxelize(g["ego_range"], rng, vs, P, 70000, batch_idx=0)
        assert np.array_equal(c.cpu().numpy(), oc) and np.array_equal(n.cpu().numpy(), on)
        assert np.array_equal(v.cpu().numpy(), ov)


def _pitched_rig(final_dim, n_cams=4):
    """synth.camera_rig with every camera pitched / rolled (10..25 deg) and a resize + crop post-transform: the points
    of an image column then spread over several BEV cells (several runs per column, and runs that leave the grid)."""
    from heal_amd import synth
    rig = synth.camera_rig(0, n_cams, final_dim[0], final_dim[1])
    for k in range(n_cams):
        a, r = np.deg2rad(10.0 + 5.0 * k), np.deg2rad(4.0 * k - 6.0)
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
        rig["rots"][k] = (rig["rots"][k].astype(np.float64) @ Rx @ Rz).astype(np.float32)
        rig["post_rots"][k] = np.diag([0.9, 0.9, 1.0]).astype(np.float32)
        rig["post_trans"][k] = np.array([-7.0 + k, 3.0, 0.0], np.float32)
    return rig


@pytest.mark.parametrize("path", ["fused", "sorted"])
def test_bev_pool_pitched_cameras_vs_oracle(path, monkeypatch):
    """K4 with cameras that are NOT level: image columns break into several runs, the case the level synthetic rig
    never produces (the fused path handles the column's main cell as a GEMM on the matrix cores and walks the rest; the
    sorted path is the bit-reproducible radix-sort pipeline)."""
    from heal_amd import ops
    monkeypatch.setenv("HEAL_LSS_PATH", path)
    final_dim, C, n_agents, D, N = (336, 448), 64, 2, 48, 4
    rng = np.random.default_rng(11)
    fH, fW = final_dim[0] // 8, final_dim[1] // 8
    frustum = O.create_frustum(list(final_dim), 8, [2, 50, 48], "LID")
    dx, bx, nx = O.gen_dx_bx([-51.2, 51.2, 0.4], [-51.2, 51.2, 0.4], [-10, 10, 20.0])
    rig = _pitched_rig(final_dim, N)
    cam = {k: np.tile(v[None], (n_agents,) + (1,) * v.ndim).astype(np.float32) for k, v in rig.items()}
    depth_logit = rng.standard_normal((n_agents * N, D, fH, fW)).astype(np.float32)
    feat = rng.standard_normal((n_agents * N, C, fH, fW)).astype(np.float32)
    out = ops.bev_pool(dev(depth_logit), dev(feat), dev(frustum), _cam_mats(cam), n_agents, N, dx.tolist(),
                       bx.tolist(), nx.tolist()).cpu().numpy()
    geom = O.lss_geometry(frustum, cam["rots"], cam["trans"], cam["intrins"], cam["post_rots"], cam["post_trans"])
    # the case this test exists for: columns with more than one run
    idx = np.trunc((geom - (bx - dx / 2)) / dx).astype(np.int64)[0]            # [N,D,fH,fW,3]
    ok = ((idx >= 0) & (idx < nx)).all(-1)
    key = np.where(ok, idx[..., 1] * nx[0] + idx[..., 0], -1)
    runs = (key[:, :, 0] >= 0).sum() + ((key[:, :, 1:] != key[:, :, :-1]) & (key[:, :, 1:] >= 0)).sum()
    assert runs > 2 * N * D * fW, runs
    x = O.lift(depth_logit, feat).reshape(n_agents, N, C, D, fH, fW).transpose(0, 1, 3, 4, 5, 2)
    ref = O.bev_pool(geom, x, dx, bx, nx)
    _pool_close(out, ref, max_bad_cells=0, name=f"bev_pool_pitched_{path}")
    assert (out != 0).any(axis=1).sum() > 1000


# ---------------------------------------------------------------------------------------------- K3
def _random_sites(rng, n, shape, batch):
    D, H, W = shape
    lin = rng.choice(batch * D * H * W, size=n, replace=False)
    b, r = np.divmod(lin, D * H * W)
    z, r = np.divmod(r, H * W)
    y, x = np.divmod(r, W)
    return np.stack([b, z, y, x], 1).astype(np.int32)


def _dense_from(st):
    C = st.features.shape[1]
    D, H, W = st.spatial_shape
    return st.dense().cpu().numpy().reshape(st.batch_size, C, D, H, W)


def test_mean_vfe_vs_oracle():
    from heal_amd import ops
    rng = np.random.default_rng(0)
    v = rng.standard_normal((5000, 5, 4)).astype(np.float32)
    n = rng.integers(0, 6, 5000).astype(np.int32)
    v *= (np.arange(5)[None, :, None] < n[:, None, None])
    got = ops.mean_vfe(dev(v), dev(n)).cpu().numpy()
    np.testing.assert_allclose(got, O.mean_vfe(v, n), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("cin,cout,ksize,stride,padding,subm", [
    (4, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), True), (16, 32, (3, 3, 3), (2, 2, 2), (1, 1, 1), False),
    (64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True), (64, 64, (3, 3, 3), (2, 2, 2), (0, 1, 1), False),
    (64, 64, (3, 1, 1), (2, 1, 1), (0, 0, 0), False), (32, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), False)])
def test_sparse_conv_layer_vs_dense_oracle(cin, cout, ksize, stride, padding, subm):
    from heal_amd import ops
    rng = np.random.default_rng(cin * 7 + cout)
    shape, batch = (11, 24, 20), 2
    idx = _random_sites(rng, 1500, shape, batch)
    feats = rng.standard_normal((len(idx), cin)).astype(np.float32)
    K = int(np.prod(ksize))
    w = (rng.standard_normal(tuple(ksize) + (cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    g = rng.uniform(0.8, 1.2, cout).astype(np.float32); b = rng.normal(0, 0.1, cout).astype(np.float32)
    mu = rng.normal(0, 0.1, cout).astype(np.float32); var = rng.uniform(0.7, 1.3, cout).astype(np.float32)
    scale = (g / np.sqrt(var + np.float32(1e-3))).astype(np.float32); shift = (b - mu * scale).astype(np.float32)
    x = ops.SparseTensor.from_unsorted(dev(feats), dev(idx), shape, batch)
    # sites come back sorted by linear coordinate
    xi = x.indices.cpu().numpy().astype(np.int64)
    lin = ((xi[:, 0] * shape[0] + xi[:, 1]) * shape[1] + xi[:, 2]) * shape[2] + xi[:, 3]
    assert np.all(np.diff(lin) > 0)
    if subm:
        nbr = x.neighbors(x.indices, shape, ksize, (1, 1, 1), tuple(k // 2 for k in ksize))
        out = ops.SparseTensor(x.conv(nbr, dev(w.reshape(K, cin, cout)), dev(scale), dev(shift)), x.indices, shape, batch)
    else:
        oi, oshape, _ = x.out_sites(ksize, stride, padding)
        nbr = x.neighbors(oi, oshape, ksize, stride, padding)
        out = ops.SparseTensor(x.conv(nbr, dev(w.reshape(K, cin, cout)), dev(scale), dev(shift)), oi, oshape, batch)
    dense, mask = O.densify(feats, idx, shape, batch)
    ref, rmask = O.sparse_conv_dense(dense, mask, w, ksize, stride, padding, subm, g, b, mu, var)
    got = _dense_from(out)
    assert got.shape == tuple(ref.shape)
    # active-site set is an index computation: exact
    om = np.zeros(rmask.shape, bool)
    oidx = out.indices.cpu().numpy()
    om[oidx[:, 0], 0, oidx[:, 1], oidx[:, 2], oidx[:, 3]] = True
    assert np.array_equal(om, rmask.numpy() > 0)
    np.testing.assert_allclose(got, ref.numpy(), rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("n,cin,cout,H,W,ksplit", [(4, 432, 512, 24, 32, None), (2, 128, 64, 16, 32, 4), (1, 72, 64, 10, 14, 3),
                                                  (3, 256, 128, 8, 16, 32)])
def test_conv3x3_winograd_split_k_equals_one_launch(n, cin, cout, H, W, ksplit, monkeypatch):
    """heal_conv3x3_winograd_splitk (round 6: small maps with a deep reduction, the camera trunk's Up block, lss_submodule.py:33-50): K
    chunks split over blocks, partial OUTPUTS (the output transform is linear) added in split order, then bias + residual + ReLU.
    Against the single launch (another order of the fp32 sums: 1e-5) and fp64 torch; two runs bit-identical; the default policy picks a
    split for the 4 x 24 x 32 layer and none for a grid that already fills the chip."""
    from heal_amd import ops
    g = torch.Generator(device="cpu").manual_seed(n * 1000 + cin)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    r = torch.randn((n, cout, H, W), generator=g).cuda()
    monkeypatch.setenv("HEAL_C3_ALGO", "winograd")
    monkeypatch.setenv("HEAL_C3_KSPLIT", "1")
    one = ops.conv3x3(x, w, b, r, True, 1)
    if ksplit is None:
        monkeypatch.delenv("HEAL_C3_KSPLIT")
        waves = ops.conv3x3_winograd_waves(n, cout, H, W)
        assert ops.conv3x3_winograd_ksplit(n, cin, cout, H, W, waves) >= 2
        assert ops.conv3x3_winograd_ksplit(4, 512, 512, 48, 64, ops.conv3x3_winograd_waves(4, 512, 48, 64)) == 1
    else:
        monkeypatch.setenv("HEAL_C3_KSPLIT", str(ksplit))
    got = ops.conv3x3(x, w, b, r, True, 1)
    assert torch.equal(got, ops.conv3x3(x, w, b, r, True, 1))
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), 1, 1) + r.double())
    scale = float(ref.abs().max())
    assert float((got - one).abs().max()) < 1e-5 * scale
    assert float((got.double() - ref).abs().max()) < 1e-4 * scale


@pytest.mark.parametrize("slot_sites", [64, 128])
@pytest.mark.parametrize("cin,cout,stride,padding,subm", [
    (4, 16, (1, 1, 1), (1, 1, 1), True), (16, 16, (1, 1, 1), (1, 1, 1), True), (16, 32, (2, 2, 2), (1, 1, 1), False),
    (32, 32, (1, 1, 1), (1, 1, 1), True)])
def test_sparse_conv_on_pair_tiles_vs_dense_oracle(cin, cout, stride, padding, subm, slot_sites, monkeypatch):
    """Round 6, the c_in <= 16 layers of VoxelBackBone8x (sparse_backbone_3d.py:48-62) on the pair-tile rulebook
    (heal_sp_neighbor_tiles + heal_sp_conv_tiles): the tiles decode to the neighbour table BIT FOR BIT (an index computation), the
    convolution matches the dense restatement, two runs are bit-identical (fixed summation order), and the device-count mode
    (capacity-sized buffers, live rows on the device) gives the same rows."""
    from heal_amd import ops
    if slot_sites != 64:
        _need_experimental()      # 128-site slots: a measured alternative, built only with HEAL_BUILD_EXPERIMENTAL=1
    monkeypatch.setenv("HEAL_SP_SLOT_SITES", str(slot_sites))
    rng = np.random.default_rng(cin * 11 + cout + slot_sites)
    shape, batch, ksize = (11, 24, 20), 2, (3, 3, 3)
    idx = _random_sites(rng, 1500, shape, batch)
    feats = rng.standard_normal((len(idx), cin)).astype(np.float32)
    w = (rng.standard_normal(ksize + (cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    g = rng.uniform(0.8, 1.2, cout).astype(np.float32); b = rng.normal(0, 0.1, cout).astype(np.float32)
    mu = rng.normal(0, 0.1, cout).astype(np.float32); var = rng.uniform(0.7, 1.3, cout).astype(np.float32)
    scale = (g / np.sqrt(var + np.float32(1e-3))).astype(np.float32); shift = (b - mu * scale).astype(np.float32)
    wd, sc, sh = dev(w.reshape(27, cin, cout)), dev(scale), dev(shift)

    def layer(x):
        if subm:
            oi, oshape, n_dev = x.indices, list(shape), x.n_dev
            st, pd = (1, 1, 1), (1, 1, 1)
        else:
            oi, oshape, n_dev, rank = x.out_sites_ex(ksize, stride, padding)
            st, pd = stride, padding
        assert x.tiles_ok(ksize, cin, cout)
        tiles = x.rulebook(oi, oshape, ksize, st, pd, cin, cout, n_out_dev=n_dev)
        assert isinstance(tiles, ops.PairTiles) and tiles.slot_sites == slot_sites
        nbr = x.neighbors(oi, oshape, ksize, st, pd, n_out_dev=n_dev)
        out = x.conv(tiles, wd, sc, sh, n_out_dev=n_dev)
        rows = int(n_dev.item()) if n_dev is not None else int(out.shape[0])   # rows behind the live count are never written
        assert torch.equal(out[:rows], x.conv(tiles, wd, sc, sh, n_out_dev=n_dev)[:rows])
        via_table = x.conv(nbr, wd, sc, sh, n_out_dev=n_dev)
        return oi, oshape, n_dev, tiles, nbr, out, via_table

    x = ops.SparseTensor.from_unsorted(dev(feats), dev(idx), shape, batch)
    oi, oshape, _, tiles, nbr, out, via_table = layer(x)
    assert torch.equal(tiles.to_neighbors(), nbr)
    dense, mask = O.densify(feats, idx, shape, batch)
    ref, rmask = O.sparse_conv_dense(dense, mask, w, ksize, stride if not subm else (1, 1, 1), padding, subm, g, b, mu, var)
    got = _dense_from(ops.SparseTensor(out, oi, oshape, batch))
    np.testing.assert_allclose(got, ref.numpy(), rtol=1e-3, atol=1e-4)
    # against the neighbour-table kernel: the same products, another order of the fp32 sums
    assert float((out - via_table).abs().max()) < 1e-5 * float(via_table.abs().max() + 1)
    # device-count mode: capacity 2 x the rows, the live count on the device
    n = len(idx)
    fpad = np.concatenate([feats, np.full((77, cin), 7.0, np.float32)])    # padding rows behind the live ones
    ipad = np.concatenate([idx, np.full((77, 4), 3, np.int32)]); ipad[n:, 0] = 0
    xd = ops.SparseTensor.from_unsorted(dev(fpad), dev(ipad), shape, batch, n_dev=torch.tensor([n], dtype=torch.int32).cuda())
    oi_d, _, n_dev, tiles_d, nbr_d, out_d, _ = layer(xd)
    live = int(out.shape[0])
    assert n_dev is None or int(n_dev.item()) == live
    assert torch.equal(tiles_d.to_neighbors()[:live], nbr[:live]) and torch.equal(out_d[:live], out)


def test_second_encoder_vs_dense_oracle():
    """The whole VoxelBackBone8x + HeightCompression on a reduced grid against the dense restatement."""
    from heal_amd.opencood.models.heter_encoders import SECOND
    from tests.golden.detfill import fill_module
    from heal_amd import synth
    rng_range = [-6.4, -6.4, -3, 6.4, 6.4, 1]  # 128 x 128 x 40 voxels of 0.1 m -> sparse shape [41,128,128]
    args = {"voxel_size": [0.1, 0.1, 0.1], "lidar_range": rng_range, "mean_vfe": {"num_point_features": 4},
            "spconv": {"num_features_in": 4, "num_features_out": 64}, "map2bev": {"feature_num": 128}}
    enc = fill_module(SECOND(args)).cuda().eval()
    pts = synth.lidar_frame(5)
    pts = pts[(np.abs(pts[:, 0]) < 7) & (np.abs(pts[:, 1]) < 7)]
    vs, cs, ns = [], [], []
    for b in range(2):
        v, c, n = cref.voxelize(pts[b::2], rng_range, [0.1, 0.1, 0.1], 5, 70000, batch_idx=b)
        vs.append(v); cs.append(c); ns.append(n)
    v, c, n = np.concatenate(vs), np.concatenate(cs), np.concatenate(ns)
    assert len(n) > 2000
    with torch.no_grad():
        got = enc({"inputs_m3": {"voxel_features": dev(v), "voxel_coords": dev(c), "voxel_num_points": dev(n)}},
                  "m3").cpu().numpy()
    sd = {k: t.cpu().numpy() for k, t in enc.state_dict().items()}
    ref = O.second_backbone(sd, "spconv_block.", O.mean_vfe(v, n), c, [41, 128, 128], 2)
    assert got.shape == ref.shape == (2, 128, 16, 16)
    # no separate "same non-zero mask" allowance: a wrong active site shows up as an O(1) value against a zero, which the
    # absolute tolerance below catches; post-ReLU values within 2e-4 of zero are the only ones that may differ in sign
    from tests.report import note
    note("second_encoder_vs_dense_oracle", nonzero_mask_mismatch=int(((got != 0) != (ref != 0)).sum()),
         max_abs_err=float(np.abs(got - ref).max()), ref_abs_max=float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-4)
    # the device point-cloud path gives the same result as the voxel path
    with torch.no_grad():
        got2 = enc({"inputs_m3": {"points": [dev(pts[0::2]), dev(pts[1::2])]}}, "m3").cpu().numpy()
    np.testing.assert_array_equal(got2, got)


def test_sparse_device_counts_and_capacity_overflow_report():
    """No-host-sync mode of the sparse family: capacity-sized buffers + device row counts give the exact-size result;
    a strided layer that activates more sites than its capacity bound (isolated voxels dilate 8x) is reported."""
    from heal_amd import ops
    rng = np.random.default_rng(0)
    shape = [9, 32, 32]
    # dense-ish blob: N_out < N_in
    zz, yy, xx = np.meshgrid(np.arange(1, 7), np.arange(4, 20), np.arange(4, 20), indexing="ij")
    idx = np.stack([np.zeros(zz.size), zz.ravel(), yy.ravel(), xx.ravel()], 1).astype(np.int32)
    idx = idx[rng.permutation(len(idx))[:900]]
    feats = rng.standard_normal((len(idx), 16)).astype(np.float32)
    cap = len(idx) + 77  # padding rows behind the live ones
    fpad = np.concatenate([feats, np.full((77, 16), 7.0, np.float32)])
    ipad = np.concatenate([idx, np.full((77, 4), 3, np.int32)])
    n_dev = torch.tensor([len(idx)], dtype=torch.int32).cuda()
    exact = ops.SparseTensor.from_unsorted(dev(feats), dev(idx), shape, 1)
    lazy = ops.SparseTensor.from_unsorted(dev(fpad), dev(ipad), shape, 1, n_dev=n_dev)
    n = len(idx)
    assert torch.equal(lazy.indices[:n], exact.indices) and torch.equal(lazy.features[:n], exact.features)
    k, st, pd = (3, 3, 3), (2, 2, 2), (1, 1, 1)
    oi, osh, _ = exact.out_sites(k, st, pd)
    oj, osh2, n_out_dev = lazy.out_sites(k, st, pd)
    m = int(n_out_dev.item())
    assert osh == osh2 and m == oi.shape[0] and torch.equal(oj[:m], oi) and not lazy.overflow()
    w = torch.randn((27, 16, 32)).cuda(); sc = torch.ones(32).cuda(); sh = torch.zeros(32).cuda()
    a = exact.conv(exact.neighbors(oi, osh, k, st, pd), w, sc, sh)
    b = lazy.conv(lazy.neighbors(oj, osh2, k, st, pd, n_out_dev=n_out_dev), w, sc, sh, n_out_dev=n_out_dev)
    assert torch.equal(b[:m], a)
    # isolated voxels on odd coordinates: each activates 8 output sites -> exceeds the capacity bound
    iso = np.array([[0, z, y, x] for z in (1, 5) for y in range(1, 30, 4) for x in range(1, 30, 4)], np.int32)
    t = ops.SparseTensor.from_unsorted(dev(np.ones((len(iso), 4), np.float32)), dev(iso), shape, 1,
                                       n_dev=torch.tensor([len(iso)], dtype=torch.int32).cuda())
    ops.verify_sparse_capacity()          # everything recorded so far stayed within capacity: no error, list cleared
    _, _, cnt = t.out_sites(k, st, pd)
    assert int(cnt.item()) == 8 * len(iso) and t.overflow()
    # ... and the violation reaches the next host synchronisation of the path as an exception, not as silently dropped sites
    with pytest.raises(Exception, match="more than its capacity"):
        ops.verify_sparse_capacity()
    assert not ops.take_sparse_checks()   # verified checks are consumed


# ---------------------------------------------------------------------------------------------- K7
@pytest.mark.parametrize("C,stride,H,W", [(128, 1, 64, 96), (256, 2, 64, 64), (512, 1, 32, 32), (512, 2, 34, 30),
                                          (128, 2, 37, 41), (256, 1, 40, 56), (512, 1, 19, 20), (512, 1, 19, 21), (256, 1, 128, 128),
                                          (128, 1, 50, 44), (128, 1, 16, 32), (256, 1, 17, 36), (128, 1, 3, 4),
                                          (256, 2, 128, 128), (128, 2, 33, 40), (256, 2, 17, 8), (128, 2, 64, 48)])
@pytest.mark.parametrize("mfma", ["1", "8", "0", "16"])
def test_grouped_conv3x3_vs_torch(C, stride, H, W, mfma, monkeypatch):
    """32-group 3x3: the vector-ALU stencil and the matrix-core kernels (stride 1, W % 4 == 0: 16 channels per group on 16x16x4
    MFMA tiles (HEAL_GCONV_MFMA=16, or =8 which also pairs groups of 8 into block-diagonal 16-channel super-groups); 4, 8 and 16
    per group at stride 1 and 2 on the 16-block 4x4x1 MFMA (=1, production); =0 forces the stencil) against torch fp64."""
    from heal_amd import ops
    monkeypatch.setenv("HEAL_GCONV_MFMA", mfma)
    g = torch.Generator().manual_seed(C + stride)
    x = torch.randn((2, C, H, W), generator=g).cuda()
    w = (torch.randn((C, C // 32, 3, 3), generator=g) * 0.2).cuda()
    b = torch.randn((C,), generator=g).cuda()
    got = ops.grouped_conv3x3(x, w, b, 32, stride, relu=True)
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride, 1, 1, 32)).float()
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-5)
    got2 = ops.grouped_conv3x3(x, w, None, 32, stride, relu=False)
    ref2 = torch.nn.functional.conv2d(x.double(), w.double(), None, stride, 1, 1, 32).float()
    np.testing.assert_allclose(got2.cpu().numpy(), ref2.cpu().numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("n,C,H,W", [(5, 64, 64, 64), (2, 128, 20, 14), (1, 256, 7, 12), (3, 3, 2, 2)])
def test_channel_dot_vs_torch(n, C, H, W):
    """Occupancy head (Conv2d(C, 1, 1)) as a channel dot product, against torch fp64."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn((n, C, H, W), generator=g).cuda()
    w = (torch.randn((1, C, 1, 1), generator=g) / C ** 0.5).cuda()
    b = torch.randn((1,), generator=g).cuda()
    for bias in (b, None):
        got = ops.channel_dot(x, w, bias)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), None if bias is None else bias.double())
        assert got.shape == ref.shape
        assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-5


def test_bias_act_vs_torch():
    from heal_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 20, 12, 8), generator=g).cuda()
    r = torch.randn((3, 20, 12, 8), generator=g).cuda()
    b = torch.randn((20,), generator=g).cuda()
    for bias, res, relu in ((b, r, True), (b, None, True), (None, r, False), (b, None, False)):
        y = x.clone()
        ops.bias_act_(y, bias, res, relu)
        ref = x + (bias.view(1, -1, 1, 1) if bias is not None else 0) + (res if res is not None else 0)
        ref = torch.relu(ref) if relu else ref
        np.testing.assert_array_equal(y.cpu().numpy(), ref.cpu().numpy())


@pytest.mark.parametrize("C,H,W", [(64, 32, 48), (128, 24, 24), (256, 16, 16), (64, 13, 21), (256, 7, 10), (128, 9, 8)])
def test_fused_resnext_bottleneck_vs_torch(C, H, W):
    _need_experimental()
    """K7b against the block it fuses, evaluated in fp64 by torch (resblock.py:100-122 with folded BN)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn((2, C, H, W), generator=g).cuda()
    w1 = (torch.randn((2 * C, C), generator=g) / C ** 0.5).cuda(); b1 = (torch.randn((2 * C,), generator=g) * 0.1).cuda()
    w2 = (torch.randn((2 * C, 2 * C // 32, 3, 3), generator=g) / (9 * 2 * C / 32) ** 0.5).cuda()
    b2 = (torch.randn((2 * C,), generator=g) * 0.1).cuda()
    w3 = (torch.randn((C, 2 * C), generator=g) / (2 * C) ** 0.5).cuda(); b3 = (torch.randn((C,), generator=g) * 0.1).cuda()
    got = ops.resnext_bottleneck(x, ops.mfma_a_fragments(w1), b1, w2, b2, ops.mfma_a_fragments(w3), b3)
    F = torch.nn.functional
    xd = x.double()
    t = torch.relu(F.conv2d(xd, w1.double().view(2 * C, C, 1, 1), b1.double()))
    t = torch.relu(F.conv2d(t, w2.double(), b2.double(), 1, 1, 1, 32))
    ref = torch.relu(F.conv2d(t, w3.double().view(C, 2 * C, 1, 1), b3.double()) + xd).float()
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-5)


def test_upsample2x_bilinear_vs_torch():
    from heal_amd import ops
    g = torch.Generator().manual_seed(0)
    for shape in ((2, 5, 12, 16), (1, 3, 1, 7), (4, 8, 24, 32)):
        x = torch.randn(shape, generator=g).cuda()
        ref = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        np.testing.assert_allclose(ops.upsample2x_bilinear(x).cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("k,stride,pad", [(3, 1, (1, 1, 1, 1)), (3, 2, (0, 1, 0, 1)), (5, 1, (2, 2, 2, 2)), (5, 2, (1, 2, 1, 2))])
def test_depthwise_conv_vs_torch(k, stride, pad):
    from heal_amd import ops
    g = torch.Generator().manual_seed(k * 10 + stride)
    x = torch.randn((3, 48, 24, 37), generator=g).cuda()
    w = torch.randn((48, 1, k, k), generator=g).cuda() * 0.3
    b = torch.randn((48,), generator=g).cuda()
    F = torch.nn.functional
    ref = F.silu(F.conv2d(F.pad(x, pad).double(), w.double(), b.double(), stride, 0, 1, 48)).float()
    got = ops.depthwise_conv(x, w, b, stride, pad, "silu")
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("n,cin,cout,H,W,act,with_res,with_bias", [
    (2, 64, 128, 32, 32, 1, False, True), (1, 128, 64, 16, 24, 1, True, True), (3, 256, 512, 8, 8, 0, False, False),
    (1, 512, 256, 12, 16, 1, True, True), (2, 32, 64, 6, 10, 2, False, True), (1, 64, 192, 50, 2, 0, True, False)])
def test_conv1x1_fused_vs_torch(n, cin, cout, H, W, act, with_res, with_bias):
    """K7c: y = act(W x + b (+ res)).  fp32 MFMA accumulates in a different order than the library GEMM:
    1e-4 relative to the output scale (the north-star tolerance for features is 1e-3)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda() if with_bias else None
    r = torch.randn((n, cout, H, W), generator=g).cuda() if with_res else None
    got = ops.conv1x1(x, w, b, r, act)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), None if b is None else b.double())
    if r is not None:
        ref = ref + r.double()
    ref = torch.relu(ref) if act == 1 else torch.nn.functional.silu(ref) if act == 2 else ref
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-4, err
    # the fragment cache must notice an in-place weight update
    w.mul_(2.0)
    got2 = ops.conv1x1(x, w, None, None, 0)
    ref2 = torch.nn.functional.conv2d(x.double(), w.double())
    assert float((got2.double() - ref2).abs().max() / ref2.abs().max()) < 1e-4


_C3_SHAPES = [
    (1, 384, 256, 64, 64, 1, False, True),      # shrink header shape (channels), reduced map
    (3, 64, 64, 40, 48, 1, True, True),         # BasicBlock conv2 + identity
    (2, 64, 64, 64, 64, 2, False, True),        # BasicBlock conv1, stride 2
    (1, 128, 64, 33, 47, 2, False, True),       # odd map, stride 2 (camera backbone 128 -> 64)
    (4, 552, 512, 12, 16, 1, False, True),      # Up of the Lift-Splat encoder
    (1, 67, 20, 19, 21, 1, True, False),        # ragged everything: Cin % 8 != 0, Cout % 64 != 0, map % 16 != 0
    (2, 3, 32, 24, 40, 2, False, False),        # image stem sized channels
    (1, 16, 130, 8, 8, 1, False, True),         # map smaller than a tile, Cout spills into a third 64-block
]
# Winograd F(2x2,3x3) is the stride-1 formulation (8- and 4-wave blocks); the implicit GEMM takes every shape
_C3_CASES = [sh + (algo,) for sh in _C3_SHAPES for algo in ("winograd", "winograd8", "winograd4", "direct") if algo == "direct" or sh[5] == 1]
# round 5: chunks of 16 input channels (heal_conv3x3_winograd_kc; measured 4-13 % slower, opt-in HEAL_WG_KC=16) where it applies
_C3_CASES += [sh + ("winograd8kc16",) for sh in _C3_SHAPES if sh[5] == 1 and sh[1] % 16 == 0]


@pytest.mark.parametrize("n,cin,cout,H,W,stride,res,relu,algo", _C3_CASES)
def test_conv3x3_mfma_vs_torch(n, cin, cout, H, W, stride, res, relu, algo, monkeypatch):
    """heal_conv3x3 (implicit GEMM) / heal_conv3x3_winograd (F(2x2,3x3), stride 1) on fp32 MFMA with fused bias / residual /
    ReLU against torch's fp64 convolution: 1e-4 relative to the output scale (fp32 accumulation order and, for Winograd, the
    transform's rounding sequence differ; the north-star tolerance for features is 1e-3)."""
    from heal_amd import ops
    if algo in ("winograd4", "winograd8kc16"):
        _need_experimental()
    kc16 = algo.endswith("kc16")
    algo = algo[:-4] if kc16 else algo
    monkeypatch.setenv("HEAL_WG_KC", "16" if kc16 else "8")
    monkeypatch.setenv("HEAL_C3_ALGO", algo if algo == "winograd4" else algo.rstrip("8"))   # winograd4: F(4x4,3x3)
    monkeypatch.setenv("HEAL_WG_WAVES", "8" if algo.endswith("8") else "4")   # 16x16- or 8x16-pixel Winograd blocks
    g = torch.Generator().manual_seed(cin * 31 + cout + H)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn((n, cout, Ho, Wo), generator=g).cuda() if res else None
    got = ops.conv3x3(x, w, b, r, relu, stride)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride, 1)
    if r is not None:
        ref = ref + r.double()
    if relu:
        ref = torch.relu(ref)
    assert got.shape == ref.shape
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-4, err
    # no bias, and the fragment cache must notice an in-place weight update
    w.mul_(-0.5)
    got2 = ops.conv3x3(x, w, None, None, False, stride)
    ref2 = torch.nn.functional.conv2d(x.double(), w.double(), None, stride, 1)
    assert float((got2.double() - ref2).abs().max() / ref2.abs().max()) < 1e-4


@pytest.mark.parametrize("algo", ["winograd", "direct"])
def test_conv3x3_full_size_properties(algo, monkeypatch):
    """BASELINE-size shrink header convolution (384 -> 256 at 256 x 256): linearity in the input and a delta kernel (centre tap
    = identity on the first 256 channels; exact for the implicit GEMM, to rounding for Winograd) -- properties that do not
    need a reference at this size."""
    from heal_amd import ops
    monkeypatch.setenv("HEAL_C3_ALGO", algo)
    exact = algo == "direct"
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn((1, 384, 256, 256), generator=g).cuda()
    x2 = torch.randn((1, 384, 256, 256), generator=g).cuda()
    w = (torch.randn((256, 384, 3, 3), generator=g) / (9 * 384) ** 0.5).cuda()
    y1, y2, y12 = ops.conv3x3(x1, w), ops.conv3x3(x2, w), ops.conv3x3(x1 + 2.0 * x2, w)
    err = float((y12 - (y1 + 2.0 * y2)).abs().max() / y12.abs().max())
    assert err < 1e-4, err
    wd = torch.zeros((256, 384, 3, 3)).cuda()
    wd[torch.arange(256), torch.arange(256), 1, 1] = 1.0
    got = ops.conv3x3(x1, wd)
    assert torch.equal(got, x1[:, :256]) if exact else float((got - x1[:, :256]).abs().max()) < 1e-5
    # shifted delta: output = input shifted by one pixel with a zero border (padding 1)
    ws = torch.zeros((256, 384, 3, 3)).cuda()
    ws[torch.arange(256), torch.arange(256), 0, 2] = 1.0     # y[o] = x[o + (-1, +1)]
    want = torch.zeros_like(x1[:, :256])
    want[:, :, 1:, :-1] = x1[:, :256, :-1, 1:]
    got = ops.conv3x3(x1, ws)
    assert torch.equal(got, want) if exact else float((got - want).abs().max()) < 1e-5


@pytest.mark.parametrize("n,cin,cout,H,W,act", [(4, 512, 176, 48, 64, 0), (4, 512, 176, 42, 56, 0), (2, 64, 20, 12, 16, 1),
                                                (1, 96, 68, 10, 12, 2)])
def test_conv1x1_pixel_major_output_equals_nchw(n, cin, cout, H, W, act):
    """The pixel-major epilogue (fused image_head | depth_head of CamEncode -> K4's input layout) writes the same numbers
    as the NCHW epilogue, permuted: identical accumulators, identical bias / activation arithmetic -> bit equal."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cout)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    a = ops.conv1x1(x, w, b, None, act)
    pm = ops.conv1x1(x, w, b, None, act, pixel_major=True)
    assert tuple(pm.shape) == (n, H * W, cout)
    assert torch.equal(pm.view(n, H, W, cout).permute(0, 3, 1, 2), a)
    nb = ops.conv1x1(x, w, None, None, act, pixel_major=True)
    assert torch.equal(nb.view(n, H, W, cout).permute(0, 3, 1, 2), ops.conv1x1(x, w, None, None, act))


def _pm_ws_views(ws, n_cells, C):
    """(state words, flags[2], rows[2]) views of a heal_bev_pool_pm workspace (carve_pm, csrc/bev_pool.hip)."""
    al = lambda n: (n + 255) // 256 * 256
    words = ws.view(torch.int32)
    off = 256
    flags, rows = [], []
    for _ in range(2):
        flags.append(ws[off:off + n_cells * 4].view(torch.int32)); off += al(n_cells * 4)
    for _ in range(2):
        rows.append(ws[off:off + n_cells * C * 4].view(torch.float32).view(n_cells, C)); off += al(n_cells * C * 4)
    return words, flags, rows


def test_bev_pool_pm_zeroed_workspace_is_self_cleaning_and_repeatable():
    """heal_bev_pool_pm never memsets: calls alternate between the two (rows, flags) halves of the workspace, cells are tagged
    by generation, and every scatter zeroes -- as tail work of its own launch -- the rows its predecessor tagged in the other
    half.  Calls on different inputs interleaved (dense scene, empty scene: every point out of range, dense again) must each
    equal a fresh evaluation; after call g the half g & 1 holds exactly the pooled rows and the other half is all zero."""
    from heal_amd import ops, synth
    rng = np.random.default_rng(5)
    final_dim, C, D, N = (96, 128), 32, 48, 4
    fH, fW = final_dim[0] // 8, final_dim[1] // 8
    frustum = O.create_frustum(list(final_dim), 8, [2, 50, 48], "LID")
    dx, bx, nx = O.gen_dx_bx([-51.2, 51.2, 0.4], [-51.2, 51.2, 0.4], [-10, 10, 20.0])
    rig = synth.camera_rig(0, N, final_dim[0], final_dim[1])
    n_cells = int(nx[0] * nx[1] * nx[2])
    gen0 = None
    for trial, shift in enumerate((0.0, 1e6, 0.0, 3.0, 0.0)):
        cam = {k: v[None].astype(np.float32).copy() for k, v in rig.items()}
        cam["trans"][..., 0] += shift           # 1e6: the whole frustum leaves the grid -> nothing is touched
        dl = rng.standard_normal((N, D, fH, fW)).astype(np.float32)
        ft = rng.standard_normal((N, C, fH, fW)).astype(np.float32)
        out = ops.bev_pool(dev(dl), dev(ft), dev(frustum), _cam_mats(cam), 1, N, dx.tolist(), bx.tolist(), nx.tolist())
        geom = O.lss_geometry(frustum, cam["rots"], cam["trans"], cam["intrins"], cam["post_rots"], cam["post_trans"])
        x = O.lift(dl, ft).reshape(1, N, C, D, fH, fW).transpose(0, 1, 3, 4, 5, 2)
        ref = O.bev_pool(geom, x, dx, bx, nx)
        _pool_close(out.cpu().numpy(), ref, max_bad_cells=0, name=f"bev_pool_pm_repeat_{trial}")
        if shift == 1e6:
            assert float(out.abs().max()) == 0.0
        ws = ops._WS[(("bev_pool_pm", 1, C, int(nx[0]), int(nx[1]), int(nx[2])), 0, torch.cuda.current_stream().cuda_stream)]
        words, flags, rows = _pm_ws_views(ws, n_cells, C)
        gen = int(words[0].item())
        gen0 = gen - trial if gen0 is None else gen0
        assert gen == gen0 + trial, (gen, gen0, trial)         # every call advances the generation by one
        assert int(words[1].item()) == gen                     # tag published by the scatter = generation adopted by the consumer
        assert float(rows[(gen & 1) ^ 1].abs().max()) == 0.0   # the previous call's rows were zeroed by this call's scatter
        tagged = flags[gen & 1] == gen
        assert float(rows[gen & 1][~tagged].abs().max() if (~tagged).any() else 0.0) == 0.0   # only tagged cells hold sums
        want = torch.from_numpy(ref[0].reshape(C, -1).T.copy()).cuda()                       # [cells, C]
        assert int(tagged.sum()) >= int((want.abs().sum(1) > 0).sum())
        assert torch.allclose(rows[gen & 1], want, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("n_agents,C,final_dim,cam_bound", [(1, 128, (384, 512), 51.2), (2, 64, (96, 128), 25.6),
                                                           (1, 32, (64, 96), 51.2)])
def test_bev_stem_block_equals_dense_path(n_agents, C, final_dim, cam_bound):
    """heal_bev_stem_block (first BasicBlock of the camera ResNetBEVBackbone read straight from K4's sparse pixel-major map)
    against the dense hand-off: same scatter -> heal_bev_pool_emit -> plain PyTorch fp32 convolutions (3x3 stride 2 + ReLU,
    1x1 stride 2) of the dense [C, ny, nx] canvas.  fp32 MFMA both ways: 1e-4 of the output scale."""
    from heal_amd import ops, synth
    g = torch.Generator().manual_seed(C + n_agents)
    D, N = 48, 4
    fH, fW = final_dim[0] // 8, final_dim[1] // 8
    frustum = dev(O.create_frustum(list(final_dim), 8, [2, 50, 48], "LID"))
    dx, bx, nx = O.gen_dx_bx([-cam_bound, cam_bound, 0.4], [-cam_bound, cam_bound, 0.4], [-10, 10, 20.0])
    rig = synth.camera_rig(0, N, final_dim[0], final_dim[1])
    cam = {k: np.tile(v[None], (n_agents,) + (1,) * v.ndim).astype(np.float32) for k, v in rig.items()}
    mats = _cam_mats(cam)
    head = torch.randn((n_agents * N, fH * fW, C + D), generator=g).cuda()
    w1 = (torch.randn((64, C, 3, 3), generator=g) / (9 * C) ** 0.5).cuda()
    wd = (torch.randn((64, C, 1, 1), generator=g) / C ** 0.5).cuda()
    b1, bd = torch.randn((64,), generator=g).cuda(), torch.randn((64,), generator=g).cuda()
    args = (head, C, D, fH, fW, frustum, mats, n_agents, N, dx.tolist(), bx.tolist(), nx.tolist())
    dense = ops.bev_pool_pm(*args)
    want_main = torch.relu(torch.nn.functional.conv2d(dense, w1, b1, stride=2, padding=1))
    want_id = torch.nn.functional.conv2d(dense, wd, bd, stride=2)
    pooled = ops.bev_pool_pm(*args, pooled=True)
    assert isinstance(pooled, ops.PooledBEV) and pooled.shape == tuple(dense.shape)
    assert pooled.stem_supported(64, 64)
    wm, wdf = ops.stem_fragments(w1, wd)
    got_main, got_id = pooled.stem_block(wm, b1, wdf, bd)
    with pytest.raises(Exception):
        pooled.dense()                                   # one consumer per scatter
    assert (dense.abs().sum(1) > 0).sum() > 200
    for got, want in ((got_main, want_main), (got_id, want_id)):
        assert got.shape == want.shape
        err = float((got - want).abs().max() / want.abs().max())
        assert err < 1e-4, err
    # the same workspace keeps working for the dense consumer afterwards (generation hand-over by either consumer)
    again = ops.bev_pool_pm(*args)
    assert torch.allclose(again, dense, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("n,cin,cout,H,W", [(2, 48, 24, 8, 8), (4, 96, 16, 12, 16), (1, 16, 96, 24, 32), (3, 240, 40, 6, 8),
                                            (1, 256, 2, 16, 16), (2, 3, 5, 4, 4)])
def test_conv1x1_padded_shapes_gate_and_skip(n, cin, cout, H, W):
    """EfficientNet MBConv project stage: y = W (sigmoid(s) . x) + b (+ skip), channel counts that are not multiples
    of the 64 x 32 tile (zero-padded fragments, guarded rows)."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin + 1000 * cout)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    gate = torch.sigmoid(torch.randn((n, cin, 1, 1), generator=g)).cuda()
    skip = torch.randn((n, cout, H, W), generator=g).cuda()
    got = ops.conv1x1(x, w, b, skip, 0, in_scale=gate)
    ref = torch.nn.functional.conv2d((gate * x).double(), w.double(), b.double()) + skip.double()
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4
    got = ops.conv1x1(x, w, b, None, 2)
    ref = torch.nn.functional.silu(torch.nn.functional.conv2d(x.double(), w.double(), b.double()))
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4


def test_conv1x1_split_k_small_maps(monkeypatch):
    """Small maps with a deep reduction (the MBConv projections at 1/32 resolution): the K chunks split over several blocks
    + a deterministic reduce with the epilogue, against the single-pass kernel (same chunks, different summation tree: 1e-5)
    and torch fp64; gate, bias, residual, SiLU; split counts that do not divide the chunk count."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(11)
    for n, cin, cout, H, W, act in ((4, 1152, 192, 12, 16, 0), (4, 672, 112, 24, 32, 0), (2, 300, 70, 6, 10, 2), (1, 1152, 320, 12, 16, 1)):
        x = torch.randn((n, cin, H, W), generator=g).cuda()
        w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
        b = torch.randn((cout,), generator=g).cuda()
        gate = torch.sigmoid(torch.randn((n, cin, 1, 1), generator=g)).cuda()
        skip = torch.randn((n, cout, H, W), generator=g).cuda()
        monkeypatch.setenv("HEAL_C1_KSPLIT", "1")
        one = ops.conv1x1(x, w, b, skip, act, in_scale=gate)
        ref = torch.nn.functional.conv2d((gate * x).double(), w.double(), b.double()) + skip.double()
        ref = torch.relu(ref) if act == 1 else torch.nn.functional.silu(ref) if act == 2 else ref
        for ks in ("0auto", "2", "5", "7", "36"):
            if ks == "0auto":
                monkeypatch.delenv("HEAL_C1_KSPLIT")
                assert ops.conv1x1_ksplit(n, cin, cout, H * W) > 1 or cin < 256
            else:
                monkeypatch.setenv("HEAL_C1_KSPLIT", ks)
            got = ops.conv1x1(x, w, b, skip, act, in_scale=gate)
            assert float((got - one).abs().max() / one.abs().max()) < 1e-5, ks
            assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4, ks
            assert torch.equal(got, ops.conv1x1(x, w, b, skip, act, in_scale=gate))      # deterministic


@pytest.mark.parametrize("n,cin,cout,H,W", [(2, 64, 128, 32, 32), (1, 128, 256, 16, 24), (3, 64, 64, 9, 16)])
def test_conv1x1_stride2_vs_torch(n, cin, cout, H, W):
    """the 1x1 stride-2 `downsample` convolution of the residual blocks (resblock.py:160-165)"""
    from heal_amd import ops
    g = torch.Generator().manual_seed(H * W + cin)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    got = ops.conv1x1(x, w, b, None, 0, stride=2)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=2)
    assert got.shape == ref.shape
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4


def test_conv1x1_rejects_unsupported_shapes():
    from heal_amd import _capi, ops
    with pytest.raises(_capi.HealAmdError):  # H*W must be a multiple of 4 (16-byte rows)
        ops.conv1x1(torch.randn((1, 64, 3, 5)).cuda(), torch.randn((64, 64, 1, 1)).cuda())
    with pytest.raises(_capi.HealAmdError):  # Cin mismatch
        ops.conv1x1(torch.randn((1, 64, 8, 8)).cuda(), torch.randn((24, 32, 1, 1)).cuda())


@pytest.mark.parametrize("n,cin,cout,H,W,stride,pad,act", [
    (4, 3, 32, 96, 128, 2, (0, 1, 0, 1), "silu"), (2, 3, 32, 97, 63, 2, (1, 1, 1, 1), "silu"), (1, 16, 24, 20, 28, 1, (1, 1, 1, 1), "none"),
    (2, 5, 70, 18, 22, 2, (0, 1, 1, 1), "relu")])
def test_conv3x3_same_padding_vs_torch(n, cin, cout, H, W, stride, pad, act):
    """heal_conv3x3_same: TF-style "same" padding (only behind the map for a stride-2 convolution on an even map -- the
    EfficientNet stem), bias and SiLU / ReLU fused, against torch's F.pad + conv2d in fp64."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin * 31 + cout)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin ** 0.5)).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    F = torch.nn.functional
    ref = F.conv2d(F.pad(x.double(), pad), w.double(), b.double(), stride)
    ref = F.silu(ref) if act == "silu" else torch.relu(ref) if act == "relu" else ref
    got = ops.conv3x3_same(x, w, b, stride, pad, act)
    assert got.shape == ref.shape
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4


def test_se_gate_vs_torch():
    from heal_amd import ops
    g = torch.Generator().manual_seed(5)
    for n, C, S in ((4, 96, 4), (2, 1152, 48), (1, 32, 8), (3, 240, 10)):
        m = torch.randn((n, C, 1, 1), generator=g).cuda()
        w1 = (torch.randn((S, C, 1, 1), generator=g) / C ** 0.5).cuda(); b1 = torch.randn((S,), generator=g).cuda()
        w2 = (torch.randn((C, S, 1, 1), generator=g) / S ** 0.5).cuda(); b2 = torch.randn((C,), generator=g).cuda()
        ref = torch.sigmoid(torch.nn.functional.conv2d(torch.nn.functional.silu(
            torch.nn.functional.conv2d(m.double(), w1.double(), b1.double())), w2.double(), b2.double()))
        got = ops.se_gate(m, w1, b1, w2, b2)
        np.testing.assert_allclose(got.cpu().numpy(), ref.float().reshape(n, C).cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("k,stride,H,W", [(3, 1, 24, 32), (5, 2, 25, 37), (3, 2, 12, 16), (5, 1, 9, 70), (3, 1, 96, 128)])
def test_squeeze_folded_into_depthwise(k, stride, H, W):
    """MBConv: depthwise -> x.mean((2, 3)) -> SE gate.  The depthwise launch also stores the per-tile sums of its outputs,
    heal_se_gate adds the tiles up (fixed order: bit-reproducible) and scales them to the mean: same gate as the separate mean."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(k * 7 + stride)
    n, C, S = 4, 96, 4
    x = torch.randn((n, C, H, W), generator=g).cuda()
    w = (torch.randn((C, 1, k, k), generator=g) * 0.3).cuda()
    b = torch.randn((C,), generator=g).cuda()
    w1 = (torch.randn((S, C, 1, 1), generator=g) / C ** 0.5).cuda(); b1 = torch.randn((S,), generator=g).cuda()
    w2 = (torch.randn((C, S, 1, 1), generator=g) / S ** 0.5).cuda(); b2 = torch.randn((C,), generator=g).cuda()
    pad = (k // 2, k // 2, k // 2, k // 2)
    plain = ops.depthwise_conv(x, w, b, stride, pad, "silu")
    want = ops.se_gate(plain.mean((2, 3)), w1, b1, w2, b2)
    y, sums = ops.depthwise_conv(x, w, b, stride, pad, "silu", channel_sums=True)
    assert torch.equal(y, plain) and sums.shape == (n, C, ops.depthwise_tiles(plain.shape[2], plain.shape[3]))
    ref_sum = plain.double().sum((2, 3))
    assert float((sums.double().sum(2) - ref_sum).abs().max() / ref_sum.abs().max()) < 1e-5
    got = ops.se_gate(sums, w1, b1, w2, b2, scale=1.0 / (plain.shape[2] * plain.shape[3]), tiles=int(sums.shape[2]))
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-6)
    again = ops.se_gate(ops.depthwise_conv(x, w, b, stride, pad, "silu", channel_sums=True)[1], w1, b1, w2, b2,
                        scale=1.0 / (plain.shape[2] * plain.shape[3]), tiles=int(sums.shape[2]))
    assert torch.equal(got, again)                        # no atomics anywhere: bit-reproducible


def test_voxelize_collated_equals_per_agent():
    """collate_batch_list on the device: per-agent K1 calls writing into shared buffers at a device-side row offset."""
    from heal_amd import ops, synth
    pts = [torch.from_numpy(synth.lidar_frame(300 + k)).cuda()[: 20000 + 5000 * k].contiguous() for k in range(3)]
    pts.append(torch.zeros((0, 4)).cuda())  # an agent with no points
    R = [-102.4, -102.4, -3, 102.4, 102.4, 1]
    v, c, n, off = ops.voxelize_collated(pts, R, [0.4, 0.4, 4], 32, 70000)
    off = off.cpu().numpy()
    assert off[0] == 0 and off[-1] == off[-2]
    for b, p in enumerate(pts[:3]):
        vb, cb, nb = ops.voxelize(p, R, [0.4, 0.4, 4], 32, 70000, batch_idx=b)
        lo, hi = int(off[b]), int(off[b + 1])
        assert hi - lo == vb.shape[0]
        assert torch.equal(v[lo:hi], vb) and torch.equal(c[lo:hi], cb) and torch.equal(n[lo:hi], nb)
    # both caps inside a batch: max_voxels = 3000 truncates every agent at its own 3000th voxel, P = 2 truncates voxels
    v, c, n, off = ops.voxelize_collated(pts, R, [0.4, 0.4, 4], 2, 3000)
    off = off.cpu().numpy()
    for b, p in enumerate(pts[:3]):
        vb, cb, nb = ops.voxelize(p, R, [0.4, 0.4, 4], 2, 3000, batch_idx=b)
        lo, hi = int(off[b]), int(off[b + 1])
        assert hi - lo == vb.shape[0] == 3000
        assert torch.equal(v[lo:hi], vb) and torch.equal(c[lo:hi], cb) and torch.equal(n[lo:hi], nb)


def test_convnext_block_nchw_path_vs_reference_formula():
    """ConvNeXtBlock (feature_alignnet_modules.py:299-344): dwconv -> permute -> LayerNorm -> Linear -> GELU -> Linear
    -> gamma -> permute -> + input, evaluated by the reference formula in fp64 against the fused NCHW path."""
    from heal_amd.opencood.models.sub_modules.bev_blocks import ConvNeXtBlock
    from tests.golden.detfill import fill_module
    torch.manual_seed(0)
    blk = fill_module(ConvNeXtBlock(64, layer_scale_init_value=1e-6)).cuda().eval()
    with torch.no_grad():
        blk.gamma.copy_(torch.linspace(0.5, 1.5, 64))  # the 1e-6 init would hide the branch in the residual
        x = torch.randn((2, 64, 32, 48)).cuda()
        got = blk(x)
        d = blk.double()
        xd = x.double()
        t = d.dwconv(xd).permute(0, 2, 3, 1)
        t = torch.nn.functional.layer_norm(t, (64,), d.norm.weight, d.norm.bias, d.norm.eps)
        t = d.pwconv2(torch.nn.functional.gelu(d.pwconv1(t)))
        ref = xd + (d.gamma * t).permute(0, 3, 1, 2)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-4, err


def test_label_assign_and_generate_label_match_reference_golden(golden):
    """VoxelPostprocessor.generate_label against outputs of the reference's own implementation (with its
    Cython bbox_overlaps compiled from the .pyx, tests/golden/gen_golden.py::gen_label); the stand-up IoU of the kernel
    against the same compiled routine's values."""
    from heal_amd import configs, ops
    from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    g = golden("label")
    # IoU core: assignment by threshold only (no gt has a "best" anchor fight) -> compare with the golden IoU matrix
    iou = g["ov"]
    assigned, neg = ops.label_assign(dev(g["ov_boxes"]), dev(g["ov_query"]), 0.35, 0.2)
    above = iou > np.float32(0.35)
    want = np.where(above.any(1), above.argmax(1), -1)
    best = [int(iou[:, k].argmax()) for k in range(iou.shape[1]) if iou[:, k].max() > 0]
    for k in range(iou.shape[1]):
        a = int(iou[:, k].argmax())
        if iou[a, k] > 0 and want[a] < 0:
            want[a] = k
    wneg = (iou < np.float32(0.2)).all(1)
    wneg[best] = False
    np.testing.assert_array_equal(assigned.cpu().numpy(), want)
    np.testing.assert_array_equal(neg.cpu().numpy().astype(bool), wneg)
    # the whole label generation
    hy = configs.lidar_pyramid([-25.6, -25.6, -3, 25.6, 25.6, 1])
    post = VoxelPostprocessor(hy["postprocess"], train=True)
    for tag in "abc":
        lab = post.generate_label(gt_box_center=g[f"{tag}_gt"], anchors=g["anchors"], mask=g[f"{tag}_mask"])
        np.testing.assert_array_equal(lab["pos_equal_one"], g[f"{tag}_pos"])
        np.testing.assert_array_equal(lab["neg_equal_one"], g[f"{tag}_neg"])
        np.testing.assert_allclose(lab["targets"], g[f"{tag}_targets"], rtol=1e-6, atol=1e-7)
        assert lab["targets"].dtype == np.float64 and lab["pos_equal_one"].shape == g[f"{tag}_pos"].shape


@pytest.mark.parametrize("ws,heads,d,L,H,W", [(4, 16, 16, 3, 16, 24), (8, 8, 32, 2, 32, 16), (16, 4, 64, 2, 32, 48),
                                              (8, 4, 64, 1, 16, 16)])
def test_window_attention_vs_torch(ws, heads, d, L, H, W):
    """Fused window attention (mswin.py:46-80) against the explicit window re-layout + baddbmm + softmax + bmm in fp64."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(ws * 100 + d)
    qkv = torch.randn((L, H, W, 3 * heads * d), generator=g).cuda()
    T = ws * ws
    bias = torch.randn((T, T), generator=g).cuda()
    scale = d ** -0.5
    got = ops.window_attention(qkv, bias, heads, d, ws, scale)
    nh, nw = H // ws, W // ws
    q = qkv.double().view(L, nh, ws, nw, ws, 3, heads, d).permute(5, 0, 6, 1, 3, 2, 4, 7).reshape(3, -1, T, d)
    dots = q[0] @ q[1].transpose(1, 2) * scale + bias.double()
    ref = dots.softmax(-1) @ q[2]
    ref = ref.view(L, heads, nh, nw, ws, ws, d).permute(0, 2, 4, 3, 5, 1, 6).reshape(L, H, W, heads * d)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, err
    got0 = ops.window_attention(qkv, None, heads, d, ws, scale)
    ref0 = ((q[0] @ q[1].transpose(1, 2) * scale).softmax(-1) @ q[2]).view(L, heads, nh, nw, ws, ws, d) \
        .permute(0, 2, 4, 3, 5, 1, 6).reshape(L, H, W, heads * d)
    assert float((got0.double() - ref0).abs().max() / ref0.abs().max()) < 1e-5


@pytest.mark.parametrize("k,cin,cout,H,W", [(1, 64, 128, 32, 32), (2, 128, 128, 16, 24), (4, 256, 128, 8, 8)])
def test_deblock_transposed_conv_as_conv1x1_plus_shuffle(k, cin, cout, H, W):
    """base_bev_backbone_resnet.py:49-74 deblocks: ConvTranspose2d(kernel = stride) + BN(eps 1e-3) + ReLU, evaluated as
    heal_conv1x1 + depth-to-space, against torch's conv_transpose2d + batch_norm + relu in fp64."""
    import torch.nn as nn
    from heal_amd.opencood.models.sub_modules.bev_blocks import _Deblock
    from tests.golden.detfill import fill_module
    blk = fill_module(_Deblock(nn.ConvTranspose2d(cin, cout, k, stride=k, bias=False),
                               nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01))).cuda().eval()
    x = torch.randn((2, cin, H, W), generator=torch.Generator().manual_seed(k)).cuda()
    with torch.no_grad():
        got = blk(x)
        d = blk.double()
        ref = torch.relu(d[1](torch.nn.functional.conv_transpose2d(x.double(), d[0].weight, None, k)))
    assert got.shape == ref.shape == (2, cout, k * H, k * W)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4
    # the same deblock writing its channel slice of a wider (concatenated) tensor from the convolution's epilogue
    blk = blk.float()
    with torch.no_grad():
        cat = torch.full((2, cout + 24, k * H, k * W), 7.0, device="cuda")
        view = blk(x, into=(cat, 8))
    # same values as the stand-alone path (which may split the reduction over blocks on a tiny map: another summation tree)
    assert view.data_ptr() == cat[:, 8:].data_ptr() and float((view - got).abs().max() / got.abs().max()) < 1e-5
    assert bool((cat[:, :8] == 7.0).all()) and bool((cat[:, 8 + cout:] == 7.0).all())   # nothing written outside the slice


def test_decode_multiscale_feature_writes_the_concatenation_in_place():
    """ResNetBEVBackbone.decode_multiscale_feature (base_bev_backbone_resnet.py:122-138): three deblocks (k = 1, 2, 4) +
    torch.cat, with every deblock writing its slice of the concatenated tensor itself, against the separate
    pixel-shuffle + cat evaluation of the same modules and torch fp64."""
    from heal_amd.opencood.models.sub_modules.bev_blocks import ResNetBEVBackbone
    from tests.golden.detfill import fill_module
    cfg = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256],
           "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]}
    bb = fill_module(ResNetBEVBackbone(cfg, 64)).cuda().eval()
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn((2, 64, 32, 48), generator=g).cuda(), torch.randn((2, 128, 16, 24), generator=g).cuda(),
             torch.randn((2, 256, 8, 12), generator=g).cuda()]
    with torch.no_grad():
        got = bb.decode_multiscale_feature(feats)
        parts = [bb.deblocks[i](feats[i]) for i in range(3)]
        d = bb.double()
        ref = torch.cat([torch.relu(d.deblocks[i][1](torch.nn.functional.conv_transpose2d(
            feats[i].double(), d.deblocks[i][0].weight, None, d.deblocks[i][0].stride))) for i in range(3)], 1)
    assert got.shape == (2, 384, 32, 48) and float((got - torch.cat(parts, 1)).abs().max() / got.abs().max()) < 1e-5
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------- K6c (V2X-ViT linear algebra)
def _gelu64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


@pytest.mark.parametrize("T,K,N,ln,act,res", [(384, 64, 128, True, "gelu", True), (256, 256, 768, True, None, False),
                                              (1000, 96, 256, False, "relu", True), (128, 32, 128, False, None, False)])
def test_linear_vs_fp64(T, K, N, ln, act, res):
    """heal_linear (fp32 MFMA GEMM, LayerNorm statistics in the prologue, bias / activation / residual in the epilogue) against a
    float64 restatement of base_transformer.py:7-40's LayerNorm -> Linear -> GELU -> (+ x); ragged token count included."""
    from heal_amd import ops
    rng = np.random.default_rng(T + K + N)
    x = rng.standard_normal((T, K)).astype(np.float32) * 2 + 0.3
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) * 0.1
    g = rng.uniform(0.5, 1.5, K).astype(np.float32); be = rng.normal(0, 0.1, K).astype(np.float32)
    r = rng.standard_normal((T, N)).astype(np.float32)
    x64 = x.astype(np.float64)
    if ln:
        mu = x64.mean(1, keepdims=True); var = x64.var(1, keepdims=True)
        x64 = (x64 - mu) / np.sqrt(var + 1e-5) * g + be
    ref = x64 @ w.astype(np.float64).T + b
    if act == "gelu":
        ref = _gelu64(ref)
    elif act == "relu":
        ref = np.maximum(ref, 0)
    if res:
        ref = ref + r
    wd, bd = dev(w), dev(b)
    stats = None
    if ln:   # the caller folds gamma / beta into the weights (v2xvit_basic._fold_ln)
        wd, bd = dev(w * g[None, :]), dev(b + w @ be)
        stats = ops.ln_stats(dev(x), 1e-5)
        mu32, rstd32 = stats.cpu().numpy().T
        np.testing.assert_allclose(mu32, x.astype(np.float64).mean(1), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rstd32, 1 / np.sqrt(x.astype(np.float64).var(1) + 1e-5), rtol=1e-5)
    got = ops.linear(dev(x), wd, bd, stats=stats, act=act, residual=dev(r) if res else None).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)


def test_linear_row_map_parts_and_merged_projection():
    """Output addressing of heal_linear (column parts to separate buffers, [outer, inner] -> [inner, outer] row transposition) and
    the split-attention merge (split_attn.py:43-62 + mswin.py:79): three to_out projections, the per-agent softmax weights over
    the three window branches and the residual as ONE K = 3 C GEMM, against the reference's sequence in float64."""
    from heal_amd import ops
    rng = np.random.default_rng(5)
    L, HW, C = 3, 256, 128
    T = L * HW
    x = rng.standard_normal((T, C)).astype(np.float32)
    w3 = (rng.standard_normal((3 * C, C)) / np.sqrt(C)).astype(np.float32)
    ref = (x.astype(np.float64) @ w3.astype(np.float64).T).reshape(L, HW, 3, C).transpose(2, 1, 0, 3)   # [3, HW, L, C]
    got = ops.linear(dev(x), dev(w3), row_map=(HW, L), parts=3).view(3, HW, L, C).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    # split attention: branches [3, T, C] -> to_out_i -> radix softmax weights -> weighted sum + residual
    br = rng.standard_normal((3, T, C)).astype(np.float32)
    wo = (rng.standard_normal((3, C, C)) / np.sqrt(C)).astype(np.float32); bo = rng.normal(0, 0.1, (3, C)).astype(np.float32)
    fc1 = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    fc2 = (rng.standard_normal((3 * C, C)) / np.sqrt(C)).astype(np.float32)
    lg = rng.uniform(0.5, 1.5, C).astype(np.float32); lb = rng.normal(0, 0.1, C).astype(np.float32)
    outs = [br[i].astype(np.float64) @ wo[i].astype(np.float64).T + bo[i] for i in range(3)]          # to_out
    gap = sum(outs).reshape(L, HW, C).mean(1)                                                          # [L, C]
    h = gap @ fc1.astype(np.float64).T
    h = (h - h.mean(1, keepdims=True)) / np.sqrt(h.var(1, keepdims=True) + 1e-5) * lg + lb
    a = np.maximum(h, 0) @ fc2.astype(np.float64).T                                                    # [L, 3 C]
    a = a.reshape(L, 3, C); a = np.exp(a - a.max(1, keepdims=True)); a /= a.sum(1, keepdims=True)       # softmax over branches
    ref = sum(outs[i].reshape(L, HW, C) * a[:, i][:, None, :] for i in range(3)) + x.reshape(L, HW, C)
    scale, bias = ops.split_attn_weights(dev(br), L, HW, dev(wo), dev(bo), dev(fc1), dev(lg), dev(lb), 1e-5, dev(fc2))
    np.testing.assert_allclose(scale.cpu().numpy(), a, rtol=1e-4, atol=1e-5)
    wo_cat = np.concatenate([wo[0], wo[1], wo[2]], 1)
    got = ops.linear(dev(br), dev(wo_cat), bias, residual=dev(x), colscale=scale, colscale_part=C, group_rows=HW,
                     bias_per_group=True, x_parts=3).cpu().numpy().reshape(L, HW, C)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)


def test_agent_attention_agent_major_equals_pixel_major():
    from heal_amd import ops
    rng = np.random.default_rng(2)
    L, P = 5, 300
    q, k, v = (dev(rng.standard_normal((P, L, 256)).astype(np.float32)) for _ in range(3))
    a = ops.agent_attention(q, k, v, 8, 0.17)
    b = ops.agent_attention(q.transpose(0, 1).contiguous(), k.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous(),
                            8, 0.17, agent_major=True)
    assert torch.equal(b.transpose(0, 1), a)


def test_v2xvit_fused_path_equals_library_path(monkeypatch):
    """The round-3 inference path of the V2X-ViT encoder (heal_linear / heal_ln_stats / heal_split_attn_weights, no library GEMM)
    against the round-2 composition of library GEMMs and ATen kernels on the same weights (itself pinned by the reference
    goldens fusion_small / baseline_small)."""
    from heal_amd import configs
    from heal_amd.opencood.models.sub_modules.v2xvit_basic import V2XTransformer
    from tests.golden.detfill import fill_module
    m = fill_module(V2XTransformer(configs._v2xvit_args()["transformer"])).cuda().eval()
    x = dev(np.random.default_rng(3).standard_normal((4, 32, 48, 256)).astype(np.float32))
    with torch.no_grad():
        monkeypatch.setenv("HEAL_V2XVIT_FUSED", "0")
        ref = m(x)
        monkeypatch.setenv("HEAL_V2XVIT_FUSED", "1")
        got = m(x)
    assert float((got - ref).abs().max() / ref.abs().max()) < 2e-4


@pytest.mark.parametrize("L", [2, 5, 8])
def test_v2xvit_ego_tail_equals_full(monkeypatch, L):
    """The last V2X-ViT block computed for the ego agent's rows only (V2XTEncoder._ego_tail: queries of agent 0, keys / values of
    every agent, window attention / split attention / feed-forward on agent 0's tokens) returns for the fused map what the
    full computation returns -- the other agents' rows of the last block are never read (V2XTransformer returns agent 0).  The
    rows that are computed go through the same kernels in the same order: bit-identical."""
    from heal_amd import configs
    from heal_amd.opencood.models.sub_modules.v2xvit_basic import V2XTransformer
    from tests.golden.detfill import fill_module
    m = fill_module(V2XTransformer(configs._v2xvit_args()["transformer"])).cuda().eval()
    x = dev(np.random.default_rng(10 + L).standard_normal((L, 32, 48, 256)).astype(np.float32))
    with torch.no_grad():
        monkeypatch.setenv("HEAL_V2XVIT_EGO_TAIL", "0")
        full = m(x)
        monkeypatch.setenv("HEAL_V2XVIT_EGO_TAIL", "1")
        ego = m(x)
        assert full.shape == ego.shape == (32, 48, 256)
        assert torch.equal(full, ego)
        monkeypatch.setenv("HEAL_V2XVIT_FUSED", "0")          # and against the library composition (reference-pinned)
        ref = m(x)
    assert float((ego - ref).abs().max() / ref.abs().max()) < 2e-4


def test_rank_rulebook_equals_hash_rulebook(monkeypatch):
    """Strided output sites and neighbour rows through the rank structure (bitmap + prefix counts) = the hash + sort path,
    bit for bit, including the capacity-sized / device-count mode and sites dropped beyond a capacity."""
    from heal_amd import ops
    rng = np.random.default_rng(11)
    shape, batch = (21, 40, 52), 3
    idx = _random_sites(rng, 6000, shape, batch)
    feats = rng.standard_normal((len(idx), 4)).astype(np.float32)
    monkeypatch.setenv("HEAL_SP_RULEBOOK", "hash")
    x_h = ops.SparseTensor.from_unsorted(dev(feats), dev(idx), shape, batch)      # radix sort + hash grid
    assert x_h._rank is None
    monkeypatch.setenv("HEAL_SP_RULEBOOK", "rank")
    x = ops.SparseTensor.from_unsorted(dev(feats), dev(idx), shape, batch)        # root rank structure: one scatter, no sort
    assert x._rank is not None and x._rank_root
    assert torch.equal(x.indices, x_h.indices) and torch.equal(x._perm, x_h._perm) and torch.equal(x.features, x_h.features)
    sub = (3, 3, 3)
    assert torch.equal(x.neighbors(x.indices, shape, sub, (1, 1, 1), (1, 1, 1)),
                       x_h.neighbors(x_h.indices, shape, sub, (1, 1, 1), (1, 1, 1)))
    for k, st, pd in (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))):
        monkeypatch.setenv("HEAL_SP_RULEBOOK", "hash")
        oi_h, osh, _, rk = x_h.out_sites_ex(k, st, pd)
        assert rk is None
        nbr_h = x_h.neighbors(oi_h, osh, k, st, pd)
        monkeypatch.setenv("HEAL_SP_RULEBOOK", "rank")
        oi, osh2, _, rank = x.out_sites_ex(k, st, pd)
        assert osh == osh2 and torch.equal(oi, oi_h) and rank is not None
        y = ops.SparseTensor(torch.zeros((oi.shape[0], 4), device="cuda"), oi, osh, batch)
        y_h = ops.SparseTensor(torch.zeros((oi.shape[0], 4), device="cuda"), oi, osh, batch)
        y._rank = rank
        assert torch.equal(y.neighbors(oi, osh, sub, (1, 1, 1), (1, 1, 1)), y_h.neighbors(oi, osh, sub, (1, 1, 1), (1, 1, 1)))
        assert torch.equal(x.neighbors(oi, osh, k, st, pd), nbr_h)


def test_root_rank_structure_device_counts_and_reuse(monkeypatch):
    """heal_sp_root_rank with a device-side row count and capacity-sized buffers (the graph-captured encoder): the live rows come out
    sorted exactly as the radix sort leaves them; the structure is rebuilt on a DIFFERENT site set in the same (dirty) buffer --
    only the granule directory is cleared per call, stale granule words must never leak; sites on the first / last cell of the
    grid and in neighbouring granules."""
    from heal_amd import _capi, ops
    rng = np.random.default_rng(23)
    shape, batch = (41, 64, 300), 2          # 300 cells per row: granules straddle rows
    cap = 5000
    nbytes = _capi.query("heal_sp_root_rank_bytes", ops._i3(shape), batch)
    rank = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")          # garbage on entry
    for trial, n_live in enumerate((4000, 1500, 4999)):
        idx = _random_sites(rng, n_live - 2, shape, batch)
        idx = np.unique(np.concatenate([idx, [[0, 0, 0, 0], [batch - 1, shape[0] - 1, shape[1] - 1, shape[2] - 1]]]).astype(np.int32), axis=0)
        rng.shuffle(idx)
        n_live = len(idx)
        pad = np.concatenate([idx, np.full((cap - n_live, 4), 7, np.int32)])     # rows beyond the live count: junk
        n_dev = torch.tensor([n_live], dtype=torch.int32, device="cuda")
        out = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")
        perm = torch.zeros((cap,), dtype=torch.int32, device="cuda")
        feats = dev(rng.standard_normal((cap, 4)).astype(np.float32))
        fs = torch.zeros((cap, 4), device="cuda")
        _capi.call("heal_sp_root_rank", ops._ptr(dev(pad)), cap, ops._i3(shape), batch, ops._ptr(out), ops._ptr(perm), ops._ptr(feats), 4,
                   ops._ptr(fs), ops._ptr(rank), nbytes, ops._ptr(n_dev), ops._stream())
        key = ((idx[:, 0].astype(np.int64) * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
        order = np.argsort(key, kind="stable")
        np.testing.assert_array_equal(out[:n_live].cpu().numpy(), idx[order])
        np.testing.assert_array_equal(perm[:n_live].cpu().numpy(), order)
        assert torch.equal(fs[:n_live], feats[torch.from_numpy(order).cuda()]) and bool((fs[n_live:] == 0).all())
        assert bool((out[n_live:] == -1).all())
        # neighbour rows through the structure = brute force on the sorted coordinates
        nbr = torch.empty((cap, 27), dtype=torch.int32, device="cuda")
        _capi.call("heal_sp_neighbors_root", ops._ptr(out), cap, ops._i3((3, 3, 3)), ops._i3((1, 1, 1)), ops._i3((1, 1, 1)),
                   ops._i3(shape), ops._i3(shape), batch, ops._ptr(rank), nbytes, cap, ops._ptr(n_dev), ops._ptr(nbr), ops._ptr(n_dev),
                   ops._stream())
        from oracle import oracle_np as O
        _, _, want = O.sparse_conv_rules(idx[order], list(shape), (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
        np.testing.assert_array_equal(nbr[:n_live].cpu().numpy(), want)


@pytest.mark.parametrize("n,width,cout,H,W,res", [(2, 128, 64, 24, 40, True), (1, 256, 128, 17, 36, True), (3, 128, 64, 8, 32, False),
                                                   (1, 256, 64, 9, 12, True)])
def test_gconv_conv3_equals_two_kernel_path(n, width, cout, H, W, res):
    """heal_gconv_conv3 (opt-in: the grouped 3x3 + pointwise conv + identity + ReLU of a ResNeXt bottleneck in one wave-specialised
    kernel, the 2C-wide intermediate in LDS) against float64 and against the two-kernel path: 4 and 8 channels per group, maps that
    are not multiples of the 8 x 32 tile, with and without the identity."""
    _need_experimental()
    from heal_amd import ops
    rng = np.random.default_rng(width + H)
    g = 32
    x = dev(rng.standard_normal((n, width, H, W)).astype(np.float32))
    w2 = dev((rng.standard_normal((width, width // g, 3, 3)) / np.sqrt(9 * width // g)).astype(np.float32))
    b2 = dev(rng.standard_normal(width).astype(np.float32) * 0.1)
    w3 = dev((rng.standard_normal((cout, width, 1, 1)) / np.sqrt(width)).astype(np.float32))
    b3 = dev(rng.standard_normal(cout).astype(np.float32) * 0.1)
    r = dev(rng.standard_normal((n, cout, H, W)).astype(np.float32)) if res else None
    assert ops.gconv_conv3_supported(width, width // g, cout, H, W)
    got = ops.gconv_conv3(x, w2, b2, g, w3, b3, r, True)
    split = ops.conv1x1(ops.grouped_conv3x3(x, w2, b2, g, 1, True), w3, b3, r, 1)
    F_ = torch.nn.functional
    ref = F_.conv2d(torch.relu(F_.conv2d(x.double(), w2.double(), b2.double(), 1, 1, 1, g)), w3.double(), b3.double())
    ref = torch.relu(ref + r.double() if res else ref)
    scale = float(ref.abs().max())
    assert float((got.double() - ref).abs().max()) < 2e-6 * scale
    assert float((got - split).abs().max()) < 4e-6 * scale


@pytest.mark.parametrize("n,cin,cout,H,W,ks,stride,res", [(2, 64, 128, 40, 56, 3, 2, True), (1, 96, 256, 33, 24, 3, 2, False),
                                                           (2, 32, 128, 18, 20, 3, 1, True), (1, 64, 128, 16, 24, 1, 1, False),
                                                           (1, 32, 128, 15, 16, 1, 2, True)])
def test_conv_gemm_vs_torch_fp64(n, cin, cout, H, W, ks, stride, res):
    """heal_conv_gemm (implicit GEMM on 128 x 128 x 32 tiles of the 32x32x2 fp32 MFMA) against a float64 convolution: 3x3 padding 1
    and 1x1, stride 1 | 2, odd map heights, tiles that straddle the map border, bias + residual + ReLU."""
    from heal_amd import ops
    rng = np.random.default_rng(n * 100 + cin + cout + H)
    x = rng.standard_normal((n, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = rng.standard_normal((n, cout, Ho, Wo)).astype(np.float32)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                     stride, ks // 2)
    if res:
        ref = ref + torch.from_numpy(r).double()
    ref = torch.relu(ref).numpy()
    got = ops.conv_gemm(dev(x), dev(w), dev(b), dev(r) if res else None, True, stride).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n,cin,cout,H,W,res,act", [(2, 128, 256, 64, 64, False, 1), (1, 256, 64, 96, 128, True, 0),
                                                    (3, 64, 128, 40, 52, False, 3), (1, 512, 256, 32, 36, True, 1)])
def test_conv1x1_tiled_equals_torch(n, cin, cout, H, W, res, act, monkeypatch):
    """heal_conv1x1_tiled (128 x 128 x 32 core on 32x32x2 fp32 MFMA, plain [Cout, Cin] weights; opt-in: at parity with heal_conv1x1
    at the scenes' shapes) against F.conv2d with the fused epilogues, incl. pixel counts that are not multiples of the 128-pixel
    tile and the depth-to-space write of the deblocks."""
    _need_experimental()
    from heal_amd import ops
    monkeypatch.setenv("HEAL_C1_TILED", "force")
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    r = torch.randn((n, cout, H, W), generator=g).cuda() if res else None
    assert ops.conv1x1_tiled_ok(n, cin, cout, H * W)
    got = ops.conv1x1(x, w, b, r, act)
    ref = torch.nn.functional.conv2d(x, w, b)
    if res:
        ref = ref + r
    ref = {0: lambda t: t, 1: torch.relu, 3: torch.nn.functional.gelu}[act](ref)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
    if not res and cout % 4 == 0 and W % 4 == 0:
        dst = torch.full((n, cout // 4 + 3, 2 * H, 2 * W), -7.0, device="cuda")
        ops.conv1x1_d2s(x, w, b, 1, 2, dst, 2)
        want = torch.nn.functional.pixel_shuffle(torch.relu(torch.nn.functional.conv2d(x, w, b)), 2)
        assert float((dst[:, 2:2 + cout // 4] - want).abs().max() / want.abs().max()) < 1e-5
        assert float(dst[:, :2].min()) == -7.0 and float(dst[:, 2 + cout // 4:].max()) == -7.0


@pytest.mark.parametrize("n,dims,f64,kind", [(5, [(64, 256, 256), (128, 128, 128), (256, 64, 64)], True, "pose"),
                                             (3, [(24, 40, 56), (12, 20, 28)], False, "pose"),
                                             (2, [(8, 48, 48)], True, "zoom"), (8, [(16, 32, 32), (8, 16, 16), (8, 8, 8), (4, 4, 4)], True, "pose")])
def test_warp_fuse_levels_equals_per_level(n, dims, f64, kind):
    """heal_warp_fuse_levels (all pyramid levels in ONE launch, the source footprint of every 16 x 16 ego tile staged through LDS)
    must be BIT-IDENTICAL to heal_warp_fuse level by level -- same sampling arithmetic, same summation order -- at the scene's
    full size (5 agents, 64 / 128 / 256 channels), on maps that do not fill a tile, with a camera crop window, with device-resident
    affine rows, and for a ZOOMING affine matrix whose footprint does not fit the staging tile (direct-gather fallback)."""
    from heal_amd import ops, synth
    from heal_amd.opencood.models.fuse_modules.pyramid_fuse import crop_window
    rng = np.random.default_rng(n * 10 + len(dims))
    if kind == "pose":
        poses = synth.agent_poses(11 + n, n, r_min=2.0, r_max=30.0)
        pw = synth.pairwise_t_matrix(poses, 8)[None].astype(np.float64 if f64 else np.float32)
        rows = O.normalize_pairwise_tfm(pw, 204.8, 204.8, 1)[0][0, :n]
    else:   # 3x zoom-out + rotation: a 16 x 16 ego tile reads a ~60 x 60 source box
        th = 0.6
        rows = np.stack([np.array([[3 * np.cos(th), -3 * np.sin(th), 0.1], [3 * np.sin(th), 3 * np.cos(th), -0.2]]),
                         np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])]).astype(np.float64)
    feats = [dev(rng.standard_normal((n, C, H, W)).astype(np.float32)) for C, H, W in dims]
    occs = [dev((rng.standard_normal((n, 1, H, W)) * 2).astype(np.float32)) for C, H, W in dims]
    crops = None
    if n >= 3:
        crops = [[crop_window(H, W, 2.0, 2.0) if a == 1 else None for a in range(n)] for C, H, W in dims]
    got = ops.warp_fuse_levels(feats, occs, rows, f64, crops)
    for l, (C, H, W) in enumerate(dims):
        cr = None if crops is None else [c if c is not None else (0, 0, 0, 0) for c in crops[l]]
        want = ops.warp_fuse(feats[l], occs[l], rows, f64, cr)
        assert got[l].shape == want.shape == (C, H, W)
        assert torch.equal(got[l], want), (l, float((got[l] - want).abs().max()))
    again = ops.warp_fuse_levels(feats, occs, torch.from_numpy(np.asarray(rows, dtype=np.float64)).cuda(), f64, crops)
    if f64:
        assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("n,cx,cin,H,W,pool", [(4, 3, 3, 336, 448, True), (2, 4, 3, 96, 128, True), (1, 3, 3, 50, 70, True),
                                               (3, 4, 4, 33, 47, False), (1, 1, 1, 64, 64, True), (2, 3, 2, 40, 36, False)])
def test_stem7x7_equals_torch(n, cx, cin, H, W, pool):
    """heal_stem7x7 (ResNet image stem: 7x7 / 2 convolution + folded BN + ReLU + 3x3 / 2 max-pool in one kernel, the first `cin`
    channels of the image tensor read in place) against plain PyTorch fp32: conv2d -> relu -> max_pool2d; full camera size, odd
    sizes whose last tiles hang over the map, a 4-channel image tensor of which 3 channels are used, and the pool-free form."""
    import torch.nn.functional as F
    from heal_amd import ops
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.randn((n, cx, H, W), generator=g).cuda()
    w = (torch.randn((64, cin, 7, 7), generator=g) / (49 * cin) ** 0.5).cuda()
    b = torch.randn((64,), generator=g).cuda()
    got = ops.stem7x7(x, w, b, pool=pool)
    ref = torch.relu(F.conv2d(x[:, :cin], w, b, stride=2, padding=3))
    if pool:
        ref = F.max_pool2d(ref, 3, 2, 1)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max() / ref.abs().max()) < 2e-6


def test_full_scene_nms_pairs_against_exact_rational_iou():
    """VERDICT r5 item 7, the full-size half: the candidates of ONE full-size scene (the 5-agent heterogeneous scene bench.py times,
    calibrated to several hundred candidates) -- EVERY pair of the top-1000 whose bounding boxes overlap goes through the exact-rational
    IoU (oracle/exact_iou.py); the GPU kernel's IoU (heal_quad_iou: the arithmetic k_nms_mask uses) must be the true value rounded to
    fp32 (one ulp of slack) and take the same `> 0.15` decision for every pair; pairs within 1e-9 of the threshold are counted."""
    from fractions import Fraction
    from heal_amd import configs, ops
    from heal_amd.pipeline import Scene, ScenePipeline
    from oracle import exact_iou as E
    from tests.report import note
    mods = ["m1", "m1", "m1", "m2", "m4"]
    hypes = configs.heal_heter(("m1", "m2", "m4"), max_cav=5)
    pipe = ScenePipeline(hypes, "cuda:0", seed=0)
    scene = Scene(5, seed=4, device="cuda:0", modalities=mods)
    pipe.calibrate_cls_bias(scene, target_candidates=600)
    with torch.no_grad():
        out = pipe.forward(scene)
    pp = pipe.post.params
    corners, scores, _ = O.decode_candidates(out["cls_preds"].cpu().numpy(), out["reg_preds"].cpu().numpy(), out["dir_preds"].cpu().numpy(),
                                             pipe.anchor_box.cpu().numpy(), pp["target_args"]["score_threshold"], 0.7853, 2,
                                             np.eye(4, dtype=np.float32))
    order = O.nms_order(scores, 1000)
    quads = np.ascontiguousarray(corners[order][:, :4, :2], np.float32)
    n = len(quads)
    assert n >= 100, n
    lo, hi = quads.min(1), quads.max(1)
    ov = ((lo[:, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[:, None, :])).all(2)
    ii, jj = np.nonzero(np.triu(ov, 1))
    got = ops.quad_iou(torch.from_numpy(quads).cuda(), torch.from_numpy(quads).cuda()).cpu().numpy()
    ref = cref.quad_iou(quads, quads)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))          # kernel == C oracle, bit for bit
    assert (got[~ov] == 0).all()                                                       # disjoint bounding boxes: exactly zero
    if len(ii) > 20000:                                                                # (bounds the Python rationals: ~1 ms per pair)
        sel = np.random.default_rng(0).choice(len(ii), 20000, replace=False)
        ii, jj = ii[sel], jj[sel]
    thr32 = np.float32(0.15)
    thr = Fraction(float(thr32))
    close = flips = off = 0
    for i, j in zip(ii, jj):
        t = E.exact_quad_iou(quads[i], quads[j])
        if t is None:
            continue
        tf = np.float32(float(t))
        g = got[i, j]
        if tf != g:
            off += 1
            # (one fp32 ulp of the true value, plus the fp64 clip's own ABSOLUTE error: a sliver of 1e-9 of the union is a difference of
            #  nearly equal areas -- its fp64 value is good to ~1e-12 absolute, not to 1e-7 of itself)
            assert abs(float(g) - float(t)) <= np.spacing(tf) + 1e-10, (i, j, float(g), float(t))
        close += abs(t - thr) < Fraction(1, 10 ** 9)
        flips += bool(g > thr32) != bool(tf > thr32)
    note("nms_full_scene_exact_rational", candidates=int(n), overlapping_pairs=int(len(ii)), within_1e9_of_threshold=int(close),
         decision_flips=int(flips), not_the_rounded_true_value=int(off))
    assert flips == 0


@pytest.mark.parametrize("nprod", [6, 9])
@pytest.mark.parametrize("n,cin,cout,H,W,res,act", [(2, 512, 256, 64, 64, True, 1), (1, 256, 512, 64, 64, False, 1), (3, 128, 256, 40, 52, False, 3),
                                                    (1, 64, 128, 96, 128, True, 0), (1, 1152, 128, 12, 16, False, 2), (2, 32, 128, 9, 20, False, 0)])
def test_conv1x1_split_bf16_error_vs_exact_fp32_kernel(n, cin, cout, H, W, res, act, nprod, monkeypatch):
    """heal_conv1x1_split (OPT-IN, HEAL_ARITH=bf16x6 | bf16x9: fp32 in / out / accumulate on the bf16 matrix cores by 3-way operand
    splitting) -- the pre-registered acceptance criterion of VERDICT r5 item 2 (i): on the same shapes its maximum error against an fp64
    reference is at most 2x that of the exact-fp32 MFMA kernel (heal_conv1x1).  Inputs with a wide dynamic range (products of normals
    and log-uniform scales) so that the dropped / reordered low-order terms would show."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout + nprod)
    scale = torch.exp2(torch.randint(-6, 7, (n, cin, 1, 1), generator=g).float())
    x = (torch.randn((n, cin, H, W), generator=g) * scale).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    r = torch.randn((n, cout, H, W), generator=g).cuda() if res else None
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double())
    if r is not None:
        ref = ref + r.double()
    ref = {0: lambda t: t, 1: torch.relu, 2: torch.nn.functional.silu, 3: lambda t: torch.nn.functional.gelu(t)}[act](ref)
    monkeypatch.delenv("HEAL_ARITH", raising=False)
    exact = ops.conv1x1(x, w, b, r, act)
    monkeypatch.setenv("HEAL_ARITH", f"bf16x{nprod}")
    assert ops.arith_products() == nprod
    split = ops.conv1x1(x, w, b, r, act)
    s_ref = float(ref.abs().max())
    e_exact = float((exact.double() - ref).abs().max()) / s_ref
    e_split = float((split.double() - ref).abs().max()) / s_ref
    from tests.report import note
    note("conv1x1_split_error", shape=[n, cin, cout, H, W], products=nprod, err_exact_fp32_kernel=e_exact, err_split=e_split)
    assert e_split <= 2.0 * e_exact + 1e-9, (e_split, e_exact)
    assert e_split < 2e-6


@pytest.mark.parametrize("n,cin,cout,H,W,relu", [(1, 128, 64, 64, 64, True), (2, 32, 64, 40, 56, False), (1, 64, 128, 30, 24, True)])
def test_conv7x7_stride2_vs_torch(n, cin, cout, H, W, relu):
    """Round 6: the 7x7 / stride 2 / padding 3 stem of BevEncode (lss_submodule.py:242; the last convolution a mirrored model left to the
    library) on heal_conv_gemm's implicit GEMM (Cout padded to a 128-channel tile) against torch's fp64 convolution."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn((n, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 7, 7), generator=g) / (49 * cin) ** 0.5).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    assert ops.conv7x7_s2_supported(cin, cout, W)
    got = ops.conv7x7_s2(x, w, b, relu)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), 2, 3)
    ref = torch.relu(ref) if relu else ref
    assert got.shape == ref.shape and got.is_contiguous()
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-5
    got2 = ops.conv7x7_s2(x, w, None, False)
    ref2 = torch.nn.functional.conv2d(x.double(), w.double(), None, 2, 3)
    assert float((got2.double() - ref2).abs().max() / ref2.abs().max()) < 1e-5
