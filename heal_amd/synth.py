"""Synthetic OPV2V-shaped scenes: seeded LiDAR frames, camera rigs and agent poses.

There is no dataset on the GPU box; bench.py, smoke() and the tests build their inputs here.
Everything is numpy + a seed, so the same scene can be regenerated anywhere.
"""
import math

import numpy as np


def lidar_frame(seed, n_rings=64, n_azimuth=1024, sensor_height=1.9, n_boxes=40, max_range=120.0,
                dropout=0.05):
    """One spinning-LiDAR sweep: rays hit the ground plane or one of `n_boxes` car-sized boxes.

    Returns float32 [N,4] (x, y, z, intensity) in the sensor frame, after the reference's
    ego-point mask (opencood/utils/pcd_utils.py:70-88) and a seeded shuffle (:91-95).
    """
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(-25.0, 2.0, n_rings))
    azim = np.linspace(-np.pi, np.pi, n_azimuth, endpoint=False)
    el, az = np.meshgrid(elev, azim, indexing="ij")
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    # ground plane z = -sensor_height
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ground = np.where(dirs[:, 2] < -1e-6, -sensor_height / dirs[:, 2], np.inf)
    t = np.minimum(t_ground, max_range)
    # boxes: axis-aligned in their own yaw frame, 4.5 x 2 x 1.6 m, sitting on the ground
    centers = rng.uniform(-100.0, 100.0, size=(n_boxes, 2))
    yaws = rng.uniform(-np.pi, np.pi, size=n_boxes)
    half = np.array([2.25, 1.0, 0.8])
    for c, yaw in zip(centers, yaws):
        ca, sa = math.cos(yaw), math.sin(yaw)
        R = np.array([[ca, sa, 0.0], [-sa, ca, 0.0], [0.0, 0.0, 1.0]])  # world -> box
        o = R @ np.array([-c[0], -c[1], sensor_height - 0.8])  # ray origin in the box frame
        d = dirs @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (-half - o) / d
            t2 = (half - o) / d
        tn = np.nanmax(np.minimum(t1, t2), axis=1)
        tf = np.nanmin(np.maximum(t1, t2), axis=1)
        hit = (tn <= tf) & (tn > 0.5)
        t = np.where(hit & (tn < t), tn, t)
    keep = np.isfinite(t) & (t < max_range) & (rng.uniform(size=t.shape) >= dropout)
    pts = dirs[keep] * t[keep, None]
    pts = pts + rng.normal(0.0, 0.01, size=pts.shape)
    inten = rng.uniform(0.0, 1.0, size=(pts.shape[0], 1))
    pcd = np.concatenate([pts, inten], 1).astype(np.float32)
    # mask_ego_points
    ego = (pcd[:, 0] >= -1.95) & (pcd[:, 0] <= 2.95) & (pcd[:, 1] >= -1.1) & (pcd[:, 1] <= 1.1)
    pcd = pcd[~ego]
    rng.shuffle(pcd, axis=0)
    return np.ascontiguousarray(pcd)


def x_to_world(pose):
    """pose = [x, y, z, roll, yaw, pitch] (degrees), the reference's convention
    (opencood/utils/transformation_utils.py:264-307) -> 4x4 float64."""
    x, y, z, roll, yaw, pitch = pose
    c_y, s_y = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    c_r, s_r = math.cos(math.radians(roll)), math.sin(math.radians(roll))
    c_p, s_p = math.cos(math.radians(pitch)), math.sin(math.radians(pitch))
    m = np.identity(4)
    m[0, 3], m[1, 3], m[2, 3] = x, y, z
    m[0, 0] = c_p * c_y
    m[0, 1] = c_y * s_p * s_r - s_y * c_r
    m[0, 2] = -c_y * s_p * c_r - s_y * s_r
    m[1, 0] = s_y * c_p
    m[1, 1] = s_y * s_p * s_r + c_y * c_r
    m[1, 2] = -s_y * s_p * c_r + c_y * s_r
    m[2, 0] = s_p
    m[2, 1] = -c_p * s_r
    m[2, 2] = c_p * c_r
    return m


def agent_poses(seed, n_agents, r_min=10.0, r_max=60.0):
    """Ego at the origin; agent k at radius U(r_min,r_max), bearing 2*pi*k/n, yaw U(-180,180)."""
    rng = np.random.default_rng(seed)
    poses = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]
    for k in range(1, n_agents):
        r = rng.uniform(r_min, r_max)
        b = 2.0 * math.pi * k / n_agents
        poses.append([r * math.cos(b), r * math.sin(b), 0.0, 0.0, rng.uniform(-180.0, 180.0), 0.0])
    return poses


def pairwise_t_matrix(poses, max_cav):
    """[L,L,4,4] float64, entry [i,j] = T_{j<-i} = inv(T_j) T_i (transformation_utils.py:21-66,
    proj_first = False); identity beyond the present agents."""
    L = max_cav
    out = np.tile(np.eye(4), (L, L, 1, 1))
    T = [x_to_world(p) for p in poses]
    for i in range(len(T)):
        for j in range(len(T)):
            if i != j:
                out[i, j] = np.linalg.solve(T[j], T[i])
    return out


def teacher_points(clouds, poses, lidar_range):
    """The early-fusion cloud DiscoNet's teacher sees (intermediate_fusion_dataset.py:96-117, 391-395): every agent's cloud
    [N_k,4] projected into the ego frame (agent 0; T_{0<-k} = inv(T_0) T_k, float32 arithmetic as project_points_by_matrix_torch),
    stacked in agent order, and masked to the open box of `lidar_range` (pcd_utils.py:41-67).  -> float32 [N,4]."""
    T0 = x_to_world(poses[0])
    out = []
    for pts, pose in zip(clouds, poses):
        pts = np.asarray(pts, np.float32)
        tfm = np.linalg.solve(T0, x_to_world(pose)).astype(np.float32)
        xyz1 = np.concatenate([pts[:, :3], np.ones((pts.shape[0], 1), np.float32)], 1)
        out.append(np.concatenate([(xyz1 @ tfm.T)[:, :3], pts[:, 3:4]], 1))
    p = np.vstack(out)
    r = lidar_range
    keep = ((p[:, 0] > r[0]) & (p[:, 0] < r[3]) & (p[:, 1] > r[1]) & (p[:, 1] < r[4]) & (p[:, 2] > r[2]) & (p[:, 2] < r[5]))
    return np.ascontiguousarray(p[keep], dtype=np.float32)


def teacher_processed_lidar(scenes, lidar_range, voxelize):
    """`teacher_processed_lidar` of a batch: scenes = [(clouds, poses), ...]; each scene's teacher_points voxelised ONCE
    (intermediate_fusion_dataset.py:396) by `voxelize(points, batch_idx) -> (voxels, coords (b,z,y,x), num_points)` (numpy; the
    oracle's voxeliser on the CPU, heal_voxelize on the device) and collated like collate_batch_list: one sample per scene."""
    parts = [voxelize(teacher_points(clouds, poses, lidar_range), b) for b, (clouds, poses) in enumerate(scenes)]
    return {"voxel_features": np.concatenate([v for v, _, _ in parts]), "voxel_coords": np.concatenate([c for _, c, _ in parts]),
            "voxel_num_points": np.concatenate([n for _, _, n in parts])}


def camera_rig(seed, n_cams=4, H=384, W=512):
    """Four cameras yawed 0/100/-100/180 deg, 90-degree FoV, no post-augmentation.
    Returns dict of float32 arrays: rots [n,3,3], trans [n,3], intrins [n,3,3], post_rots, post_trans."""
    yaws = np.deg2rad([0.0, 100.0, -100.0, 180.0])[:n_cams]
    rots, trans = [], []
    # camera frame (x right, y down, z forward) -> ego frame (x forward, y left, z up)
    base = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    for yw in yaws:
        c, s = math.cos(yw), math.sin(yw)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        rots.append(Rz @ base)
        trans.append(Rz @ np.array([1.0, 0.0, 1.5]))
    K = np.array([[W / 2.0, 0.0, W / 2.0], [0.0, W / 2.0, H / 2.0], [0.0, 0.0, 1.0]])
    return {
        "rots": np.stack(rots).astype(np.float32),
        "trans": np.stack(trans).astype(np.float32),
        "intrins": np.tile(K, (n_cams, 1, 1)).astype(np.float32),
        "post_rots": np.tile(np.eye(3), (n_cams, 1, 1)).astype(np.float32),
        "post_trans": np.zeros((n_cams, 3), np.float32),
    }


# ---- detection-head maps for the late-fusion decode (tests, tests/golden/gen_golden_late.py, scripts/late_bench.py) ---------
BACKGROUND = -6.0


def make_cav(rng, anchors, tfm, n_clusters, mode="normal", density=0.8):
    """One cav's maps (tfm: its 4x4 cav -> ego matrix).  Background everywhere; `n_clusters` 3 x 3 neighbourhoods (both
    anchors) marked as candidates (their logits are filled from the ladder later).  mode "empty": no candidate; "filtered":
    every candidate far too high or too long; "dense": every anchor a candidate."""
    H, W, A = anchors.shape[:3]
    cls = rng.uniform(BACKGROUND - 2.0, BACKGROUND + 2.0, (1, A, H, W)).astype(np.float32)
    reg = np.zeros((1, 7 * A, H, W), np.float32)
    dirp = np.zeros((1, 2 * A, H, W), np.float32)
    cand = np.zeros((A, H, W), bool)
    if mode == "dense":
        cand[:] = True
    elif mode != "empty":
        for _ in range(n_clusters):
            h0, w0 = rng.integers(1, H - 1), rng.integers(1, W - 1)
            cand[:, h0 - 1:h0 + 2, w0 - 1:w0 + 2] |= rng.random((A, 3, 3)) < density
    a, h, w = np.nonzero(cand)
    d = (rng.standard_normal((len(a), 7)) * 0.2).astype(np.float32)
    if mode == "filtered":
        half = np.arange(len(a)) % 2 == 0
        d[half, 2] = 4.0 + rng.uniform(0, 1, half.sum())             # z centre ~ 5 m: zmax > 1
        d[~half, 5] = 1.2 + rng.uniform(0, 0.3, (~half).sum())       # l = 3.9 e^1.2 ~ 13 m: x_len or y_len > 6
    for k in range(7):
        reg[0, a * 7 + k, h, w] = d[:, k]
    for b in range(2):
        dirp[0, a * 2 + b, h, w] = rng.standard_normal(len(a)).astype(np.float32)
    tfm = np.asarray(tfm, np.float32)
    return {"cls": cls, "reg": reg, "dir": dirp, "anchors": anchors, "tfm": tfm, "_cand": cand}


def deal_ladder(rng, cavs, lo=0.25, hi=0.95, min_step=2e-5):
    """Distinct scores lo, lo + step, ... < hi dealt to the candidates of all cavs in random order; the step must be at least
    `min_step` (twice the score margin the late-fusion fixtures keep)."""
    total = sum(int(c["_cand"].sum()) for c in cavs)
    step = (hi - lo) / total
    assert step >= min_step, step
    scores = lo + step * rng.permutation(total).astype(np.float64)
    logits = np.log(scores / (1.0 - scores)).astype(np.float32)
    off = 0
    for c in cavs:
        n = int(c["_cand"].sum())
        c["cls"][0][c["_cand"]] = logits[off:off + n]
        off += n
