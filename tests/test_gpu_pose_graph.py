"""heal_pose_graph_align (heal_amd/csrc/pose_graph.hip, ops.pose_graph_align) against the float64 host path of the box alignment
(box_align_v2.box_alignment_relative_sample_np), at the smallest shapes at which each part of the kernel can go wrong.

  integers      cluster_of_box, the landmark count and the edge count equal the host path's exactly (the fixtures' generator asserts
                the margins that make them comparable: tests/posegraph_refs.py)
  poses         within 10 x d_ref of the host path's float64 result, in metres and in radians; d_ref is the recorded disagreement
                of the two CPU solvers (profiles/pose_graph_tolerance.json, tests/test_pose_graph_cpu.py) -- never a figure of
                the kernel's.  The factor 10 covers a different, equally valid LM path to the same stationary point.
  stationarity  the inf-norm of the cost's gradient at the kernel's agent poses (float64, on the host, every landmark at its own
                optimum) is at most 10 x the host path's own at its result
"""
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, configs, ops
from heal_amd.opencood.models.sub_modules import box_align_v2 as BA
from heal_amd.opencood.models.sub_modules import pose_graph_optim as PG
from tests import posegraph_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_AGENTS, MAX_BOXES = 8, 1024
BN = (0.1, 0.02)


def tol():
    return 10.0 * R.d_ref()


def to_device(scenes, dtype=torch.float64):
    corners, unc, pose, rec = [], [], [], []
    with_unc = all(s["unc"] is not None for s in scenes)
    for s in scenes:
        corners += [torch.from_numpy(c).to(DEV, dtype) for c in s["corners"]]
        if with_unc:
            unc += [torch.from_numpy(u).to(DEV, dtype) for u in s["unc"]]
        pose.append(s["pose"])
        rec.append(s["pose"].shape[0])
    return corners, torch.from_numpy(np.concatenate(pose)).to(DEV), unc if with_unc else None, rec


def run(scenes, **extra):
    """-> per scene dict(refined [A,3], cluster, landmarks, edges, iterations, status, chi2) from ONE launch over all scenes (they
    share their options)."""
    corners, pose, unc, rec = to_device(scenes)
    refined, stats, cluster = ops.pose_graph_align(corners, pose, unc, rec, return_stats=True, **{**scenes[0]["opts"], **extra})
    torch.cuda.synchronize()
    refined, cluster = refined.cpu().numpy(), cluster.cpu().numpy()
    stats = {k: v.cpu().numpy() for k, v in stats.items()}
    out, a, b = [], 0, 0
    for k, s in enumerate(scenes):
        A, nb = s["pose"].shape[0], sum(len(c) for c in s["corners"])
        out.append({"refined": refined[a:a + A], "cluster": cluster[b:b + nb], "landmarks": int(stats["landmarks"][k]),
                    "edges": int(stats["edges"][k]), "iterations": int(stats["iterations"][k]), "status": int(stats["status"][k]),
                    "chi2": float(stats["chi2_final"][k])})
        a, b = a + A, b + nb
    return out


def check(s, stationarity=True):
    """One scene alone on the device against the host path: integers, poses, stationarity.  -> (device result, host result)."""
    got, want = run([s])[0], R.host_result(s)
    assert np.array_equal(got["cluster"], want["cluster_of_box"])
    assert (got["landmarks"], got["edges"]) == (want["landmarks"], want["active_edges"])
    assert got["status"] == want["status"], (got["status"], want["status"])
    d = R.pose_disagreement(got["refined"], want["refined"])
    print(f"seed {s['seed']}: {got['landmarks']} landmarks, {got['edges']} edges, iterations device {got['iterations']} host "
          f"{want['iterations']}, pose disagreement {d:.3e} (tolerance {tol():.3e})")
    assert d <= tol(), (d, tol())
    assert np.all(got["refined"][:, 2] > -180.0) and np.all(got["refined"][:, 2] <= 180.0)
    if stationarity and want["pgo"] is not None:
        _, g_dev = R.reduced_cost_and_gradient(s, got["refined"])
        _, g_host = R.reduced_cost_and_gradient(s, want["refined"])
        print(f"    gradient inf-norm: device {g_dev:.3e}, host {g_host:.3e}")
        assert g_dev <= 10.0 * g_host, (g_dev, g_host)
    return got, want


# ---- agents ------------------------------------------------------------------------------------------------------------------
def test_one_agent_returns_its_pose_with_zero_landmarks():
    s = R.scene(601, 1, 5, min_seen_by=1, seen=1.0)
    got, _ = check(s)
    assert got["landmarks"] == 0 and got["edges"] == 0 and got["status"] == PG.STATUS_NO_EDGES
    assert got["refined"].tobytes() == s["pose"][:, [0, 1, 4]].tobytes()


@pytest.mark.parametrize("agents", [2, 3, 5, 8])
def test_noise_free_boxes_recover_the_true_poses(agents):
    s = R.scene(610 + agents, agents, 3 * agents)
    got, _ = check(s)
    true = np.c_[s["true_pose"][:, :2], np.degrees(s["true_pose"][:, 2])]
    assert R.pose_disagreement(s["pose"][:, [0, 1, 4]], true) > 0.05
    assert R.pose_disagreement(got["refined"], true) <= tol()
    assert got["status"] == PG.STATUS_CONVERGED


# ---- sizes: the tile edges of the neighbour test (64 lanes, 256 threads, 4 rounds) and of the landmark loops -----------------------
@pytest.mark.parametrize("boxes", [63, 64, 65, 255, 256, 257, MAX_BOXES])
def test_boxes_per_sample_at_the_tile_edges(boxes):
    s = R.scene(700 + boxes, 4, 14, box_noise=BN, pad_boxes_to=boxes)
    assert sum(len(c) for c in s["corners"]) == boxes
    got, _ = check(s)
    assert got["landmarks"] == 14


@pytest.mark.parametrize("landmarks", [63, 64, 65])
def test_landmarks_at_the_wave_edges(landmarks):
    s = R.scene(800 + landmarks, 3, landmarks, box_noise=BN)
    got, _ = check(s)
    assert got["landmarks"] == landmarks


def test_many_landmarks_use_both_landmark_rounds():
    s = R.scene(870, 3, 300, box_noise=BN, seen=0.7)            # > 256 landmarks: the second landmark per thread
    got, _ = check(s, stationarity=False)
    assert got["landmarks"] == 300


def test_one_box_over_the_limit_is_refused_before_any_launch():
    assert ops.pose_graph_limits() == (MAX_AGENTS, MAX_BOXES)
    assert not ops.pose_graph_supported(2, MAX_BOXES + 1) and not ops.pose_graph_supported(MAX_AGENTS + 1, 4)
    corners = [torch.zeros((MAX_BOXES // 2 + 1, 8, 3), dtype=torch.float64, device=DEV),
               torch.zeros((MAX_BOXES // 2, 8, 3), dtype=torch.float64, device=DEV)]
    pose = torch.zeros((2, 6), dtype=torch.float64, device=DEV)
    before = ops.POSE_CALLS["align"]
    with pytest.raises(_capi.HealAmdError, match="out of range"):
        ops.pose_graph_align(corners, pose, None, [2])
    nine = [torch.zeros((1, 8, 3), dtype=torch.float64, device=DEV)] * (MAX_AGENTS + 1)
    with pytest.raises(_capi.HealAmdError, match="out of range"):
        ops.pose_graph_align(nine, torch.zeros((MAX_AGENTS + 1, 6), dtype=torch.float64, device=DEV), None, [MAX_AGENTS + 1])
    with pytest.raises(_capi.HealAmdError, match="no CPU path"):
        ops.pose_graph_align([c.cpu() for c in corners[:1]], pose[:1].cpu(), None, [1])
    assert ops.POSE_CALLS["align"] == before


# ---- agents that do not take part ----------------------------------------------------------------------------------------------
def test_agents_without_boxes_or_clusters_keep_their_pose_bitwise():
    s = R.scene(901, 5, 8, box_noise=BN, empty_agents=(2,), lonely_agents=(4,))
    got, _ = check(s)
    noisy = s["pose"][:, [0, 1, 4]]
    assert got["refined"][[0, 2, 4]].tobytes() == noisy[[0, 2, 4]].tobytes()
    assert np.all(got["cluster"][R.host_result(s)["cluster_of_box"] < 0] == -1)
    for a in (1, 3):
        assert got["refined"][a].tobytes() != noisy[a].tobytes()


def test_ego_without_an_edge():
    """The solution is a whole orbit (nothing ties the graph to the fixed ego): the final cost and the relative pose of two
    connected agents are compared, not absolute poses.  A pose within d of a minimiser costs at most d^2 trace(H) more."""
    s = R.scene(902, 4, 9, box_noise=BN, lonely_agents=(0,))
    got, want = run([s])[0], R.host_result(s)
    assert np.array_equal(got["cluster"], want["cluster_of_box"]) and got["edges"] == want["active_edges"]
    assert got["refined"][0].tobytes() == s["pose"][0, [0, 1, 4]].tobytes()
    c_dev, _ = R.reduced_cost_and_gradient(s, got["refined"])
    c_host, _ = R.reduced_cost_and_gradient(s, want["refined"])
    trace = R.hessian_trace(want["pgo"])
    print(f"ego without an edge: cost device {c_dev:.15e} host {c_host:.15e}, trace(H) {trace:.3e}")
    assert c_dev <= c_host + 10.0 * R.d_ref() ** 2 * trace
    rel = lambda r: R.relative(np.r_[r[1, :2], np.radians(r[1, 2])], np.r_[r[2, :2], np.radians(r[2, 2])])   # noqa: E731
    d = np.abs(rel(got["refined"]) - rel(want["refined"]))
    d[2] = abs(PG.wrap_angle(d[2]))
    assert d.max() <= tol(), d


# ---- clusters ------------------------------------------------------------------------------------------------------------------
def test_two_boxes_of_one_agent_in_one_cluster():
    s = R.with_twin(R.scene(903, 3, 6, box_noise=BN, seen=1.0), agent=1)
    got, want = check(s)
    k = want["cluster_of_box"][len(s["corners"][0]) + len(s["corners"][1]) - 1]
    assert k >= 0 and np.sum(want["cluster_of_box"][len(s["corners"][0]):len(s["corners"][0]) + len(s["corners"][1])] == k) == 2


def test_yaws_near_pi():
    s = R.scene(904, 4, 10, box_noise=BN, near_pi=True)
    assert np.all(np.abs(np.abs(s["true_pose"][:, 2]) - np.pi) < 0.05)
    check(s)
    check(R.scene(905, 3, 8, near_pi=True))


# ---- options ---------------------------------------------------------------------------------------------------------------------
OPTION_SCENES = {
    "use_uncertainty_false": lambda: R.scene(911, 3, 8, box_noise=BN, opts={"use_uncertainty": False}),
    "no_uncertainty_list": lambda: R.scene(912, 3, 8, box_noise=BN, unc=False),
    "normalize_uncertainty": lambda: R.scene(913, 3, 8, box_noise=BN, opts={"normalize_uncertainty": True}),
    "landmark_xy": lambda: R.scene(914, 3, 8, box_noise=BN, opts={"landmark_SE2": False}),
    "drop_hard_boxes": lambda: R.scene(915, 4, 9, box_noise=BN, yaw_flip_objects=(2, 5), opts={"drop_hard_boxes": True}),
    "drop_unsure_edge": lambda: R.scene(916, 3, 10, box_noise=BN, log_sigma2=(-7.0, -1.0), opts={"drop_unsure_edge": True}),
    "adaptive_landmark_one_varying": lambda: R.scene(917, 4, 9, box_noise=BN, yaw_flip_objects=(3,), opts={"adaptive_landmark": True}),
    "abandon_not_taken": lambda: R.scene(918, 3, 8, box_noise=BN, opts={"abandon_hard_cases": True}),
    "thresholds": lambda: R.scene(919, 3, 8, box_noise=BN, opts={"thres": 1.0, "yaw_var_thres": 0.1}),
}


@pytest.mark.parametrize("name", list(OPTION_SCENES))
def test_each_option_alone(name):
    s = OPTION_SCENES[name]()
    got, want = check(s)
    if name == "drop_unsure_edge":
        assert 0 < got["edges"] < int(np.sum(want["cluster_of_box"] >= 0))
    if name == "drop_hard_boxes":
        assert got["edges"] < int(np.sum(want["cluster_of_box"] >= 0))
    if name == "adaptive_landmark_one_varying":
        kinds = [v[2] for v in want["pgo"].vertex_list() if v[0] >= s["pose"].shape[0]]
        assert kinds.count(False) == 1 and kinds.count(True) >= 1        # SE2 and XY landmarks in one graph


@pytest.mark.parametrize("name", ["abandon_few_landmarks", "abandon_yaw_varies"])
def test_abandon_hard_cases_returns_the_input_bits(name):
    s = R.golden_cases()[name]
    got, want = check(s)
    assert got["status"] == PG.STATUS_ABANDONED and got["iterations"] == 0
    assert got["refined"].tobytes() == s["pose"][:, [0, 1, 4]].tobytes()


def test_max_iterations_bounds_the_solve():
    s = R.scene(920, 3, 8, box_noise=BN)
    got = run([s], max_iterations=2)[0]
    assert got["iterations"] == 2 and got["status"] == PG.STATUS_MAX_ITERATIONS
    assert run([s], max_iterations=10 ** 6)[0]["iterations"] == run([s])[0]["iterations"]


# ---- non-finite input ------------------------------------------------------------------------------------------------------------
def test_nan_corner_returns_the_noisy_pose_with_a_status():
    bad = R.scene(930, 3, 6, box_noise=BN)
    bad["corners"] = [c.copy() for c in bad["corners"]]
    bad["corners"][1][0, 3, 1] = np.nan
    good = R.scene(931, 3, 6, box_noise=BN)
    out = run([bad, good])
    assert out[0]["status"] == PG.STATUS_NONFINITE and out[0]["iterations"] == 0
    assert out[0]["refined"].tobytes() == bad["pose"][:, [0, 1, 4]].tobytes() and np.all(out[0]["cluster"] == -1)
    alone = run([good])[0]                                               # the neighbour in the batch is not touched by it
    assert out[1]["refined"].tobytes() == alone["refined"].tobytes() and out[1]["status"] == PG.STATUS_CONVERGED


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_batch_equals_single_launches_and_launches_repeat_bitwise():
    scenes = [R.scene(941, 2, 7, box_noise=BN), R.scene(942, 5, 20, box_noise=BN, empty_agents=(3,)), R.scene(943, 3, 9, box_noise=BN)]
    batch = run(scenes)
    again = run(scenes)
    for k, s in enumerate(scenes):
        single = run([s])[0]
        for key in ("refined", "cluster"):
            assert batch[k][key].tobytes() == single[key].tobytes() == again[k][key].tobytes(), (k, key)
        for key in ("landmarks", "edges", "iterations", "status", "chi2"):
            assert batch[k][key] == single[key] == again[k][key], (k, key)
        want = R.host_result(s)
        assert R.pose_disagreement(batch[k]["refined"], want["refined"]) <= tol()


# ---- fp32 boxes straight from the stage-1 postprocessor ------------------------------------------------------------------------------
def test_stage1_output_through_box_alignment_relative():
    from heal_amd.opencood.data_utils.post_processor.uncertainty_voxel_postprocessor import UncertaintyVoxelPostprocessor
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unc_post.npz"))
    p = configs.lidar_uncertainty([float(v) for v in g["sq_range"]])["postprocess"]
    p["gt_range"] = [float(v) for v in g["gt_range"]]
    post = UncertaintyVoxelPostprocessor(p, train=False)
    stage1 = {k: torch.from_numpy(g[f"st_{k}"]).to(DEV) for k in ("cls_preds", "reg_preds", "unc_preds", "dir_preds")}
    assert stage1["cls_preds"].shape[-2:] == (16, 16)
    with torch.no_grad():
        corners, _, uncs = post.post_process_stage1(stage1, torch.from_numpy(g["st_anchors"]).to(DEV))
    assert len(corners) == 2 and all(c.dtype == torch.float32 and c.is_cuda and c.shape[0] > 0 for c in corners)
    corners, uncs = list(corners) + [None], list(uncs) + [None]           # and a third agent that detected nothing
    poses = torch.tensor([[0.0, 0.0, 0.3, 0.0, 10.0, 0.0], [0.4, -0.3, 0.2, 0.0, 11.0, 0.0], [5.0, 5.0, 0.0, 0.0, 90.0, 0.0]],
                         dtype=torch.float64)
    record_len = torch.tensor([3])
    out = BA.box_alignment_relative(corners, uncs, poses, record_len)
    refined, stats, _ = ops.pose_graph_align(corners, poses, uncs, record_len, return_stats=True)
    assert out.shape == (3, 6) and out.dtype == torch.float64 and out.is_cuda
    assert torch.equal(out[:, [0, 1, 4]], refined) and torch.equal(out[:, [2, 3, 5]].cpu(), poses[:, [2, 3, 5]])
    assert out[2, [0, 1, 4]].cpu().numpy().tobytes() == poses[2, [0, 1, 4]].numpy().tobytes()
    # the same boxes as float64 through the host path: the integer results agree when the fixture's margins allow the comparison
    host = [c.double().cpu().numpy() if c is not None else np.zeros((0, 8, 3)) for c in corners]
    hunc = [u.double().cpu().numpy() if u is not None else np.zeros((0, 3)) for u in uncs]
    graph = R.assert_comparable(host, poses.numpy(), hunc, {})
    assert int(stats["landmarks"][0]) == graph["landmarks"] and int(stats["edges"][0]) == graph["active_edges"]
