"""The host path of CoAlign's box alignment (heal_amd/opencood/models/sub_modules/{box_align_v2,pose_graph_optim}.py) on the CPU:
its graph against what the reference builds (tests/golden/pose_graph.npz, recorded through a stand-in for g2o), its minimiser
against scipy's on the same cost, and the plumbing of the device entry points (header, binding, support rule).

d_ref, measured 2026-10 on the build machine (scipy 1.15, the nine scenes of posegraph_refs.tolerance_scenes()): 3.2e-8 (metres /
radians) -- scipy's trust-region solver stops at the resolution of the cost (~sqrt(eps)), the host optimiser goes on to the
rounding of the gradient; with noise-free boxes the two agree to 7e-15.  The GPU test's tolerance is 10 x the recorded figure.
"""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heal_amd import _capi
from heal_amd.opencood.models.sub_modules import box_align_v2 as BA
from heal_amd.opencood.models.sub_modules import pose_graph_optim as PG
from tests import posegraph_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph.npz")
REF_ROOT = "/root/reference"
HAVE_REFERENCE = os.path.isdir(os.path.join(REF_ROOT, "opencood"))
SYMBOLS = ["heal_pose_graph_align", "heal_pose_graph_supported", "heal_pose_graph_workspace"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name):
    g = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    counts = g["counts"]
    split = np.cumsum(counts)[:-1]
    corners = np.split(g["corners"], split)
    unc = np.split(g["unc"], split) if bool(g["has_unc"]) else None
    return g, corners, unc, json.loads(str(g["opts"]))


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= 1e-12 * np.abs(b))


# ---- 1. the graph -----------------------------------------------------------------------------------------------------------------
def test_golden_covers_every_option(golden):
    names = [str(n) for n in golden["names"]]
    assert names == list(R.golden_cases())
    seen = set()
    for n in names:
        seen |= set(_case(golden, n)[3])
    assert {"use_uncertainty", "normalize_uncertainty", "landmark_SE2", "adaptive_landmark", "abandon_hard_cases", "drop_hard_boxes",
            "drop_unsure_edge", "thres", "yaw_var_thres"} <= seen
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", list(R.golden_cases()))
def test_graph_equals_the_reference(golden, name):
    g, corners, unc, opts = _case(golden, name)
    # the committed inputs are the generator's scene, bit for bit
    s = R.golden_cases()[name]
    assert np.array_equal(np.concatenate(s["corners"]), g["corners"]) and np.array_equal(s["pose"], g["pose"])
    pose = g["pose"].copy()
    built = BA.build_pose_graph(corners, pose, unc, **{**R.OPTION_DEFAULTS, **opts})
    assert np.array_equal(pose, g["pose"])                       # the input is not modified
    if len(g["vid"]) == 0:                                       # the reference abandoned the sample
        assert built["pgo"] is None
        out = BA.box_alignment_relative_sample_np(corners, pose, unc, **opts)
        assert out.tobytes() == g["returned"].tobytes() == g["pose"][:, [0, 1, 4]].tobytes()
        return
    verts, edges = built["pgo"].vertex_list(), built["pgo"].edge_list()
    assert [v[0] for v in verts] == g["vid"].tolist()
    assert [v[1] for v in verts] == g["vfixed"].tolist()
    assert [v[2] for v in verts] == g["vse2"].tolist()
    for k, (_, _, se2, est) in enumerate(verts):
        d = 3 if se2 else 2
        want = g["vest"][k, :d].copy()
        if se2:
            want[2] = PG.wrap_angle(want[2])                      # the stand-in keeps the angle as given; SE2 wraps it
        assert len(est) == d and np.all(np.isnan(g["vest"][k, d:])) and _close(est, want), (name, k, est, want)
    assert [list(e[0]) for e in edges] == g["eij"].tolist()
    assert [e[1] for e in edges] == g["ese2"].tolist()
    for k, (_, se2, meas, info) in enumerate(edges):
        d = 3 if se2 else 2
        want = g["emeas"][k, :d].copy()
        if se2:
            want[2] = PG.wrap_angle(want[2])
        assert _close(meas, want), (name, k, meas, want)
        assert info.shape == (d, d) and _close(info, g["einfo"][k, :d, :d]), (name, k)
    assert built["active_edges"] == len(edges) and built["landmarks"] == len(verts) - len(g["counts"])


# ---- 2. the minimiser against a second solver --------------------------------------------------------------------------------------
def test_minimiser_against_scipy_and_record_d_ref():
    per_scene = {str(s["seed"]): R.mirror_vs_scipy(s) for s in R.tolerance_scenes()}
    d_ref = max(per_scene.values())
    print("pose graph: host optimiser vs scipy.optimize.least_squares, largest pose disagreement per scene:", per_scene)
    os.makedirs(os.path.dirname(R.TOLERANCE_FILE), exist_ok=True)
    with open(R.TOLERANCE_FILE, "w") as f:
        json.dump({"d_ref": d_ref, "per_scene": per_scene, "unit": "metres / radians",
                   "what": "largest agent-pose disagreement between pose_graph_optim.PoseGraphOptimization2D and "
                           "scipy.optimize.least_squares (xtol = ftol = gtol = 1e-15) on the same cost from the same start"},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    # two solvers of one cost: the figure is recorded, and a disagreement above a millimetre would mean they minimise different things
    assert 0.0 < d_ref < 1e-3, per_scene
    for s in R.tolerance_scenes():
        h = R.host_result(s)
        assert h["status"] == PG.STATUS_CONVERGED and h["iterations"] < 100, (s["seed"], h["status"], h["iterations"])


def test_cost_and_gradient_agree_with_finite_differences():
    s = R.scene(301, 3, 6, box_noise=(0.1, 0.02), yaw_flip_objects=(1,), opts={"adaptive_landmark": True})
    pgo = R.rebuilt_graph(s)
    grad = pgo.gradient()
    assert any(not v[2] for v in pgo.vertex_list()) and any(v[2] for v in pgo.vertex_list() if v[0] >= 3)   # XY and SE2 landmarks
    for vid, g in grad.items():
        for k in range(len(g)):
            est = pgo._vertices[vid]["estimate"]
            keep, h = est[k], 1e-6
            est[k] = keep + h
            up = pgo.chi2()
            est[k] = keep - h
            dn = pgo.chi2()
            est[k] = keep
            assert abs((up - dn) / (2 * h) - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (vid, k)


# ---- 3. noise-free boxes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agents", [2, 3, 5, 8])
def test_noise_free_boxes_recover_the_true_poses(agents):
    s = R.scene(400 + agents, agents, 4 * agents)
    true = np.c_[s["true_pose"][:, :2], np.degrees(s["true_pose"][:, 2])]
    assert R.pose_disagreement(s["pose"][:, [0, 1, 4]], true) > 0.05          # the start is off
    out = BA.box_alignment_relative_sample_np(s["corners"], s["pose"], s["unc"])
    assert R.pose_disagreement(out, true) < 1e-9
    assert np.all(out[:, 2] > -180.0) and np.all(out[:, 2] <= 180.0)


# ---- 4. / 5. exits that return the input ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["abandon_few_landmarks", "abandon_yaw_varies"])
def test_abandon_hard_cases_returns_the_input_bits(name):
    s = R.golden_cases()[name]
    out = BA.box_alignment_relative_sample_np(s["corners"], s["pose"], s["unc"], **s["opts"])
    assert out.tobytes() == s["pose"][:, [0, 1, 4]].tobytes()
    taken = R.golden_cases()["abandon_not_taken"]
    moved = BA.box_alignment_relative_sample_np(taken["corners"], taken["pose"], taken["unc"], **taken["opts"])
    assert moved.tobytes() != taken["pose"][:, [0, 1, 4]].tobytes()


def test_agents_without_edges_and_samples_without_clusters_return_the_noisy_poses():
    s = R.scene(501, 4, 6, box_noise=(0.1, 0.02), empty_agents=(2,), lonely_agents=(3,))
    out = BA.box_alignment_relative_sample_np(s["corners"], s["pose"], s["unc"])
    noisy = s["pose"][:, [0, 1, 4]]
    assert out[[0, 2, 3]].tobytes() == noisy[[0, 2, 3]].tobytes()            # the fixed ego, the empty agent, the lonely agent
    assert out[1].tobytes() != noisy[1].tobytes()
    lonely = R.scene(502, 3, 0, lonely_agents=(0, 1, 2))                       # boxes, but no two within the threshold
    assert lonely["graph"]["landmarks"] == 0 and sum(len(c) for c in lonely["corners"]) == 6
    assert BA.box_alignment_relative_sample_np(lonely["corners"], lonely["pose"], lonely["unc"]).tobytes() == \
        lonely["pose"][:, [0, 1, 4]].tobytes()
    empty = [np.zeros((0, 8, 3))] * 2
    pose = np.array([[1.0, 2.0, 0.0, 0.0, 30.0, 0.0], [4.0, 5.0, 0.0, 0.0, -170.0, 0.0]])
    assert BA.box_alignment_relative_sample_np(empty, pose, None).tobytes() == pose[:, [0, 1, 4]].tobytes()
    out = BA.box_alignment_relative_np(s["corners"] + empty, s["unc"] + [np.zeros((0, 3))] * 2, np.concatenate([s["pose"], pose]), [4, 2])
    assert out.shape == (6, 3) and out[4:].tobytes() == pose[:, [0, 1, 4]].tobytes()


def test_yaw_is_normalised_for_every_agent():
    s = R.scene(503, 3, 6, box_noise=(0.1, 0.02))
    pose = s["pose"].copy()
    pose[:, 4] += 360.0                                                          # the same poses, yaws outside (-180, 180]
    out = BA.box_alignment_relative_sample_np(s["corners"], pose, s["unc"])
    ref = BA.box_alignment_relative_sample_np(s["corners"], s["pose"], s["unc"])
    assert np.all(out[:, 2] > -180.0) and np.all(out[:, 2] <= 180.0)
    assert R.pose_disagreement(out, ref) < 1e-9


# ---- 6. signature ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_REFERENCE, reason="reference tree not present")
def test_signatures_and_defaults_equal_the_reference():
    import ast
    with open(os.path.join(REF_ROOT, "opencood", "models", "sub_modules", "box_align_v2.py")) as f:
        tree = ast.parse(f.read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name in ("box_alignment_relative_sample_np", "box_alignment_relative_np"):
        a = fns[name].args
        names = [x.arg for x in a.args]
        defaults = [ast.literal_eval(d) for d in a.defaults]
        ours = inspect.signature(getattr(BA, name))
        assert [p for p in ours.parameters if ours.parameters[p].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD] == names
        got = [p.default for p in ours.parameters.values() if p.default is not inspect.Parameter.empty]
        assert got == defaults and [type(x) for x in got] == [type(x) for x in defaults]
        assert (a.kwarg is not None) == any(p.kind == inspect.Parameter.VAR_KEYWORD for p in ours.parameters.values())
    with open(os.path.join(REF_ROOT, "opencood", "models", "sub_modules", "pose_graph_optim.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PoseGraphOptimization2D")
    for m in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
        ours = inspect.signature(getattr(PG.PoseGraphOptimization2D, m.name))
        assert list(ours.parameters) == [x.arg for x in m.args.args], m.name


# ---- the host path stays off the GPU; plumbing of the device path ---------------------------------------------------------------------
def test_host_path_does_not_initialise_a_gpu():
    code = ("import numpy as np, torch\n"
            "from tests import posegraph_refs as R\n"
            "from heal_amd.opencood.models.sub_modules import box_align_v2 as BA\n"
            "s = R.scene(7, 3, 5, box_noise=(0.1, 0.02))\n"
            "BA.box_alignment_relative_sample_np(s['corners'], s['pose'], s['unc'])\n"
            "assert not torch.cuda.is_initialized()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pose_header_is_bound():
    sig = _capi.signatures_pose()
    assert sorted(sig) == SYMBOLS
    with open(_capi.HEADER_POSE) as f:
        text = f.read()
    assert sorted(set(re.findall(r"\b(heal_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))) == SYMBOLS
    res, args = sig["heal_pose_graph_align"]
    assert res is ctypes.c_int and len(args) == 20 and args[:5] == [ctypes.c_void_p] * 5 and args[5:11] == [ctypes.c_int] * 6
    assert args[11:13] == [ctypes.c_double] * 2 and args[13] is ctypes.c_int and args[14:18] == [ctypes.c_void_p] * 4
    assert sig["heal_pose_graph_workspace"][0] is ctypes.c_size_t
    lib = _capi.lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert not set(sig) & set(_capi.signatures())                       # outside the versioned inference ABI
    for name, value in (("STATUS_CONVERGED", 0), ("STATUS_MAX_ITERATIONS", 1), ("STATUS_NO_EDGES", 2), ("STATUS_ABANDONED", 3),
                        ("STATUS_NONFINITE", 4)):
        assert _capi.header_define("HEAL_POSE_" + name, _capi.HEADER_POSE) == value == getattr(PG, name)
    assert _capi.header_define("HEAL_POSE_MAX_ITERATIONS", _capi.HEADER_POSE) == PG.MAX_ITERATIONS


def test_support_and_workspace_rules():
    from heal_amd import ops
    A, B = ops.pose_graph_limits()
    assert (A, B) == (8, 1024)
    for a, b in ((1, 0), (1, 5), (A, B), (2, B)):
        assert ops.pose_graph_supported(a, b), (a, b)
    for a, b in ((0, 4), (A + 1, 4), (2, B + 1), (2, -1)):
        assert not ops.pose_graph_supported(a, b), (a, b)
    q = lambda *v: _capi.query("heal_pose_graph_workspace", *v)             # noqa: E731
    assert q(1, 2, 0) > 0 and q(3, 10, 300) > q(3, 10, 100) > 0
    assert q(0, 0, 0) == 0 and q(1, 9, 4) == 0 and q(1, 2, B + 1) == 0 and q(2, 1, 4) == 0
