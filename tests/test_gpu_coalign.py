"""CoAlign multiscale fusion on the MI355X: heal_warp_att_fuse_levels against the reference arithmetic in fp64 (bound: 4 x the
error of the reference's own fp32 composition on the device, ceiling 1e-4), the fixture cases and the end-to-end model against the
reference's goldens, refusals, launch-to-launch bit equality, captured-graph replay on another scene, and the gradient path."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, configs, ops, synth
from tests.golden.detfill import fill_module
from tests.test_coalign_cpu import CASES, E2E_RANGE, case_inputs, e2e_data, load_golden, make_fusion_net, rel_err

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]
DEV = "cuda:0"
FULL = [(64, 256, 256), (128, 128, 128), (256, 64, 64)]          # lidar_coalign.yaml on the full range
DAIR = [(64, 128, 256), (128, 64, 128), (256, 32, 64)]           # the DAIR-V2X range


def scene_inputs(n, levels, seed, map_m, r_max):
    """Scaled inputs (randn * C^(-1/4): the ego does not dominate the softmax) and one set of normalised affine rows [n, 2, 3]."""
    from oracle import oracle_np as O
    gen = torch.Generator().manual_seed(seed)
    feats = [(torch.randn((n, C, H, W), generator=gen) * C ** -0.25).to(DEV) for C, H, W in levels]
    pw = synth.pairwise_t_matrix(synth.agent_poses(seed, n, r_min=4.0, r_max=r_max), max(n, 5))[None]
    aff = O.normalize_pairwise_tfm(pw, map_m[0], map_m[1], 1)
    return feats, np.ascontiguousarray(aff[0][0, :n])


def reference_level(x, rows, mode, dtype):
    """fusion_in_one.py:87-151 for one scene and level in `dtype` on the device.  The sampling grid is built in the affine matrix's
    dtype (fp64) and rounded to fp32, as warp_affine_simple's `.to(src)` rounds it for an fp32 map, in BOTH precisions: the fp64
    oracle then samples where the fp32 run samples."""
    n, C, H, W = x.shape
    M = torch.as_tensor(rows, dtype=torch.float64, device=x.device)
    grid = F.affine_grid(M, [n, C, H, W], align_corners=False).to(torch.float32).to(dtype)
    ego = F.grid_sample(x.to(dtype), grid, align_corners=False)
    if mode == "max":
        return ego.max(dim=0)[0]
    t = ego.view(n, C, -1).permute(2, 0, 1)
    attn = torch.softmax(torch.bmm(t, t.transpose(1, 2)) / float(np.sqrt(C)), -1)
    return torch.bmm(attn, t).permute(1, 2, 0).view(n, C, H, W)[0]


def check_vs_fp64(feats, rows, mode, what, affine=None):
    with torch.no_grad():
        got = ops.warp_att_fuse_levels(feats, rows if affine is None else affine, True, mode)
        for l, x in enumerate(feats):
            oracle = reference_level(x, rows, mode, torch.float64).cpu().numpy()
            e_ref = rel_err(reference_level(x, rows, mode, torch.float32).double().cpu().numpy(), oracle)
            e_ker = rel_err(got[l].double().cpu().numpy(), oracle)
            print(f"{what} level {l} {tuple(x.shape)} {mode}: kernel vs fp64 {e_ker:.2e}, torch fp32 composition vs fp64 {e_ref:.2e}")
            assert tuple(got[l].shape) == tuple(x.shape[1:])
            assert e_ker <= 1e-4, (what, l, e_ker)
            assert e_ker <= 4 * e_ref, (what, l, e_ker, e_ref)
    return got


@pytest.mark.parametrize("mode", ["att", "max"])
def test_full_size_three_levels_one_launch_vs_fp64(mode):
    feats, rows = scene_inputs(5, FULL, 21, (204.8, 204.8), 60.0)
    check_vs_fp64(feats, rows, mode, "full size, 5 agents")


def test_dair_shapes_vs_fp64():
    feats, rows = scene_inputs(2, DAIR, 22, (102.4, 204.8), 40.0)
    check_vs_fp64(feats, rows, "att", "DAIR-V2X, 2 agents")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_agent_counts_vs_fp64(n):
    feats, rows = scene_inputs(n, [(64, 24, 40), (128, 12, 20), (256, 6, 10)], 30 + n, (38.4, 64.0), 20.0)
    check_vs_fp64(feats, rows, "att", f"{n} agents")
    check_vs_fp64(feats, rows, "max", f"{n} agents")


def test_odd_sizes_and_channel_counts_vs_fp64():
    feats, rows = scene_inputs(5, [(64, 37, 53), (128, 19, 27), (256, 9, 13), (40, 5, 3)], 41, (59.2, 84.8), 30.0)
    check_vs_fp64(feats, rows, "att", "odd sizes, 4 levels")


def test_one_level_alone_and_device_affines_vs_fp64():
    feats, rows = scene_inputs(5, [(128, 50, 70)], 42, (80.0, 112.0), 40.0)
    host = check_vs_fp64(feats, rows, "att", "one level")
    dev = check_vs_fp64(feats, rows, "att", "one level, device affines", affine=torch.from_numpy(rows).to(DEV))
    assert torch.equal(host[0], dev[0])


def test_far_agents_keep_their_softmax_share():
    """Poses out to beyond the map: most neighbour pixels are out of reach, whole waves skip those agents' loads, and the zero
    logit still takes part in the softmax (dropping it would move the output by tenths of its maximum: tests/test_coalign_cpu.py)."""
    feats, rows = scene_inputs(5, [(64, 96, 96), (128, 48, 48), (256, 24, 24)], 43, (76.8, 76.8), 90.0)
    check_vs_fp64(feats, rows, "att", "far agents")


def test_two_launches_are_bit_equal():
    feats, rows = scene_inputs(5, [(64, 100, 90), (128, 50, 45), (256, 25, 23)], 44, (80.0, 72.0), 30.0)
    with torch.no_grad():
        a = ops.warp_att_fuse_levels(feats, rows)
        b = ops.warp_att_fuse_levels(feats, rows)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals():
    f = lambda n, C=16, dt=torch.float32: torch.zeros((n, C, 8, 8), dtype=dt, device=DEV)   # noqa: E731
    rows = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (9, 1, 1))
    with torch.no_grad():
        ops.warp_att_fuse_levels([f(8)], rows[:8])
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(9)], rows)                                   # 9 agents
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3), f(2)], rows[:3])                         # levels of different agent counts
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3, dt=torch.float16)], rows[:3])             # not fp32
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3)] * 5, rows[:3])                           # more than 4 levels
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([], rows[:3])
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3)], rows[:2])                               # affine rows for another agent count
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3)], rows[:3], mode="mean")
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels([f(3).cpu()], rows[:3])


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.mark.parametrize("prefix", sorted(CASES))
def test_fixture_case_on_device_matches_reference(g, prefix, monkeypatch):
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import fuse_levels, ms_fused_ok
    net = make_fusion_net(prefix)
    feats, rl, aff = case_inputs(g, prefix)
    feats = [f.to(DEV) for f in feats]
    with torch.no_grad():
        assert ms_fused_ok(net, feats, [int(v) for v in rl])
        fused = fuse_levels(net, feats, rl, aff)
        monkeypatch.setenv("HEAL_MSATT_FUSED", "0")
        assert not ms_fused_ok(net, feats, [int(v) for v in rl])
        plain = fuse_levels(net, feats, rl, aff)
    for l in range(len(feats)):
        want = g[f"{prefix}out{l}"]
        e_f, e_p = rel_err(fused[l].cpu().numpy(), want), rel_err(plain[l].cpu().numpy(), want)
        print(f"{prefix} level {l}: fused {e_f:.2e}, torch on the device {e_p:.2e}")
        assert e_f <= 1e-3 and e_p <= 1e-3, (l, e_f, e_p)


@pytest.mark.parametrize("prefix,method", [("e2e_", "att"), ("e2emax_", "max")])
def test_model_on_device_matches_reference(g, prefix, method, monkeypatch):
    from heal_amd.opencood.models.fuse_modules import fusion_in_one
    from heal_amd.opencood.tools.train_utils import create_model
    model = fill_module(create_model(configs.lidar_coalign(method, E2E_RANGE))).to(DEV).eval()
    data = e2e_data(g)
    data["inputs_m1"] = {k: v.to(DEV) for k, v in data["inputs_m1"].items()}
    data["pairwise_t_matrix"] = data["pairwise_t_matrix"].to(DEV)
    taken = []
    real = fusion_in_one.ms_fused_ok
    monkeypatch.setattr(fusion_in_one, "ms_fused_ok", lambda *a: taken.append(real(*a)) or taken[-1])
    for fused in ("1", "0"):
        monkeypatch.setenv("HEAL_MSATT_FUSED", fused)
        with torch.no_grad():
            out = model(data)
        assert taken[-1] == (fused == "1")
        for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
            e = rel_err(out[key].cpu().numpy(), g[f"{prefix}{name}"])
            assert e <= 1e-3, (fused, key, e)


def test_coalign_pipeline_graph_replay_equals_eager():
    from heal_amd.pipeline import Scene, ScenePipeline
    pipe = ScenePipeline(configs.lidar_coalign("att", SMALL_RANGE), DEV, seed=3)
    scene, other = Scene(3, seed=31, device=DEV), Scene(3, seed=32, device=DEV)
    for s, seed in ((scene, 31), (other, 32)):
        s.points = {k: p[(p[:, 0].abs() < 28) & (p[:, 1].abs() < 28)][:6000].contiguous() for k, p in s.points.items()}
        s.pairwise = synth.pairwise_t_matrix(synth.agent_poses(seed, 3, r_min=3.0, r_max=10.0), 5)[None]
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
        pipe.calibrate_cls_bias(other, 300)
        eager = pipe.forward(other)
        eager = {k: eager[k].clone() for k in ("cls_preds", "reg_preds", "dir_preds")}
        eb, es = pipe.step(other)
        pipe.capture(scene, warmup=1)
        pipe.replay(other)
        gb, gs = pipe.replay(other)
        _capi.guard_check(getattr(pipe, "_guard", []), "CoAlign replay")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in eager.values())
    assert tuple(eager["cls_preds"].shape) == (1, 2, 64, 64)
    assert (gb is None) == (eb is None)
    print("boxes on the replayed scene:", None if eb is None else int(eb.shape[0]))
    if eb is not None:
        assert gb.shape == eb.shape and torch.allclose(gb, eb, atol=1e-3) and torch.allclose(gs, es, atol=1e-4)


@pytest.mark.grad
def test_gradient_path_on_device_matches_cpu(g):
    """Under autograd fuse_levels runs the reference's torch arithmetic on the device: the golden outputs, and the gradients of
    every level's input equal the CPU's within 1e-4."""
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import fuse_levels
    grads = {}
    for dev in ("cpu", DEV):
        net = make_fusion_net("n3_")
        feats, rl, aff = case_inputs(g, "n3_")
        feats = [f.to(dev).requires_grad_(True) for f in feats]
        out = fuse_levels(net, feats, rl, aff)
        for l, y in enumerate(out):
            assert rel_err(y.detach().cpu().numpy(), g[f"n3_out{l}"]) <= 1e-4, (dev, l)
        sum(y.square().mean() for y in out).backward()
        grads[dev] = [f.grad.cpu().numpy() for f in feats]
    for l, (a, b) in enumerate(zip(grads[DEV], grads["cpu"])):
        assert float(np.abs(b).max()) > 0 and rel_err(a, b) <= 1e-4, l
