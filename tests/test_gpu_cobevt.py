"""CoBEVT fusion on the MI355X: heal_agent_window_attention against an fp64 restatement of the reference's Attention
(swap_fusion_modules.py:86-131), the module and the end-to-end model against the reference's goldens (tests/golden/cobevt_small.npz),
the full-size HIP path against the module's own torch path in fp64, a captured-graph replay, and the gradient path on the device."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.golden.detfill import fill_module

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]        # the end-to-end case of cobevt_small.npz
COBEVT_ARGS = {"input_dim": 256, "mlp_dim": 256, "agent_size": 5, "window_size": 4, "dim_head": 32, "drop_out": 0.1, "depth": 3}
HEADS, D, WS = 8, 32, 4


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _groups(t, mode, L, H, W):
    """[L, H, W, c] -> [groups, T = 16 L, c] in the reference's (l w1 w2) token order."""
    c = t.shape[-1]
    X, Y = H // WS, W // WS
    if mode == "window":     # 'b m d (x w1) (y w2) -> (b x y) (m w1 w2) d'
        return t.view(L, X, WS, Y, WS, c).permute(1, 3, 0, 2, 4, 5).reshape(X * Y, L * 16, c)
    return t.view(L, WS, X, WS, Y, c).permute(2, 4, 0, 1, 3, 5).reshape(X * Y, L * 16, c)   # 'b m d (w1 x) (w2 y) -> ..'


def _ungroup(o, mode, L, H, W):
    c = o.shape[-1]
    X, Y = H // WS, W // WS
    if mode == "window":
        return o.view(X, Y, L, WS, WS, c).permute(2, 0, 3, 1, 4, 5).reshape(L, H, W, c)
    return o.view(X, Y, L, WS, WS, c).permute(2, 3, 0, 4, 1, 5).reshape(L, H, W, c)


def attention_fp64(qkv, bias, n_valid, mode, scale):
    """swap_fusion_modules.py:86-131 without the projections, in fp64: qkv [L,H,W,768] -> [L,H,W,256]."""
    L, H, W, _ = qkv.shape
    g = _groups(qkv.double(), mode, L, H, W)                       # [G, T, 768]
    G, T = g.shape[:2]
    q, k, v = (g[..., i * 256:(i + 1) * 256].reshape(G, T, HEADS, D).permute(0, 2, 1, 3) for i in range(3))
    sim = torch.einsum("bhid,bhjd->bhij", q * scale, k) + bias.double()[None]
    key_ok = (torch.arange(T, device=qkv.device) // 16) < n_valid
    sim = sim.masked_fill(~key_ok[None, None, None, :], -float("inf"))
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), v)      # masked keys: their V is never weighted
    return _ungroup(out.permute(0, 2, 1, 3).reshape(G, T, HEADS * D), mode, L, H, W)


def _bias(L, seed):
    from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import _relative_position_index
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(((2 * L - 1) * 49, HEADS), generator=gen)
    return table[_relative_position_index(L, WS)].permute(2, 0, 1).contiguous().cuda()


KERNEL_CASES = [(m, L, n, 32) for m in ("window", "grid") for L in (2, 5) for n in range(1, L + 1)] + \
               [(m, 5, n, 128) for m in ("window", "grid") for n in (3, 5)] + [("grid", 2, 1, 128)]


@pytest.mark.parametrize("mode,L,n_valid,hw", KERNEL_CASES)
def test_agent_window_attention_matches_fp64(mode, L, n_valid, hw):
    from heal_amd import ops
    gen = torch.Generator().manual_seed(1000 * L + 10 * n_valid + hw)
    qkv = torch.randn((L, hw, hw, 3 * HEADS * D), generator=gen).cuda()
    bias = _bias(L, n_valid)
    scale = D ** -0.5
    got = ops.agent_window_attention(qkv, bias, n_valid, mode, HEADS, D, WS, scale)
    want = attention_fp64(qkv, bias, n_valid, mode, scale)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(got).any())
    # every query row, the padded agents' included
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) <= 1e-5
    for l in range(L):
        assert rel_err(got[l].cpu().numpy(), want[l].cpu().numpy()) <= 1e-5, l


@pytest.mark.parametrize("mode,L,n_valid", [("window", 5, 3), ("grid", 5, 1), ("grid", 2, 1)])
def test_agent_window_attention_ignores_masked_keys(mode, L, n_valid):
    """K (and V) of masked agents set to NaN: the reference masks their scores, so its result is unaffected -- and so is ours."""
    from heal_amd import ops
    gen = torch.Generator().manual_seed(7 + L + n_valid)
    qkv = torch.randn((L, 32, 32, 3 * HEADS * D), generator=gen).cuda()
    bias = _bias(L, 3)
    scale = D ** -0.5
    want = attention_fp64(qkv, bias, n_valid, mode, scale)
    qkv[n_valid:, :, :, 256:] = float("nan")
    got = ops.agent_window_attention(qkv, bias, n_valid, mode, HEADS, D, WS, scale)
    assert not bool(torch.isnan(got).any())
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) <= 1e-5


def test_agent_window_attention_rejects_bad_inputs():
    from heal_amd import _capi, ops
    qkv = torch.zeros((2, 16, 16, 768), device="cuda")
    bias = torch.zeros((HEADS, 32, 32), device="cuda")
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention(qkv, bias, 0, "window", HEADS, D, WS, 1.0)
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention(qkv, bias, 3, "window", HEADS, D, WS, 1.0)
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention(qkv, bias, 1, "diagonal", HEADS, D, WS, 1.0)
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention(qkv, bias[:, :16], 1, "grid", HEADS, D, WS, 1.0)
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention(qkv[:, :, :14], bias, 1, "grid", HEADS, D, WS, 1.0)


def test_agent_mean_matches_torch():
    from heal_amd import ops
    x = torch.randn((5, 32, 32, 256), device="cuda")
    assert rel_err(ops.agent_mean(x).cpu().numpy(), x.double().mean(0).cpu().numpy()) <= 1e-6


class _Count:
    def __init__(self, monkeypatch):
        from heal_amd import ops
        self.n = 0
        real = ops.agent_window_attention

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, "agent_window_attention", counted)


def _x(g, prefix):
    """The module cases' feature maps are stored as int8 codes (exact in fp32 after the scale)."""
    return g[f"{prefix}x_code"].astype(np.float32) / np.float32(g["x_scale"])


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cobevt_small.npz"))


def _cobevt(agent_size):
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import CoBEVT
    return fill_module(CoBEVT(dict(COBEVT_ARGS, agent_size=agent_size))).cuda().eval()


@pytest.mark.parametrize("prefix", ["l5n5_", "l5n3_", "l2n1_", "b2_"])
def test_cobevt_module_on_device_matches_reference(g, prefix, monkeypatch):
    from oracle import oracle_np as O
    calls = _Count(monkeypatch)
    model = _cobevt(int(g[f"{prefix}agent_size"]))
    aff = O.normalize_pairwise_tfm(g[f"{prefix}pairwise"], *g["HW_m"], 1)
    x = torch.from_numpy(_x(g, prefix)).cuda()
    got = model(x, torch.from_numpy(g[f"{prefix}record_len"]), aff).cpu().numpy()
    n_scenes = len(g[f"{prefix}record_len"])
    assert calls.n == 2 * 3 * n_scenes          # window + grid attention, 3 blocks, per scene
    assert rel_err(got, g[f"{prefix}out"]) <= 1e-3, rel_err(got, g[f"{prefix}out"])
    # the dist tail's entry point: fuse_warped on an already-warped stack
    if n_scenes == 1:
        from heal_amd.opencood.models.fuse_modules.fusion_in_one import warp_to_ego
        n = int(g[f"{prefix}record_len"][0])
        ego = warp_to_ego(x, aff[0][0, :n], True)
        assert rel_err(model.fuse_warped(ego).cpu().numpy(), g[f"{prefix}out"][0]) <= 1e-3


def test_heter_model_baseline_cobevt_on_device_matches_reference(g, monkeypatch):
    from heal_amd import configs
    from heal_amd.opencood.tools.train_utils import create_model
    calls = _Count(monkeypatch)
    model = fill_module(create_model(configs.lidar_baseline("cobevt", E2E_RANGE))).cuda().eval()
    data = {"inputs_m1": {"voxel_features": torch.from_numpy(g["e2e_voxel_features"]).cuda(),
                          "voxel_coords": torch.from_numpy(g["e2e_voxel_coords"]).to(torch.int32).cuda(),
                          "voxel_num_points": torch.from_numpy(g["e2e_voxel_num_points"]).to(torch.int32).cuda()},
            "agent_modality_list": ["m1", "m1"], "record_len": torch.tensor([2]),
            "pairwise_t_matrix": torch.from_numpy(g["e2e_pairwise"]).cuda()}
    out = model(data)
    assert calls.n == 6
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].cpu().numpy(), g[f"e2e_{name}"])
        assert e < 1e-3, (key, e)


@pytest.mark.parametrize("n", [5, 3])
def test_cobevt_full_size_hip_vs_torch_fp64(n, monkeypatch):
    """5 agents, +-102.4 m: the 128 x 128 fusion map of lidar_cobevt.yaml.  The fusion + detection heads on the HIP path against the
    same module's torch path in fp64 on the device."""
    from heal_amd import configs, synth
    from heal_amd.opencood.tools.train_utils import create_model
    from oracle import oracle_np as O
    model = fill_module(create_model(configs.lidar_baseline("cobevt"))).cuda().eval()
    gen = torch.Generator().manual_seed(40 + n)
    x = (torch.randn((n, 256, 128, 128), generator=gen) * 0.5).cuda()
    pw = synth.pairwise_t_matrix(synth.agent_poses(50 + n, n, r_min=5.0, r_max=40.0), 5)[None]
    aff = O.normalize_pairwise_tfm(pw, 204.8, 204.8, 1)
    calls = _Count(monkeypatch)
    fused = model.fusion_net(x, torch.tensor([n]), aff)
    assert calls.n == 6
    heads = [model.cls_head, model.reg_head]
    got = [h(fused).cpu().numpy() for h in heads]
    f64 = copy.deepcopy(model.fusion_net).double()
    ref = f64(x.double(), torch.tensor([n]), aff)
    assert calls.n == 6                             # fp64: the torch composition
    want = [copy.deepcopy(h).double()(ref).cpu().numpy() for h in heads]
    for a, b, name in zip(got, want, ("cls", "reg")):
        assert rel_err(a, b) <= 1e-3, (name, rel_err(a, b))


def test_cobevt_pipeline_graph_replay_equals_eager():
    from heal_amd import configs
    from heal_amd.pipeline import Scene, ScenePipeline
    hypes = configs.lidar_baseline("cobevt", SMALL_RANGE)
    pipe = ScenePipeline(hypes, "cuda:0", seed=3)
    from heal_amd import synth
    scene, other = Scene(3, seed=31, device="cuda:0"), Scene(3, seed=32, device="cuda:0")
    for s, seed in ((scene, 31), (other, 32)):      # the small range: points and poses near the ego
        s.points = {k: p[(p[:, 0].abs() < 28) & (p[:, 1].abs() < 28)][:6000].contiguous() for k, p in s.points.items()}
        s.pairwise = synth.pairwise_t_matrix(synth.agent_poses(seed, 3, r_min=3.0, r_max=10.0), 5)[None]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = pipe.forward(other)
        eager = {k: eager[k].clone() for k in ("cls_preds", "reg_preds", "dir_preds")}
        eb, es = pipe.step(other)
        pipe.capture(scene, warmup=1)
        pipe.replay(other)
        gb, gs = pipe.replay(other)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in eager.values())
    assert (gb is None) == (eb is None)
    if eb is not None:
        assert gb.shape == eb.shape and torch.allclose(gb, eb, atol=1e-3) and torch.allclose(gs, es, atol=1e-4)


@pytest.mark.grad
def test_cobevt_gradient_path_on_device_matches_cpu(g):
    """Under autograd the module runs the reference's torch arithmetic on the device: same output as the golden, and the gradients
    of the input and of every parameter equal the CPU's."""
    from oracle import oracle_np as O
    aff = O.normalize_pairwise_tfm(g["l5n3_pairwise"], *g["HW_m"], 1)
    grads = {}
    for dev in ("cpu", "cuda"):
        from heal_amd.opencood.models.fuse_modules.fusion_in_one import CoBEVT
        model = fill_module(CoBEVT(dict(COBEVT_ARGS))).to(dev).eval()
        x = torch.from_numpy(_x(g, "l5n3_")).to(dev).requires_grad_(True)
        out = model(x, torch.tensor([3]), aff)
        assert rel_err(out.detach().cpu().numpy(), g["l5n3_out"]) <= 1e-4, dev
        out.square().mean().backward()
        grads[dev] = {"x": x.grad.cpu()}
        grads[dev].update({n: p.grad.cpu() for n, p in model.named_parameters()})
    for name, want in grads["cpu"].items():
        got = grads["cuda"][name]
        assert bool(torch.isfinite(got).all()), name
        assert rel_err(got.numpy(), want.numpy()) <= 1e-3, (name, rel_err(got.numpy(), want.numpy()))
