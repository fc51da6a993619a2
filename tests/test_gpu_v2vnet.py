"""V2VNet fusion on the MI355X: heal_v2v_message bit-exact against fp64 on integer fixtures, heal_gru_zero_state within a stated
ulp bound of torch's fp32 functions, the module and the end-to-end model against the reference's goldens
(tests/golden/v2vnet_small.npz), the full-size and camera-size HIP path against the module's own torch path in fp64, captured-graph
replay, and the gradient path on the device."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, ops
from tests.golden.detfill import fill_module
from tests.test_v2vnet_cpu import CASES, E2E_RANGE, case_inputs, e2e_data, make_v2vnet, rel_err, v2vnet_args

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]
DEV = "cuda:0"


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def message_fixture(n_ego, N, cin, cout, H, W, seed, zero_agent=None):
    """Small integers (|x| <= 3, |w| <= 2, |E| <= 8, |res| <= 8) and masks in {0, 1/4, 1/2, 3/4, 1}: every product and sum of the
    kernel is exact in fp32 (sum |w||x| + |E| + |res| < 2^22 for the shapes here), so results equal an fp64 evaluation rounded
    at the kernel's rounding points."""
    gen = torch.Generator().manual_seed(seed)
    xs = _ints(gen, (n_ego, N, cin, H, W), -3, 3)
    w = _ints(gen, (cout, cin, 3, 3), -2, 2)
    mask = _ints(gen, (n_ego, N, H, W), 0, 4) / 4.0
    if zero_agent is not None:
        mask[:, zero_agent] = 0.0
    e = _ints(gen, (n_ego, cout + 16, H, W), -8, 8)       # wider than cout: the kernel reads a channel slice
    res = _ints(gen, (n_ego, cout, H, W), -8, 8)
    assert 9 * cin * 2 * 3 * N + 8 + 8 < 2 ** 22
    return [t.to(DEV) for t in (xs, w, mask, e, res)]


def message_fp64(xs, w, mask, e, res, mode):
    n_ego, N, cin, H, W = xs.shape
    cout = w.shape[0]
    conv = F.conv2d(xs.double().reshape(n_ego * N, cin, H, W), w.double(), padding=1).reshape(n_ego, N, cout, H, W)
    m = mask.double()[:, :, None]
    E = e.double()[:, :cout]
    if mode == "mean":
        tot = (m * conv).sum(1)                 # exact: the order of the kernel's sum does not matter
        v = ((tot + m.sum(1) * E) / N).float()  # fp32 division of an exact value (the kernel's one rounding)
    else:
        v = (m * (conv + E[:, None])).max(1)[0].float()
    if res is not None:
        v = (res.double() + v.double()).float()
    return v


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("N", range(1, 9))
def test_v2v_message_exact(mode, N):
    for (H, W, cin, cout, n_ego, th, split, use_res, zero) in [
            (13, 11, 24, 80, 2, None, None, True, None),      # odd map, channel tails, default tile / split
            (16, 16, 16, 64, 1, "4", 1, False, 0),            # one ego, an all-zero mask agent
            (9, 20, 8, 72, 2, "16", None, True, N - 1),       # 16-row tiles, zero mask on the last agent
            (17, 18, 16, 64, 1, "8", N, False, None),         # the agent split at its maximum (N partials + reduce)
            (3, 5, 12, 20, 2, None, None, True, None),        # cin = 8 + 4: a partial second chunk; cout below one 64-row block
            (1, 1, 3, 65, 1, "4", None, False, None),         # cin below one chunk; cout one row into a second block; a 1 x 1 map
            (3, 5, 3, 65, 1, "16", N, True, None),            # the same channel edges through the split path
            (1, 1, 12, 20, 2, "8", None, True, 0)]:           # a 1 x 1 map with a partial chunk and an all-zero mask agent
        xs, w, mask, e, res = message_fixture(n_ego, N, cin, cout, H, W, seed=100 * N + H, zero_agent=zero)
        old = os.environ.get("HEAL_V2V_TH")
        if th:
            os.environ["HEAL_V2V_TH"] = th
        try:
            with torch.no_grad():
                got = ops.v2v_message(xs, mask, e, w, res if use_res else None, mode, nsplit=split)
        finally:
            if th:
                if old is None:
                    del os.environ["HEAL_V2V_TH"]
                else:
                    os.environ["HEAL_V2V_TH"] = old
        want = message_fp64(xs, w, mask, e, res if use_res else None, mode)
        assert torch.equal(got, want), (mode, N, H, W, th, split, float((got - want).abs().max()))


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("N,nsplit", [(5, 3), (7, 4)])
def test_v2v_message_uneven_split_exact(mode, N, nsplit):
    """Agent splits of unequal length (5 = 2 + 2 + 1, 7 = 2 + 2 + 2 + 1) on the integer fixture: bit for bit the fp64 evaluation,
    and the bits of the unsplit launch; an odd map, a partial channel chunk and a Cout tail."""
    for H, W, cin, cout, n_ego, use_res in [(13, 11, 12, 65, 2, True), (3, 5, 24, 20, 1, False)]:
        xs, w, mask, e, res = message_fixture(n_ego, N, cin, cout, H, W, seed=1000 * N + nsplit + H, zero_agent=N - 1)
        res = res if use_res else None
        with torch.no_grad():
            got = ops.v2v_message(xs, mask, e, w, res, mode, nsplit=nsplit)
            one = ops.v2v_message(xs, mask, e, w, res, mode, nsplit=1)
        want = message_fp64(xs, w, mask, e, res, mode)
        assert torch.equal(got, want), (mode, N, nsplit, H, W, float((got - want).abs().max()))
        assert torch.equal(one, want), (mode, N, H, W)


def test_v2v_message_split_equals_unsplit():
    xs, w, mask, e, _ = message_fixture(1, 5, 16, 64, 20, 20, seed=7)
    xs = xs + 0.1 * torch.randn_like(xs)                # not exact any more: the split must still be deterministic and close
    with torch.no_grad():
        a = ops.v2v_message(xs, mask, e, w, None, "mean", nsplit=1)
        b = ops.v2v_message(xs, mask, e, w, None, "mean", nsplit=3)
        c = ops.v2v_message(xs, mask, e, w, None, "mean", nsplit=3)
    assert torch.equal(b, c)
    assert rel_err(b.cpu(), a.cpu()) < 1e-6


def test_v2v_message_rejects_bad_inputs():
    xs, w, mask, e, res = message_fixture(1, 3, 8, 64, 8, 8, seed=3)
    with pytest.raises(_capi.HealAmdError):
        ops.v2v_message(xs, mask, e, w, None, "sum")
    with pytest.raises(_capi.HealAmdError):
        ops.v2v_message(xs, mask[:, :2], e, w)
    with pytest.raises(_capi.HealAmdError):
        ops.v2v_message(xs, mask, e[:, :32], w)           # E narrower than cout
    with pytest.raises(_capi.HealAmdError):
        ops.v2v_message(xs.repeat(1, 3, 1, 1, 1), mask.repeat(1, 3, 1, 1), e, w)   # 9 agents
    with pytest.raises(_capi.HealAmdError):
        ops.v2v_message(xs, mask, e, w[:, :, :1, :1])


def test_gru_zero_state_within_4_ulp():
    """h = sigmoid(u) * tanh(c) against torch's fp32 sigmoid and tanh: |h - h_torch| <= 4 ulp(h_torch) (expf / tanhf are within
    2 ulp, the division and product add one rounding each), with an add operand that is a channel slice of a wider tensor."""
    gen = torch.Generator().manual_seed(5)
    gates = (torch.randn((3, 64, 9, 7), generator=gen) * 4).to(DEV)
    wide = (torch.randn((3, 96, 9, 7), generator=gen) * 4).to(DEV)
    add = wide[:, 32:]
    with torch.no_grad():
        h = ops.gru_zero_state(gates, add)
        h0 = ops.gru_zero_state(gates)
    for got, u, c in ((h, gates[:, :32] + add[:, :32], gates[:, 32:] + add[:, 32:]), (h0, gates[:, :32], gates[:, 32:])):
        want = (torch.sigmoid(u) * torch.tanh(c)).cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32))
        err = np.abs(got.cpu().numpy() - want) / ulp
        assert float(err.max()) <= 4, float(err.max())


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "v2vnet_small.npz"))


@pytest.mark.parametrize("prefix", sorted(CASES))
def test_v2vnet_module_on_device_matches_reference(g, prefix):
    model = make_v2vnet(prefix).to(DEV)
    x, rl, aff = case_inputs(g, prefix)
    with torch.no_grad():
        assert model.fused_ok(x.to(DEV), [int(v) for v in rl])
        got = model(x.to(DEV), rl, aff).cpu().numpy()
    assert rel_err(got, g[f"{prefix}out"]) <= 1e-3, rel_err(got, g[f"{prefix}out"])


def test_v2vnet_model_on_device_matches_reference(g):
    from heal_amd import configs
    from heal_amd.opencood.tools.train_utils import create_model
    model = fill_module(create_model(configs.lidar_baseline("v2vnet", E2E_RANGE))).to(DEV).eval()
    data = e2e_data(g)
    data["inputs_m1"] = {k: v.to(DEV) for k, v in data["inputs_m1"].items()}
    data["pairwise_t_matrix"] = data["pairwise_t_matrix"].to(DEV)
    with torch.no_grad():
        out = model(data)
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].cpu().numpy(), g[f"e2e_{name}"])
        assert e <= 1e-3, (key, e)


def _vs_fp64(n, H, W, seed, bound):
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import V2VNetFusion
    from heal_amd import synth
    from oracle import oracle_np as O
    model = fill_module(V2VNetFusion(v2vnet_args({}, (H, W), 256))).to(DEV).eval()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 256, H, W), generator=gen).to(DEV)
    pw = synth.pairwise_t_matrix(synth.agent_poses(seed, n, r_min=4.0, r_max=30.0), 5)[None]
    aff = O.normalize_pairwise_tfm(pw, H * 0.4 * 4, W * 0.4 * 4, 1)
    with torch.no_grad():
        got = model(x, torch.tensor([n]), aff)
        ref = model.double().forward_torch(x.double(), torch.tensor([n]), aff)
    e = rel_err(got.cpu().numpy(), ref.cpu().numpy())
    print(f"V2VNet {n} agents {H}x{W}x256: HIP path vs fp64 torch, max relative error {e:.2e} (bound {bound})")
    assert e <= bound, e


def test_v2vnet_full_size_vs_fp64():
    """5 agents at 128 x 128 x 256 (lidar_v2vnet.yaml): the HIP path against the reference arithmetic in fp64 on the device.
    Bound 1e-4 relative to the output's maximum (fp32 accumulation over K = 2304 x 5 agents, two rounds)."""
    _vs_fp64(5, 128, 128, 11, 1e-4)


def test_v2vnet_camera_size_vs_fp64():
    """camera_v2vnet.yaml: 64 x 64 maps, 3 agents."""
    _vs_fp64(3, 64, 64, 12, 1e-4)


def test_v2vnet_module_graph_replay_after_weight_change(g):
    """Capture the module, change msg_cnn's weight in place, run it eagerly (which rebuilds the weight slices): the replay still
    returns the captured output bit for bit and every address it logged is live; the eager run sees the change."""
    model = make_v2vnet("n3_").to(DEV)
    x, rl, aff = case_inputs(g, "n3_")
    x = x.to(DEV)
    st = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(st):
        eager = model(x, rl, aff).clone()
        _capi.guard_take()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            y = model(x, rl, aff)
        log = _capi.guard_take()
        graph.replay()
        st.synchronize()
        assert torch.equal(y, eager)
        want = y.clone()
        model.msg_cnn.weight.mul_(0.5)
        changed = model(x, rl, aff)
        _capi.guard_check(log, "V2VNet replay after a weight change")
        graph.replay()
        st.synchronize()
    assert not torch.equal(changed, want)
    assert torch.equal(y, want)


def test_v2vnet_pipeline_graph_replay_equals_eager():
    from heal_amd import configs, synth
    from heal_amd.pipeline import Scene, ScenePipeline
    pipe = ScenePipeline(configs.lidar_baseline("v2vnet", SMALL_RANGE), DEV, seed=3)
    scene, other = Scene(3, seed=31, device=DEV), Scene(3, seed=32, device=DEV)
    for s, seed in ((scene, 31), (other, 32)):
        s.points = {k: p[(p[:, 0].abs() < 28) & (p[:, 1].abs() < 28)][:6000].contiguous() for k, p in s.points.items()}
        s.pairwise = synth.pairwise_t_matrix(synth.agent_poses(seed, 3, r_min=3.0, r_max=10.0), 5)[None]
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
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
def test_v2vnet_gradient_path_on_device_matches_cpu(g):
    """Under autograd the module runs the reference's torch arithmetic on the device: the golden output, and the gradients of the
    input and of every parameter equal the CPU's within 1e-4."""
    grads = {}
    for dev in ("cpu", DEV):
        model = make_v2vnet("n3_").to(dev)
        x, rl, aff = case_inputs(g, "n3_")
        x = x.to(dev).requires_grad_(True)
        out = model(x, rl, aff)
        assert rel_err(out.detach().cpu().numpy(), g["n3_out"]) <= 1e-4, dev
        out.square().mean().backward()
        grads[dev] = {"x": x.grad.cpu()}
        grads[dev].update({n: p.grad.cpu() for n, p in model.named_parameters()})
    for k, v in grads["cpu"].items():
        assert rel_err(grads[DEV][k].numpy(), v.numpy()) <= 1e-4, k
