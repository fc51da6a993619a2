"""DiscoNet fusion on the MI355X: heal_disco_fuse's logits bit-exact against fp64 on integer fixtures, its output within a derived
bound of an fp64 softmax-and-sum, the module and the end-to-end model against the goldens (tests/golden/disconet_small.npz), the
realistic sizes against the module's own torch path in fp64, operand checks, captured-graph replay, and the gradient path."""
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests.backward_refs import shift_rows          # noqa: F401  (tests/test_gpu_where2comm.py imports it from here)
from tests.coalign_refs import device_rows_case
from tests.golden.disco_fill import fill_disco
from tests.test_disconet_cpu import CASES, E2E_RANGE, TOL, case_inputs, e2e_data, e2e_hypes, make_disco, rel_err

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]
DEV = "cuda:0"
M1, M2, M3 = ops.DISCO_WIDTHS
W4_SCALE = 2.0 ** -6          # conv1_4's weights are +-2^-6: a power of two keeps every product exact and the logits moderate


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def disco_fixture(n, C, H, W, seed, equal=False):
    """Integer operands: |x| <= 1, |W1n| <= 1, |E0| <= 8, |W2|, |W3| <= 1, |b2|, |b3| <= 8, w4 = +-2^-6 (alternating), b4 = 2^-6 * small int.
    The warped maps are multiples of 1/4.  Bounds on every intermediate (and so on every partial sum, in any order):
      |h1| <= C + 8,  |h2| <= 128 |h1| + 8,  |h3| <= 32 |h2| + 8,  |logit| / 2^-6 <= 8 |h3| + 8,
    all multiples of 1/4: exact in fp32 while 4 x the last bound is below 2^24 (asserted)."""
    gen = torch.Generator().manual_seed(seed)
    feats = _ints(gen, (n, C, H, W), -1, 1)
    if equal:
        feats = feats[:1].repeat(n, 1, 1, 1)
    w1n = _ints(gen, (M1, C), -1, 1)
    e0 = _ints(gen, (M1, H, W), -8, 8)
    w2, b2 = _ints(gen, (M2, M1), -1, 1), _ints(gen, (M2,), -8, 8)
    w3, b3 = _ints(gen, (M3, M2), -1, 1), _ints(gen, (M3,), -8, 8)
    w4 = torch.tensor([1.0, -1.0] * (M3 // 2)) * W4_SCALE      # alternating signs: about half of the logits are clamped
    b4 = _ints(gen, (1,), -4, 4) * W4_SCALE
    b1 = C + 8
    b2_ = M1 * b1 + 8
    b3_ = M2 * b2_ + 8
    assert 4 * (M3 * b3_ + 8) < 2 ** 24
    return [t.to(DEV) for t in (feats, e0, w1n, w2, b2, w3, b3, w4, b4)]


def warp_fp64(feats, rows):
    """The reference's warp (affine_grid + grid_sample) in fp64 on the CPU; for the translations used here the exact values are
    multiples of 1/4, so the fp64 result is rounded to that grid."""
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import _warp_affine_simple
    nbr = _warp_affine_simple(feats.double().cpu(), torch.from_numpy(rows), feats.shape[2:])
    return torch.round(nbr * 4) / 4


def logits_fp64(nbr, e0, w1n, w2, b2, w3, b3, w4, b4):
    d = lambda t: t.double().cpu()     # noqa: E731
    h1 = torch.relu(torch.einsum("mc,nchw->nmhw", d(w1n), nbr) + d(e0)[None])
    h2 = torch.relu(torch.einsum("om,nmhw->nohw", d(w2), h1) + d(b2)[None, :, None, None])
    h3 = torch.relu(torch.einsum("om,nmhw->nohw", d(w3), h2) + d(b3)[None, :, None, None])
    return torch.relu(torch.einsum("m,nmhw->nhw", d(w4), h3) + d(b4))


def run_kernel(ops_in, rows):
    feats, e0, w1n, w2, b2, w3, b3, w4, b4 = ops_in
    with torch.no_grad():
        return ops.disco_fuse(feats, rows, True, e0, ops.mfma_a_fragments(w1n), w2, b2, w3, b3, w4, b4, return_scores=True)


def out_bound(n):
    """|out - sum_a softmax(l)_a x_a| per element, for |x_a| <= 1 and logits that the kernel holds exactly:
    e_a = expf(l_a - max) carries at most 2 ulp = 4 eps relative error (eps = 2^-24; l_a - max is exact for these logits); the
    sequential sum den adds (n - 1) eps; the division 1 eps: p_a is within (n + 8) eps.  The product p_a x_a adds 1 eps and the
    sequential sum over agents (n - 1) eps: (2 n + 8) eps sum_a p_a |x_a| <= (2 n + 8) eps.  One more eps covers the second-order
    terms."""
    return (2 * n + 9) * 2.0 ** -24


# (H, W, C, shifts): power-of-two maps (exact sampling coordinates exist for no other size) that are not multiples of the 16 x 4
# tile, a channel count that is not a multiple of the 32-channel chunk nor of a 16-row A tile, half- and whole-pixel shifts
def _shapes(n):
    far = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (1.0, 2.0), (-0.5, 0.5), (-3.0, 1.0), (2.5, -1.5), (0.5, 0.5)]
    return [(8, 8, 36, far[:n]),
            (2, 32, 64, [(0.0, 0.0)] + [(s, 0.0) for s in (0.5, -1.0, 1.5, -2.0, 2.5, -3.0, 3.5)][:n - 1]),
            (16, 4, 32, far[:n][::-1]),
            (8, 32, 20, far[:n])]


@pytest.mark.parametrize("n", [1, 3, 5, 8])
def test_disco_fuse_logits_exact_and_output_within_bound(n):
    for H, W, C, shifts in _shapes(n):
        fx = disco_fixture(n, C, H, W, seed=10 * n + H)
        rows = shift_rows(shifts, H, W)
        out, scores = run_kernel(fx, rows)
        nbr = warp_fp64(fx[0], rows)
        want = logits_fp64(nbr, *fx[1:])
        assert torch.equal(scores.cpu(), want.float()), (n, H, W, C, float((scores.cpu().double() - want).abs().max()))
        if n > 1:
            assert float((want > 0).float().mean()) > 0.05 and float((want == 0).float().mean()) > 0.05     # both ReLU branches
        ref = (torch.softmax(want, dim=0)[:, None] * nbr).sum(0)
        err = float((out.cpu().double() - ref).abs().max())
        print(f"disco_fuse n={n} {H}x{W}x{C}: logits exact, output error {err:.3e} (bound {out_bound(n):.3e})")
        assert err <= out_bound(n), (n, H, W, C, err)
        with torch.no_grad():       # without the testing hook the output is the same, bit for bit
            assert torch.equal(ops.disco_fuse(fx[0], rows, True, fx[1], ops.mfma_a_fragments(fx[2]), *fx[3:]), out)


def test_disco_fuse_logits_exact_on_a_grid_of_more_than_one_block_per_cu():
    """128 x 256 pixels are 512 blocks: two resident blocks per CU, and a second round of blocks on some."""
    n, C, H, W = 3, 32, 128, 256
    fx = disco_fixture(n, C, H, W, seed=77)
    rows = shift_rows([(0.0, 0.0), (2.5, -1.0), (-7.0, 3.5)], H, W)
    out, scores = run_kernel(fx, rows)
    nbr = warp_fp64(fx[0], rows)
    want = logits_fp64(nbr, *fx[1:])
    assert torch.equal(scores.cpu(), want.float())
    ref = (torch.softmax(want, dim=0)[:, None] * nbr).sum(0)
    assert float((out.cpu().double() - ref).abs().max()) <= out_bound(n)


def test_disco_fuse_single_agent_skips_the_layer():
    """One agent: the output is the warped map exactly, with or without the PixelWeightLayer operands."""
    fx = disco_fixture(1, 36, 8, 8, seed=5)
    rows = shift_rows([(0.5, -1.0)], 8, 8)
    with torch.no_grad():
        bare = ops.disco_fuse(fx[0], rows, True, None, None, None, None, None, None, None, None)
    out, _ = run_kernel(fx, rows)
    assert torch.equal(bare, out) and torch.equal(bare.cpu(), warp_fp64(fx[0], rows)[0].float())


@pytest.mark.parametrize("n", [3, 5, 8])
def test_disco_fuse_agent_out_of_the_map_takes_part_in_the_softmax(n):
    H, W, C = 8, 16, 32
    fx = disco_fixture(n, C, H, W, seed=70 + n)
    shifts = [(0.0, 0.0), (W + 2.0, 0.0)] + [(0.5 * k, 0.0) for k in range(1, n - 1)]     # agent 1 is translated out of the map
    rows = shift_rows(shifts, H, W)
    out, scores = run_kernel(fx, rows)
    nbr = warp_fp64(fx[0], rows)
    assert float(nbr[1].abs().max()) == 0.0
    want = logits_fp64(nbr, *fx[1:])
    assert torch.equal(scores.cpu(), want.float())
    ref = (torch.softmax(want, dim=0)[:, None] * nbr).sum(0)
    assert float((out.cpu().double() - ref).abs().max()) <= out_bound(n)
    # the absent agent keeps its share: dropping it from the softmax gives a different result
    keep = [a for a in range(n) if a != 1]
    dropped = (torch.softmax(want[keep], dim=0)[:, None] * nbr[keep]).sum(0)
    assert float((dropped - ref).abs().max()) > 1e-3


@pytest.mark.parametrize("n", [3, 5, 8])
def test_disco_fuse_equal_logits_give_weights_of_one_nth(n):
    """n copies of one map under the same affine: n equal logits, expf(0) = 1, den = n, every weight the fp32 quotient 1 / n; the
    output equals the fp32 evaluation ((p x + p x) + ...) bit for bit."""
    H, W, C = 8, 8, 32
    fx = disco_fixture(n, C, H, W, seed=90 + n, equal=True)
    rows = shift_rows([(0.5, 0.0)] * n, H, W)
    out, scores = run_kernel(fx, rows)
    assert all(torch.equal(scores[a], scores[0]) for a in range(n))
    x = warp_fp64(fx[0], rows)[0].float()
    p = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    acc = torch.zeros_like(x)
    for _ in range(n):
        acc = acc + p * x
    assert torch.equal(out.cpu(), acc)


def test_disco_fuse_odd_map_against_fp64():
    """A 13 x 11 map: its sampling coordinates are not exact in fp32 (only power-of-two sizes are), so the logits are compared
    with the fp64 evaluation of the reference's arithmetic within 1e-5 of their maximum instead of bit for bit."""
    n, C, H, W = 3, 36, 13, 11
    fx = disco_fixture(n, C, H, W, seed=13)
    rows = shift_rows([(0.0, 0.0), (0.5, 1.0), (-1.5, 0.5)], H, W)
    out, scores = run_kernel(fx, rows)
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import _warp_affine_simple
    nbr = _warp_affine_simple(fx[0].double().cpu(), torch.from_numpy(rows), (H, W))
    want = logits_fp64(nbr, *fx[1:])
    assert rel_err(scores.cpu().double().numpy(), want.numpy()) <= 1e-5
    ref = (torch.softmax(want, dim=0)[:, None] * nbr).sum(0)
    assert rel_err(out.cpu().double().numpy(), ref.numpy()) <= 1e-5


@pytest.mark.parametrize("grid_f64", [True, False])
def test_disco_fuse_device_rows_equal_host_rows(grid_f64):
    """The rows as a float64 CUDA tensor (read by the kernel at run time) give the bits of the rows passed by value."""
    n, H, W, rows = device_rows_case()
    fx = disco_fixture(n, 8, H, W, seed=21)
    frag = ops.mfma_a_fragments(fx[2])
    with torch.no_grad():
        host = ops.disco_fuse(fx[0], rows, grid_f64, fx[1], frag, *fx[3:], return_scores=True)
        devr = ops.disco_fuse(fx[0], torch.from_numpy(rows).to(DEV), grid_f64, fx[1], frag, *fx[3:], return_scores=True)
    assert float(host[0].abs().max()) > 0 and float(host[1].abs().max()) > 0
    assert torch.equal(devr[0], host[0]) and torch.equal(devr[1], host[1])


def test_disco_fuse_rejects_bad_inputs():
    feats, e0, w1n, w2, b2, w3, b3, w4, b4 = disco_fixture(3, 32, 8, 8, seed=3)
    frag = ops.mfma_a_fragments(w1n)
    rows = shift_rows([(0.0, 0.0)] * 3, 8, 8)
    with pytest.raises(_capi.HealAmdError, match="agents"):
        ops.disco_fuse(feats.repeat(3, 1, 1, 1), shift_rows([(0.0, 0.0)] * 9, 8, 8), True, e0, frag, w2, b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="e0"):
        ops.disco_fuse(feats, rows, True, e0[:, :4], frag, w2, b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="dtype"):
        ops.disco_fuse(feats, rows, True, e0, frag, w2.double(), b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="dtype"):
        ops.disco_fuse(feats.half(), rows, True, e0, frag, w2, b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="w1n_frag"):
        ops.disco_fuse(feats, rows, True, e0, frag[:, :4], w2, b2, w3, b3, w4, b4)       # fragments of another channel count
    with pytest.raises(_capi.HealAmdError, match="w2"):
        ops.disco_fuse(feats, rows, True, e0, frag, w2[:, :64], b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="b3"):
        ops.disco_fuse(feats, rows, True, e0, frag, w2, b2, w3, b3[:4], w4, b4)
    with pytest.raises(_capi.HealAmdError, match="multiple of"):
        ops.disco_fuse(feats[:, :30], rows, True, e0, frag, w2, b2, w3, b3, w4, b4)
    with pytest.raises(_capi.HealAmdError, match="affine"):
        ops.disco_fuse(feats, rows[:2], True, e0, frag, w2, b2, w3, b3, w4, b4)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disconet_small.npz"))


@pytest.mark.parametrize("prefix", sorted(CASES))
def test_disconet_module_on_device_matches_reference(g, prefix):
    model = make_disco(prefix).to(DEV)
    x, rl, aff = case_inputs(g, prefix)
    with torch.no_grad():
        assert model.fused_ok(x.to(DEV), [int(v) for v in rl])
        got = model(x.to(DEV), rl, aff).cpu().numpy()
    assert rel_err(got, g[f"{prefix}out"]) <= TOL, rel_err(got, g[f"{prefix}out"])


def test_disconet_model_on_device_matches_reference(g):
    from heal_amd.opencood.tools.train_utils import create_model
    model = fill_disco(create_model(e2e_hypes())).to(DEV).eval()
    data = e2e_data(g)
    data["inputs_m1"] = {k: v.to(DEV) for k, v in data["inputs_m1"].items()}
    data["pairwise_t_matrix"] = data["pairwise_t_matrix"].to(DEV)
    calls = {}
    ops.TIMING = calls
    try:
        with torch.no_grad():
            out = model(data)
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert "disco_fuse_c256" in calls          # the kernel ran: no quiet torch path
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].cpu().numpy(), g[f"e2e_{name}"])
        assert e <= TOL, (key, e)


def test_disconet_more_than_eight_agents_falls_back_to_torch():
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import DiscoFusion
    model = fill_disco(DiscoFusion(32)).to(DEV).eval()
    x = torch.randn((9, 32, 8, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    aff = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (1, 9, 9, 1, 1))
    with torch.no_grad():
        assert not model.fused_ok(x, [9]) and model.fused_ok(x[:8], [8])
        got = model(x, torch.tensor([9]), aff)
        want = model.forward_torch(x, torch.tensor([9]), aff)
    assert torch.equal(got, want)


def _vs_fp64(n, H, W, seed):
    from heal_amd import synth
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import DiscoFusion
    from oracle import oracle_np as O
    model = fill_disco(DiscoFusion(256)).to(DEV).eval()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 256, H, W), generator=gen).to(DEV)
    pw = synth.pairwise_t_matrix(synth.agent_poses(seed, n, r_min=4.0, r_max=30.0), 5)[None]
    aff = O.normalize_pairwise_tfm(pw, H * 0.4 * 2, W * 0.4 * 2, 1)
    rl = torch.tensor([n])
    old = os.environ.get("HEAL_DISCO_FUSED")
    with torch.no_grad():
        assert model.fused_ok(x, [n])
        got = model(x, rl, aff)
        os.environ["HEAL_DISCO_FUSED"] = "0"
        try:
            assert not model.fused_ok(x, [n])
            ref32 = model(x, rl, aff)              # the reference's own fp32 arithmetic on the device
        finally:
            if old is None:
                del os.environ["HEAL_DISCO_FUSED"]
            else:
                os.environ["HEAL_DISCO_FUSED"] = old
        ref = model.double().forward_torch(x.double(), rl, aff)
    scale = float(ref.abs().max())
    err_hip = float((got.double() - ref).abs().max()) / scale
    err_ref32 = float((ref32.double() - ref).abs().max()) / scale
    print(f"DiscoNet {n} agents {H}x{W}x256 vs fp64 torch: HIP path {err_hip:.3e}, torch fp32 path {err_ref32:.3e} "
          f"(ratio {err_hip / err_ref32:.2f}, allowed 4)")
    assert err_hip <= 4 * err_ref32, (err_hip, err_ref32)


def test_disconet_lidar_baseline_size_vs_fp64():
    """5 agents at 128 x 128 x 256 (configs.lidar_baseline): the HIP path against the reference arithmetic in fp64 on the device,
    as error relative to the output's maximum, no more than 4 x the error of the reference's own fp32 arithmetic (the factor
    allows for the different summation order of the MFMA chains and the split of layer 1)."""
    _vs_fp64(5, 128, 128, 11)


def test_disconet_yaml_size_vs_fp64():
    """5 agents at 256 x 256 x 256 (the disco YAMLs: stride-1 shrinker)."""
    _vs_fp64(5, 256, 256, 12)


def test_disconet_camera_size_vs_fp64():
    """3 agents at 64 x 64 x 256."""
    _vs_fp64(3, 64, 64, 13)


def test_disconet_module_graph_replay_after_weight_change(g):
    """Capture the module, change conv1_1's weight and a BatchNorm running statistic in place, run it eagerly (which rebuilds the
    folded weights): the replay still returns the captured output bit for bit and every address it logged is live; the eager run
    sees the change."""
    model = make_disco("n3_").to(DEV)
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
        model.pixel_weight_layer.conv1_1.weight.mul_(0.5)
        changed_w = model(x, rl, aff).clone()
        model.pixel_weight_layer.bn1_2.running_var.mul_(4.0)
        changed_bn = model(x, rl, aff).clone()
        _capi.guard_check(log, "DiscoNet replay after a weight change")
        graph.replay()
        st.synchronize()
        ref = model.forward_torch(x, rl, aff)
    assert not torch.equal(changed_w, want) and not torch.equal(changed_bn, changed_w)
    assert rel_err(changed_bn.cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert torch.equal(y, want)


def test_disconet_pipeline_graph_replay_equals_eager():
    from heal_amd import configs, synth
    from heal_amd.pipeline import Scene, ScenePipeline
    pipe = ScenePipeline(configs.lidar_baseline("disconet", SMALL_RANGE), DEV, seed=3)
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
def test_disconet_gradient_path_on_device_matches_cpu(g):
    """Under autograd the module runs the reference's torch arithmetic on the device: the golden output, and the gradients of the
    input and of every parameter equal the CPU's within 1e-4."""
    grads = {}
    for dev in ("cpu", DEV):
        model = make_disco("n3_").to(dev)
        x, rl, aff = case_inputs(g, "n3_")
        x = x.to(dev).requires_grad_(True)
        assert not model.fused_ok(x, [3])
        out = model(x, rl, aff)
        assert rel_err(out.detach().cpu().numpy(), g["n3_out"]) <= TOL, dev
        out.square().mean().backward()
        grads[dev] = {"x": x.grad.cpu()}
        grads[dev].update({n: p.grad.cpu() for n, p in model.named_parameters()})
    for k, v in grads["cpu"].items():
        assert rel_err(grads[DEV][k].numpy(), v.numpy()) <= 1e-4, k
