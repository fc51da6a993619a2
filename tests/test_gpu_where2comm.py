"""Where2comm and Who2com fusion on the MI355X: heal_warp_mha_fuse's logits bit-exact against fp64 on integer fixtures, its context
within a derived bound of an fp64 softmax-and-sum, the warped ego map exact; the modules and the end-to-end models against the
goldens (tests/golden/where2comm_small.npz, who2com_small.npz), the realistic sizes against the module's own torch path in fp64,
operand checks, captured-graph replay, and the gradient path."""
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests.coalign_refs import device_rows_case
from tests.golden.w2c_fill import fill_w2c
from tests.test_gpu_disconet import shift_rows
from tests.test_where2comm_cpu import (CASES, TOL, WHO_CASES, case_inputs, e2e_data, e2e_hypes, make_w2c, make_who, rel_err)

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]
DEV = "cuda:0"
X_MAX, KV_MAX, B_MAX = 1, 2, 1        # |q_map|, |x_ego| <= 1; |kv_map| <= 2; |bq|, |bk|, |bv| <= 1 (integers)
V_BOUND = float(KV_MAX + B_MAX)       # |v_j| = |S_j(v_map) + bv|: a bilinear sample is a convex combination (or less, at the border)


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def mha_fixture(n, C, heads, H, W, seed, equal=False):
    """Integer operands.  The sampled maps are multiples of 1/4 (half-pixel translations on power-of-two maps), the biases integers
    and scale = 1 / sqrt(d) a power of two (asserted), so q * scale is a multiple of scale / 4, k a multiple of 1/4 and every
    product and partial sum of a logit a multiple of scale / 16 bounded by d * scale * (X_MAX + B_MAX) * (KV_MAX + B_MAX): exact
    in fp32, in any order, while 16 x that bound / scale is below 2^24 (asserted)."""
    d = C // heads
    scale = d ** -0.5
    assert np.log2(scale) == round(np.log2(scale))
    assert 16 * d * (X_MAX + B_MAX) * (KV_MAX + B_MAX) < 2 ** 24
    gen = torch.Generator().manual_seed(seed)
    q_map = _ints(gen, (C, H, W), -X_MAX, X_MAX)
    kv_map = _ints(gen, (n, 2 * C, H, W), -KV_MAX, KV_MAX)
    x_ego = _ints(gen, (C, H, W), -X_MAX, X_MAX)
    if equal:
        kv_map = kv_map[:1].repeat(n, 1, 1, 1)
    bq, bk, bv = (_ints(gen, (C,), -B_MAX, B_MAX) for _ in range(3))
    return [t.to(DEV) for t in (q_map, kv_map, x_ego, bq, bk, bv)]


def warp_fp64(maps, rows, exact=True):
    """The reference's warp (affine_grid + grid_sample) in fp64 on the CPU; for the translations of the integer fixtures the exact
    values are multiples of 1/4, so the fp64 result is rounded to that grid."""
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import _warp_affine_simple
    out = _warp_affine_simple(maps.double().cpu(), torch.from_numpy(np.asarray(rows)), maps.shape[2:])
    return torch.round(out * 4) / 4 if exact else out


def restate(fx, rows, heads, dtype=torch.float64, device="cpu", exact=True):
    """The issue's restatement: sample the projected maps, add the biases, scale q, per-head softmax over ALL agents, weighted
    sum -> (logits [n, heads, H, W], probabilities, v [n, C, H, W], ctx [C, H, W], ego_warped [C, H, W])."""
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import _warp_affine_simple
    q_map, kv_map, x_ego, bq, bk, bv = (t.to(device=device, dtype=dtype) for t in fx)
    n, C2, H, W = kv_map.shape
    C, d = C2 // 2, C2 // 2 // heads
    M = torch.from_numpy(np.asarray(rows)).to(device)

    def S(t, m):
        y = _warp_affine_simple(t, m, (H, W))
        return torch.round(y * 4) / 4 if exact else y
    q = S(q_map[None], M[:1])[0] + bq[:, None, None]
    kv = S(kv_map, M)
    k, v = kv[:, :C] + bk[None, :, None, None], kv[:, C:] + bv[None, :, None, None]
    logits = ((q * d ** -0.5).view(1, heads, d, H, W) * k.view(n, heads, d, H, W)).sum(2)
    p = torch.softmax(logits, dim=0)
    ctx = (p[:, :, None] * v.view(n, heads, d, H, W)).sum(0).reshape(C, H, W)
    return logits, p, v, ctx, S(x_ego[None], M[:1])[0]


def ctx_bound(n):
    """|ctx - sum_a softmax(l)_a v_a| per element, for |v_a| <= V_BOUND (held exactly: a multiple of 1/4 plus an integer) and
    logits that the kernel holds exactly.  As out_bound of tests/test_gpu_disconet.py: e_a = expf(l_a - max) carries at most 2 ulp
    = 4 eps relative error (eps = 2^-24; l_a - max is exact for these logits); the sequential sum den adds (n - 1) eps; the
    division 1 eps: p_a is within (n + 8) eps.  The product p_a v_a adds 1 eps and the sequential sum over agents (n - 1) eps:
    (2 n + 8) eps sum_a p_a |v_a| <= (2 n + 8) eps V_BOUND.  One more eps covers the second-order terms."""
    return (2 * n + 9) * 2.0 ** -24 * V_BOUND


def run_kernel(fx, rows, heads, logits=True):
    with torch.no_grad():
        return ops.warp_mha_fuse(*fx, heads, rows, True, return_logits=logits)


def check_exact(fx, rows, heads, n):
    ctx, ego, logits = run_kernel(fx, rows, heads)
    want_l, _, _, want_ctx, want_ego = restate(fx, rows, heads)
    assert torch.equal(logits.cpu(), want_l.float()), float((logits.cpu().double() - want_l).abs().max())
    assert torch.equal(ego.cpu(), want_ego.float())
    err = float((ctx.cpu().double() - want_ctx).abs().max())
    assert err <= ctx_bound(n), (err, ctx_bound(n))
    ctx2, ego2 = run_kernel(fx, rows, heads, logits=False)       # without the testing hook: the same, bit for bit
    assert torch.equal(ctx2, ctx) and torch.equal(ego2, ego)
    return err, want_l


# (H, W, C, heads): power-of-two maps (exact sampling coordinates exist for no other size) that are not multiples of the 16 x 4
# tile; head dims 4, 16, 16, 16 and 4; one case with a single head
SHAPES = [(8, 8, 32, 8), (2, 32, 128, 8), (16, 4, 64, 4), (8, 32, 16, 1), (8, 8, 16, 4)]
FAR = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (1.0, 2.0), (-0.5, 0.5), (-3.0, 1.0), (2.5, -1.5), (0.5, 0.5)]


@pytest.mark.parametrize("n", [1, 3, 5, 8])
def test_warp_mha_fuse_logits_exact_and_context_within_bound(n):
    for i, (H, W, C, heads) in enumerate(SHAPES):
        fx = mha_fixture(n, C, heads, H, W, seed=10 * n + i)
        shifts = FAR[:n] if i % 2 == 0 else [(0.5, -1.0)] + FAR[1:n][::-1]       # the ego's own row is a shift too in every other case
        err, want_l = check_exact(fx, shift_rows(shifts, H, W), heads, n)
        if n > 1:
            assert float(want_l.std()) > 0.1            # the logits differ: the softmax is not uniform
        print(f"warp_mha_fuse n={n} {H}x{W}x{C} heads={heads}: logits exact, context error {err:.3e} (bound {ctx_bound(n):.3e})")


def test_warp_mha_fuse_exact_on_a_grid_of_more_than_one_block_per_cu():
    """128 x 256 pixels x 8 heads are 4096 one-wave blocks: several resident per CU, and further rounds."""
    n, C, heads, H, W = 3, 32, 8, 128, 256
    fx = mha_fixture(n, C, heads, H, W, seed=77)
    check_exact(fx, shift_rows([(0.0, 0.0), (2.5, -1.0), (-7.0, 3.5)], H, W), heads, n)


@pytest.mark.parametrize("n", [3, 5, 8])
def test_warp_mha_fuse_agent_out_of_the_map_keeps_its_share(n):
    H, W, C, heads = 8, 16, 32, 8
    fx = mha_fixture(n, C, heads, H, W, seed=70 + n)
    shifts = [(0.0, 0.0), (W + 2.0, 0.0)] + [(0.5 * k, 0.0) for k in range(1, n - 1)]     # agent 1 is translated out of the map
    rows = shift_rows(shifts, H, W)
    _, want_l = check_exact(fx, rows, heads, n)
    ctx, _, logits = run_kernel(fx, rows, heads)
    assert float(warp_fp64(fx[1], rows)[1].abs().max()) == 0.0
    # its key is the bias alone: logit = scale * (q . bk) per head, exactly
    d = C // heads
    q = warp_fp64(fx[0][None], rows[:1])[0] + fx[3].double().cpu()[:, None, None]
    bias_logit = ((q * d ** -0.5).view(heads, d, H, W) * fx[4].double().cpu().view(heads, d, 1, 1)).sum(1)
    assert torch.equal(logits[1].cpu(), bias_logit.float())
    # ... and it keeps its share: dropping it from the softmax gives a different result
    _, p, v, want_ctx, _ = restate(fx, rows, heads)
    keep = [a for a in range(n) if a != 1]
    dropped = (torch.softmax(want_l[keep], dim=0)[:, :, None] * v[keep].view(n - 1, heads, d, H, W)).sum(0).reshape(C, H, W)
    assert float((dropped - want_ctx).abs().max()) > 1e-3


@pytest.mark.parametrize("n", [3, 5, 8])
def test_warp_mha_fuse_equal_agents_give_probabilities_of_one_nth(n):
    """n copies of one projected map under the identity: n equal logits per head, every probability 1 / n, and the context is v_0
    within the bound."""
    H, W, C, heads = 8, 8, 32, 8
    fx = mha_fixture(n, C, heads, H, W, seed=90 + n, equal=True)
    rows = shift_rows([(0.0, 0.0)] * n, H, W)
    ctx, _, logits = run_kernel(fx, rows, heads)
    assert all(torch.equal(logits[a], logits[0]) for a in range(n))
    v0 = fx[1][0, C:] + fx[5][:, None, None]
    assert float((ctx - v0).abs().max()) <= ctx_bound(n)
    check_exact(fx, rows, heads, n)


def test_warp_mha_fuse_odd_map_against_fp64():
    """13 x 11, C = 64, 8 heads (d = 8: the scale is not a power of two), Gaussian operands: against the restatement in fp64, as error
    relative to max |ctx|, no more than 4 x the error of the same restatement evaluated by torch in fp32 on the device."""
    n, C, heads, H, W = 3, 64, 8, 13, 11
    gen = torch.Generator().manual_seed(13)
    fx = [torch.randn(s, generator=gen).to(DEV) for s in ((C, H, W), (n, 2 * C, H, W), (C, H, W), (C,), (C,), (C,))]
    rows = shift_rows([(0.25, -0.5), (0.5, 1.0), (-1.5, 0.75)], H, W)
    ctx, ego, logits = run_kernel(fx, rows, heads)
    want_l, _, _, want_ctx, want_ego = restate(fx, rows, heads, exact=False)
    l32, _, _, ctx32, ego32 = restate(fx, rows, heads, torch.float32, DEV, exact=False)
    scale = float(want_ctx.abs().max())
    err_hip = float((ctx.cpu().double() - want_ctx).abs().max()) / scale
    err_t32 = float((ctx32.cpu().double() - want_ctx).abs().max()) / scale
    err_l = float((logits.cpu().double() - want_l).abs().max()) / float(want_l.abs().max())
    err_e = float((ego.cpu().double() - want_ego).abs().max())
    print(f"warp_mha_fuse 13x11x64 vs fp64: kernel {err_hip:.3e}, torch fp32 on the device {err_t32:.3e} (allowed 4 x); "
          f"logits {err_l:.3e} (torch fp32 {float((l32.cpu().double() - want_l).abs().max()) / float(want_l.abs().max()):.3e}), "
          f"warped ego {err_e:.3e} (torch fp32 {float((ego32.cpu().double() - want_ego).abs().max()):.3e})")
    assert err_hip <= 4 * err_t32, (err_hip, err_t32)


@pytest.mark.parametrize("grid_f64", [True, False])
def test_warp_mha_fuse_device_rows_equal_host_rows(grid_f64):
    """The rows as a float64 CUDA tensor (read by the kernel at run time) give the bits of the rows passed by value."""
    n, H, W, rows = device_rows_case()
    fx = mha_fixture(n, 8, 2, H, W, seed=21)
    with torch.no_grad():
        host = ops.warp_mha_fuse(*fx, 2, rows, grid_f64, return_logits=True)
        devr = ops.warp_mha_fuse(*fx, 2, torch.from_numpy(rows).to(DEV), grid_f64, return_logits=True)
    assert len(host) == 3 and all(float(t.abs().max()) > 0 for t in host)
    assert all(torch.equal(d, h) for d, h in zip(devr, host))


def test_warp_mha_fuse_rejects_bad_inputs():
    n, C, heads, H, W = 3, 32, 8, 8, 8
    q, kv, x, bq, bk, bv = mha_fixture(n, C, heads, H, W, seed=3)
    rows = shift_rows([(0.0, 0.0)] * n, H, W)
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.warp_mha_fuse(q.cpu(), kv, x, bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.warp_mha_fuse(q, kv.cpu(), x, bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="dtype"):
        ops.warp_mha_fuse(q.half(), kv, x, bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="dtype"):
        ops.warp_mha_fuse(q, kv.double(), x, bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="dtype"):
        ops.warp_mha_fuse(q, kv, x, bq, bk.double(), bv, heads, rows)
    with torch.enable_grad(), pytest.raises(_capi.HealAmdError, match="autograd"):     # (the suite runs under no_grad)
        ops.warp_mha_fuse(q, kv.clone().requires_grad_(True) * 2.0, x, bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="heads"):
        ops.warp_mha_fuse(q, kv, x, bq, bk, bv, 5, rows)
    with pytest.raises(_capi.HealAmdError, match="agents"):
        ops.warp_mha_fuse(q, kv.repeat(3, 1, 1, 1), x, bq, bk, bv, heads, shift_rows([(0.0, 0.0)] * 9, H, W))
    with pytest.raises(_capi.HealAmdError, match="kv_map"):
        ops.warp_mha_fuse(q, kv[:, :C], x, bq, bk, bv, heads, rows)                    # C instead of 2C channels
    with pytest.raises(_capi.HealAmdError, match="x_ego"):
        ops.warp_mha_fuse(q, kv, x[:, :4], bq, bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="bq"):
        ops.warp_mha_fuse(q, kv, x, bq[:4], bk, bv, heads, rows)
    with pytest.raises(_capi.HealAmdError, match="bv"):
        ops.warp_mha_fuse(q, kv, x, bq, bk, torch.cat([bv, bv]), heads, rows)
    with pytest.raises(_capi.HealAmdError, match="affine"):
        ops.warp_mha_fuse(q, kv, x, bq, bk, bv, heads, rows[:2])


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "where2comm_small.npz"))


@pytest.fixture(scope="module")
def gw():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "who2com_small.npz"))


def _timed(fn):
    calls = {}
    ops.TIMING = calls
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    return out, calls


@pytest.mark.parametrize("prefix", sorted(CASES))
def test_where2comm_module_on_device_matches_reference(g, prefix):
    model = make_w2c(prefix).to(DEV)
    x, rl, aff = case_inputs(g, prefix)
    x = x.to(DEV)
    with torch.no_grad():
        assert model.fused_ok(x, [int(v) for v in rl]) == (prefix != "odd_")       # 13 x 11: H W % 4 != 0, the torch path
    got, calls = _timed(lambda: model(x, rl, aff))
    assert (f"warp_mha_fuse_c{CASES[prefix]}" in calls) == (prefix != "odd_")      # the kernel ran: no quiet torch path
    assert rel_err(got.cpu().numpy(), g[f"{prefix}out"]) <= TOL, rel_err(got.cpu().numpy(), g[f"{prefix}out"])


@pytest.mark.parametrize("prefix", sorted(WHO_CASES))
def test_who2com_module_on_device_matches_reference(gw, prefix):
    model = make_who(prefix).to(DEV)
    x, rl, aff = case_inputs(gw, prefix)
    x = x.to(DEV)
    with torch.no_grad():
        assert model.fused_ok(x, [int(v) for v in rl])
    got, calls = _timed(lambda: model(x, rl, aff))
    assert "warp_att_fuse_levels" in calls and any(k.startswith("conv3x3") for k in calls)
    assert rel_err(got.cpu().numpy(), gw[f"{prefix}out"]) <= TOL, rel_err(got.cpu().numpy(), gw[f"{prefix}out"])


@pytest.mark.parametrize("method", ["where2comm", "who2com"])
def test_model_on_device_matches_reference(g, gw, method):
    from heal_amd.opencood.tools.train_utils import create_model
    gold = g if method == "where2comm" else gw
    model = fill_w2c(create_model(e2e_hypes(method))).to(DEV).eval()
    data = e2e_data(gold)
    data["inputs_m1"] = {k: v.to(DEV) for k, v in data["inputs_m1"].items()}
    data["pairwise_t_matrix"] = data["pairwise_t_matrix"].to(DEV)
    out, calls = _timed(lambda: model(data))
    if method == "where2comm":
        assert "warp_mha_fuse_c256" in calls
    else:
        assert "warp_att_fuse_levels" in calls and any(k.startswith("conv3x3") and k.endswith("_512_256") for k in calls)
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].cpu().numpy(), gold[f"e2e_{name}"])
        assert e <= TOL, (key, e)


def _vs_fp64(n, H, W, seed):
    from heal_amd import synth
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import Where2commFusion
    from oracle import oracle_np as O
    model = fill_w2c(Where2commFusion(256)).to(DEV).eval()
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn((n, 256, H, W), generator=gen) * 1.5).to(DEV)
    pw = synth.pairwise_t_matrix(synth.agent_poses(seed, n, r_min=4.0, r_max=30.0), 5)[None]
    aff = O.normalize_pairwise_tfm(pw, H * 0.4 * 2, W * 0.4 * 2, 1)
    rl = torch.tensor([n])
    with torch.no_grad():
        assert model.fused_ok(x, [n])
        got = model(x, rl, aff)
        model.fused = False
        assert not model.fused_ok(x, [n])
        ref32 = model(x, rl, aff)                  # the reference's own fp32 arithmetic on the device
        ref = model.double().forward_torch(x.double(), rl, aff)
    scale = float(ref.abs().max())
    err_hip = float((got.double() - ref).abs().max()) / scale
    err_ref32 = float((ref32.double() - ref).abs().max()) / scale
    print(f"Where2comm {n} agents {H}x{W}x256 vs fp64 torch: HIP path {err_hip:.3e}, torch fp32 path {err_ref32:.3e} "
          f"(ratio {err_hip / err_ref32:.2f}, allowed 4)")
    assert err_hip <= 4 * err_ref32, (err_hip, err_ref32)


def test_where2comm_lidar_baseline_size_vs_fp64():
    """5 agents at 128 x 128 x 256 (configs.lidar_baseline): the HIP path against the reference arithmetic in fp64 on the device,
    as error relative to the output's maximum, no more than 4 x the error of the reference's own fp32 arithmetic."""
    _vs_fp64(5, 128, 128, 11)


def test_where2comm_camera_size_vs_fp64():
    """3 agents at 64 x 64 x 256."""
    _vs_fp64(3, 64, 64, 13)


def test_where2comm_more_than_the_maximum_of_agents_falls_back_to_torch():
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import Where2commFusion
    top = ops.W2C_MAX_AGENTS
    model = fill_w2c(Where2commFusion(32)).to(DEV).eval()
    x = torch.randn((top + 1, 32, 8, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    aff = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (1, top + 1, top + 1, 1, 1))
    with torch.no_grad():
        assert not model.fused_ok(x, [top + 1]) and model.fused_ok(x[:top], [top])
        got = model(x, torch.tensor([top + 1]), aff)
        want = model.forward_torch(x, torch.tensor([top + 1]), aff)
        taken, calls = _timed(lambda: model(x[:top], torch.tensor([top]), aff))
        want_taken = model.forward_torch(x[:top], torch.tensor([top]), aff)
    assert torch.equal(got, want)
    assert "warp_mha_fuse_c32" in calls and rel_err(taken.cpu().numpy(), want_taken.cpu().numpy()) <= TOL


def test_where2comm_module_graph_capture_follows_weight_changes(g):
    """Capture the module and replay: the eager output.  Then change in_proj_weight and norm1.bias in place, run eagerly (which
    rebuilds the split weights), capture again and replay: the derived weights follow.  Single-stream captures."""
    model = make_w2c("n3_").to(DEV)
    x, rl, aff = case_inputs(g, "n3_")
    x = x.to(DEV)
    st = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(st):
        eager = model(x, rl, aff).clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            y = model(x, rl, aff)
        graph.replay()
        st.synchronize()
        assert torch.equal(y, eager)
        model.mha_fusion.attn.in_proj_weight.mul_(0.5)
        changed_w = model(x, rl, aff).clone()
        model.mha_fusion.norm1.bias.add_(0.25)
        changed = model(x, rl, aff).clone()
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2, stream=st):
            y2 = model(x, rl, aff)
        graph2.replay()
        st.synchronize()
        ref = model.forward_torch(x, rl, aff)
    assert not torch.equal(changed_w, eager) and not torch.equal(changed, changed_w)
    assert torch.equal(y2, changed)
    assert rel_err(changed.cpu().numpy(), ref.cpu().numpy()) <= TOL


def test_where2comm_pipeline_graph_replay_equals_eager():
    from heal_amd import configs, synth
    from heal_amd.pipeline import Scene, ScenePipeline
    pipe = ScenePipeline(configs.lidar_baseline("where2comm", SMALL_RANGE), DEV, seed=3)
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
@pytest.mark.parametrize("method", ["where2comm", "who2com"])
def test_gradient_path_on_device_matches_cpu(g, gw, method):
    """Under autograd the modules run the reference's torch arithmetic on the device: the golden output, and the gradients of the
    input and of every parameter equal the CPU's within 1e-4."""
    gold, make = (g, make_w2c) if method == "where2comm" else (gw, make_who)
    grads = {}
    for dev in ("cpu", DEV):
        model = make("n3_").to(dev)
        x, rl, aff = case_inputs(gold, "n3_")
        x = x.to(dev).requires_grad_(True)
        assert not model.fused_ok(x, [3])
        out = model(x, rl, aff)
        assert rel_err(out.detach().cpu().numpy(), gold["n3_out"]) <= TOL, dev
        out.square().mean().backward()
        grads[dev] = {"x": x.grad.cpu()}
        grads[dev].update({n: p.grad.cpu() for n, p in model.named_parameters()})
    for k, v in grads["cpu"].items():
        assert rel_err(grads[DEV][k].numpy(), v.numpy()) <= 1e-4, k
