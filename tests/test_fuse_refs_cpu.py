"""tests/fuse_refs.py proven without a GPU, on every fixture tests/test_gpu_fuse_conformance.py launches:
  1. each reference equals, to 1e-12, the float64 torch arithmetic of the module's own torch path (fusion_in_one.py:
     DiscoFusion.forward_torch; Where2commFusion's EncodeLayer attention fed the sampled maps) -- with the modules' warp replaced
     by the sampler on the kernels' fp32 taps, because float64 grid_sample forms other weights under a rotation (the sampler itself is
     proven against grid_sample in tests/test_coalign_refs_cpu.py, and on the identity fixtures the unpatched module is compared too);
  2. a statement-for-statement fp32 emulation of each kernel stays within the bound: the reference alone meets it;
  3. TEETH: every seeded defect of the kind the kernels can have exceeds the bound on at least one fixture."""
import numpy as np
import pytest
import torch

from heal_amd.opencood.models.fuse_modules import fusion_in_one as F1
from heal_amd.opencood.models.fuse_modules.where2comm_attn import EncodeLayer
from tests import fuse_refs as R

RTOL = 1e-12
M1, M2, M3 = R.M1, R.M2, R.M3


def close(a, b, tol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(np.abs(b), 1.0)).all())


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@pytest.fixture
def tap_warp(monkeypatch):
    """The modules' warp_affine_simple on the kernels' fp32 taps, evaluated in float64."""
    def warp(src, M, dsize):
        assert tuple(dsize) == tuple(src.shape[2:])
        return torch.from_numpy(R.sample_f64(src.numpy(), M.numpy())[0])
    monkeypatch.setattr(F1, "_warp_affine_simple", warp)


def test_rounding_counts_and_case_tables():
    k = R.disco_k(5, 36)
    assert (k["x"], k["l1"], k["l2"], k["l3"], k["l4"], k["p"], k["out"]) == (4, 42, 67, 32, 8, 13, 22)
    k = R.mha_k(3, 16)
    assert (k["s"], k["p"], k["out"]) == (6 + 5 + 1 + 16, 11, 19)
    for cases in (R.DISCO_CASES, R.MHA_CASES):
        assert {f"n{n}" for n in range(1, 9)} <= set(cases) and all(cases[f"n{n}"][0] == n for n in range(1, 9))
        assert all(H <= 37 and W <= 21 for _, _, H, W, _, _, _ in cases.values())
    assert sorted(c for _, c, *_ in R.DISCO_CASES.values() if c != 12) == sorted(R.DISCO_CHANNELS)
    assert [C // h for C, h in R.MHA_HEADS] == [1, 3, 3, 16, 16]
    assert float(np.exp(np.float32(-R.UNDERFLOW_GAP))) < 2.0 ** -149 / 2


@pytest.mark.parametrize("kernel", ["disco", "mha"])
def test_the_poses_do_what_the_suite_says(kernel):
    """rot: some neighbour is reached by part of the map; offmap: agent 1 by no pixel, agent 2 by some 16 x 4 tiles in full or in
    part and by most not at all; ego: the ego's own sample leaves the map."""
    cases = R.DISCO_CASES if kernel == "disco" else R.MHA_CASES
    for name, (n, _, H, W, pose, _, _) in cases.items():
        fx = R.disco_fixture(name) if kernel == "disco" else R.mha_fixture(name)
        rc = R.reached(fx["rows"], H, W)
        if pose == "rot" and H * W >= 64:
            assert rc[0].all() and any(r.any() and not r.all() for r in rc[1:]), name
        if pose == "offmap":
            assert rc[0].all() and not rc[1].any() and rc[2].any() and not rc[2].all(), name
            tiles = [rc[2][y:y + 4, x:x + 16] for y in range(0, H, 4) for x in range(0, W, 16)]
            assert any(t.any() and not t.all() for t in tiles) and any(not t.any() for t in tiles), name
        if pose == "ego":
            assert rc[0].any() and not rc[0].all(), name


# ------------------------------------------------------------------------------------------------- 1. against the modules
def disco_module(fx):
    """DiscoFusion in float64 with the fixture's folded weights: BatchNorm as the identity (running_var + eps = 1), conv1_1 =
    [W1n | W1e] without bias."""
    C = fx["C"]
    m = F1.DiscoFusion(C).double().eval()
    pw = m.pixel_weight_layer
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    with torch.no_grad():
        pw.conv1_1.weight.copy_(t(np.concatenate([fx["w1n"], fx["w1e"]], 1)).reshape(M1, 2 * C, 1, 1))
        pw.conv1_1.bias.zero_()
        pw.conv1_2.weight.copy_(t(fx["w2"]).reshape(M2, M1, 1, 1))
        pw.conv1_2.bias.copy_(t(fx["b2"]))
        pw.conv1_3.weight.copy_(t(fx["w3"]).reshape(M3, M2, 1, 1))
        pw.conv1_3.bias.copy_(t(fx["b3"]))
        pw.conv1_4.weight.copy_(t(fx["w4"]).reshape(1, M3, 1, 1))
        pw.conv1_4.bias.copy_(t(fx["b4"]))
        for bn in (pw.bn1_1, pw.bn1_2, pw.bn1_3):
            bn.running_var.fill_(1.0 - bn.eps)
    return m


def disco_module_out(fx):
    n = fx["n"]
    aff = np.zeros((1, n, n, 2, 3))
    aff[0, 0] = fx["rows"]
    with torch.no_grad():
        return disco_module(fx).forward_torch(torch.from_numpy(fx["feats"]).double(), torch.tensor([n]), aff)[0].numpy()


@pytest.mark.parametrize("name", sorted(R.DISCO_CASES))
def test_disco_reference_equals_the_module_in_float64(tap_warp, name):
    fx, ref = R.disco_fixture(name), R.disco_ref(name)
    assert close(ref["out"], disco_module_out(fx))
    assert (np.abs(ref["out"]) <= ref["T"] * (1 + 1e-12) + 1e-300).all() and np.isfinite(ref["B"]).all() and close(ref["p"].sum(0), 1.0)
    if fx["n"] * fx["H"] * fx["W"] >= 100 and fx["n"] > 1:          # both branches of the last ReLU
        assert (ref["logit"] > 0).mean() > 0.05 and (ref["logit"] == 0).mean() > 0.05, ((ref["logit"] > 0).mean(), name)


@pytest.mark.parametrize("name", ["identity3", "identity5"])
def test_disco_reference_against_the_unpatched_module_on_the_identity(name):
    """With torch's own float64 grid_sample: under the identity its weights differ from the fp32 taps by the rounding of the pixel
    coordinate only (a few EPS of the map's extent), which the logits amplify by the layers' gains: 1e-4 absolute is a guard against
    a sampler that is wrong altogether, no more."""
    fx, ref = R.disco_fixture(name), R.disco_ref(name)
    assert float(np.abs(ref["out"] - disco_module_out(fx)).max()) <= 1e-4


def mha_module_out(fx):
    """The module's attention (EncodeLayer.attn, an nn.MultiheadAttention in (agent, pixel, channel) order) in float64 with identity
    in- and out-projections and the fixture's biases, fed the maps sampled by the module's warp -> (ctx [C, H, W], the probabilities
    averaged over the heads [n, H, W])."""
    C, H, W, n = fx["C"], fx["H"], fx["W"], fx["n"]
    attn = EncodeLayer(C, n_head=fx["heads"]).double().eval().attn
    eye = torch.eye(C, dtype=torch.float64)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    with torch.no_grad():
        attn.in_proj_weight.copy_(torch.cat([eye, eye, eye]))
        attn.in_proj_bias.copy_(torch.cat([t(fx["bq"]), t(fx["bk"]), t(fx["bv"])]))
        attn.out_proj.weight.copy_(eye)
        attn.out_proj.bias.zero_()
        M = t(fx["rows"])
        tokens = lambda m: m.permute(0, 2, 3, 1).flatten(1, 2)      # noqa: E731  (fusion_in_one.py: Where2commFusion.forward_torch)
        q = tokens(F1._warp_affine_simple(t(fx["q_map"])[None], M[:1], (H, W)))
        kv = F1._warp_affine_simple(t(fx["kv_map"]), M, (H, W))
        ctx, w = attn(q, tokens(kv[:, :C]), tokens(kv[:, C:]))
    return ctx[0].t().reshape(C, H, W).numpy(), w[:, 0].t().reshape(n, H, W).numpy()


@pytest.mark.parametrize("name", sorted(R.MHA_CASES))
def test_mha_reference_equals_the_module_in_float64(tap_warp, name):
    """nn.MultiheadAttention scales q by the float64 1 / sqrt(d): the reference is evaluated with that number here (the GPU suite
    gives it the fp32 number the kernel receives)."""
    fx = R.mha_fixture(name)
    d = fx["C"] // fx["heads"]
    ref = R.mha_reference(*(fx[o] for o in R.MHA_OPERANDS), fx["heads"], float(d) ** -0.5, fx["rows"])
    ctx, w = mha_module_out(fx)
    assert close(ref["ctx"], ctx) and close(ref["p"].mean(1), w)
    assert (np.abs(ref["ctx"]) <= ref["T"] * (1 + 1e-12) + 1e-300).all() and np.isfinite(ref["B_ctx"]).all()
    x, xa = R.sample_f64(fx["x_ego"][None], fx["rows"][:1])
    assert ref["ego_warped"].dtype == np.float32 and R.max_ratio(ref["ego_warped"], x[0], ref["k"]["x"] * R.EPS * xa[0] * (1 + 1e-6)) <= 1.0
    assert abs(fx["scale"] - float(d) ** -0.5) <= R.EPS * float(d) ** -0.5


def test_large_logit_fixtures_have_dominated_pixels():
    """More than a tenth of the pixels (per head for Where2comm) have one agent leading every other by more than 105; there the
    float64 output is that agent's sample."""
    ref = R.disco_ref("large")
    dom, who = R.dominated(ref["logit"])
    assert dom.mean() > 0.1 and not dom.all()
    x, _ = R.sample_f64(R.disco_fixture("large")["feats"], R.disco_fixture("large")["rows"])
    pick = np.take_along_axis(x, who[None, None], 0)[0]
    assert float(np.abs(ref["out"] - pick)[:, dom].max()) < 1e-30
    ref = R.mha_ref("large")
    dom, _ = R.dominated(ref["logits"])
    assert dom.mean() > 0.1 and not dom.all()


# ------------------------------------------------------------------------------------------------- 2. emulation within the bound
@pytest.mark.parametrize("grid_f64", [True, False])
@pytest.mark.parametrize("name", sorted(R.DISCO_CASES))
def test_disco_emulation_is_within_the_bound(name, grid_f64):
    fx, ref = R.disco_fixture(name), R.disco_ref(name, grid_f64)
    out, scores = R.emulate_disco(*(fx[o] for o in R.DISCO_OPERANDS), fx["rows"], grid_f64)
    r_out, r_l = R.max_ratio(out, ref["out"], ref["B"]), R.max_ratio(scores, ref["logit"], ref["B_logit"])
    print(f"disco {name} grid_f64={grid_f64}: emulation err / bound out {r_out:.4f} scores {r_l:.4f}")
    assert r_out <= 1.0 and r_l <= 1.0
    assert R.max_ratio(f32(ref["out"]), ref["out"], ref["B"]) <= 1.0          # rounding the reference to fp32 stays inside
    own, B_own = R.disco_out_given_scores(fx["feats"], scores, fx["rows"], grid_f64)      # phase 2 on the emulation's own logits
    r_own = R.max_ratio(out, own, B_own)
    print(f"disco {name} grid_f64={grid_f64}: emulation err / bound out given its own scores {r_own:.4f}")
    assert r_own <= 1.0
    if fx["n"] > 1 and fx["H"] > 1 and fx["W"] > 1:
        # teeth of that check: phase 2 gathering the north-east and south-west taps from each other's address, the logits untouched
        n, C, H, W = fx["feats"].shape
        off, tw, _ = R.k5_taps(fx["rows"], H, W, grid_f64)
        v = fx["feats"].astype(np.float64).reshape(n, C, H * W)[
            np.arange(n)[:, None, None, None], np.arange(C)[None, :, None, None], off[..., [0, 2, 1, 3]][:, None]]
        xs = (v * tw[:, None]).sum(-1)
        lg = scores.astype(np.float64).reshape(n, -1)
        p = np.exp(lg - lg.max(0))
        p /= p.sum(0)
        assert R.max_ratio(f32((p[:, None] * xs).sum(0).reshape(C, H, W)), own, B_own) > 1.0
    if fx["n"] == 1:
        assert np.array_equal(out, R.sample_f32(fx["feats"], fx["rows"], grid_f64)[0] + np.float32(0))


@pytest.mark.parametrize("grid_f64", [True, False])
@pytest.mark.parametrize("name", sorted(R.MHA_CASES))
def test_mha_emulation_is_within_the_bound(name, grid_f64):
    fx, ref = R.mha_fixture(name), R.mha_ref(name, grid_f64)
    ctx, logits = R.emulate_mha(*(fx[o] for o in R.MHA_OPERANDS), fx["heads"], fx["scale"], fx["rows"], grid_f64)
    r_ctx, r_l = R.max_ratio(ctx, ref["ctx"], ref["B_ctx"]), R.max_ratio(logits, ref["logits"], ref["B_logits"])
    print(f"mha {name} grid_f64={grid_f64}: emulation err / bound ctx {r_ctx:.4f} logits {r_l:.4f}")
    assert r_ctx <= 1.0 and r_l <= 1.0
    assert R.max_ratio(f32(ref["ctx"]), ref["ctx"], ref["B_ctx"]) <= 1.0


# ------------------------------------------------------------------------------------------------- 3. teeth
def shifted_rows(rows):
    """Agent a samples through row a - 1 (the ego keeps its own)."""
    return rows[np.maximum(np.arange(len(rows)) - 1, 0)]


def disco_plain(fx, x, e0=None, keep=None, agents=None, w3=None, last_relu=True):
    """DiscoNet's reduction in float64 on samples x [n, C, P]; e0 [128, P] or per agent [n, 128, P]; keep [n, P] False drops an agent
    from the softmax; agents: the agents that take part at all -> (out [C, H, W], logits [n, H, W])."""
    n, C, H, W = fx["n"], fx["C"], fx["H"], fx["W"]
    d = lambda key: np.asarray(fx[key], np.float64)      # noqa: E731
    e0 = d("e0").reshape(M1, -1) if e0 is None else e0
    w3 = d("w3") if w3 is None else w3
    h1 = R.relu(np.einsum("mc,ncp->nmp", d("w1n"), x) + (e0[None] if e0.ndim == 2 else e0))
    h2 = R.relu(np.einsum("om,nmp->nop", d("w2"), h1) + d("b2")[None, :, None])
    h3 = R.relu(np.einsum("om,nmp->nop", w3, h2) + d("b3")[None, :, None])
    logit = np.einsum("o,nop->np", d("w4"), h3) + d("b4")[0]
    logit = R.relu(logit) if last_relu else logit
    lg = logit if keep is None else np.where(keep, logit, -np.inf)
    if agents is not None:
        lg, x = lg[agents], x[agents]
    e = np.exp(lg - lg.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    return (p[:, None] * x).sum(0).reshape(C, H, W), logit.reshape(n, H, W)


def disco_mutants(fx):
    n, C, H, W, rows = fx["n"], fx["C"], fx["H"], fx["W"], fx["rows"]
    x = R.sample_f64(fx["feats"], rows)[0].reshape(n, C, -1)
    mut = {"plain": disco_plain(fx, x)}
    e0s = R.sample_f64(np.repeat(fx["e0"][None], n, 0), rows)[0].reshape(n, M1, -1)
    mut["bias_added_before_sampling"] = disco_plain(fx, x, e0=e0s)
    rc = R.reached(rows, H, W).reshape(n, -1)
    if not rc.all():
        mut["out_of_reach_agent_dropped_from_the_softmax"] = disco_plain(fx, x, keep=rc | ~rc.any(0, keepdims=True))
    if n > 1:
        mut["ego_left_out_of_the_softmax"] = disco_plain(fx, x, agents=np.arange(1, n))
        mut["taps_of_agent_a_from_row_a_minus_1"] = disco_plain(fx, R.sample_f64(fx["feats"], shifted_rows(rows))[0].reshape(n, C, -1))
    mut["w3_transposed"] = disco_plain(fx, x, w3=np.asarray(fx["w3"], np.float64).reshape(M2, M3).T)
    mut["relu_missing_on_the_last_layer"] = disco_plain(fx, x, last_relu=False)
    return mut


def mha_plain(fx, q, k, v, keep=None, agents=None, head_of="div"):
    """Where2comm's reduction in float64 on q [C, P] (scaled), k, v [n, C, P] (biases added) -> (ctx [C, H, W], logits [n, heads, H, W])."""
    n, C, H, W, heads = fx["n"], fx["C"], fx["H"], fx["W"], fx["heads"]
    d = C // heads
    if head_of == "div":
        hd = lambda t: t.reshape(t.shape[:-2] + (heads, d, t.shape[-1]))      # noqa: E731
        back = lambda t: t.reshape(C, H, W)      # noqa: E731
    else:           # channel c belongs to head c % heads
        hd = lambda t: np.swapaxes(t.reshape(t.shape[:-2] + (d, heads, t.shape[-1])), -3, -2)      # noqa: E731
        back = lambda t: np.swapaxes(t, 0, 1).reshape(C, H, W)      # noqa: E731
    logits = (hd(q)[None] * hd(k)).sum(2)
    lg = logits if keep is None else np.where(keep[:, None], logits, -np.inf)
    vv = hd(v)
    if agents is not None:
        lg, vv = lg[agents], vv[agents]
    e = np.exp(lg - lg.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    return back((p[:, :, None] * vv).sum(0)), logits.reshape(n, heads, H, W)


def mha_mutants(fx):
    n, C, H, W, rows, s = fx["n"], fx["C"], fx["H"], fx["W"], fx["rows"], fx["scale"]
    d = lambda key: np.asarray(fx[key], np.float64)      # noqa: E731
    col = lambda b: d(b)[:, None]      # noqa: E731
    S = lambda m, r: R.sample_f64(m, r)[0].reshape(m.shape[0], m.shape[1], -1)      # noqa: E731
    qs, kv = S(d("q_map")[None], rows[:1])[0], S(d("kv_map"), rows)
    q, k, v = (qs + col("bq")) * s, kv[:, :C] + col("bk")[None], kv[:, C:] + col("bv")[None]
    mut = {"plain": mha_plain(fx, q, k, v)}
    bcol = lambda b: d(b)[None, :, None, None]      # noqa: E731
    kvb = S(d("kv_map") + np.concatenate([bcol("bk"), bcol("bv")], 1), rows)
    mut["bias_added_before_sampling"] = mha_plain(fx, S(d("q_map")[None] + bcol("bq"), rows[:1])[0] * s, kvb[:, :C], kvb[:, C:])
    rc = R.reached(rows, H, W).reshape(n, -1)
    if not rc.all():
        mut["out_of_reach_agent_dropped_from_the_softmax"] = mha_plain(fx, q, k, v, keep=rc | ~rc.any(0, keepdims=True))
    if n > 1:
        mut["ego_left_out_of_the_softmax"] = mha_plain(fx, q, k, v, agents=np.arange(1, n))
        kvr = S(d("kv_map"), shifted_rows(rows))
        mut["taps_of_agent_a_from_row_a_minus_1"] = mha_plain(fx, q, kvr[:, :C] + col("bk")[None], kvr[:, C:] + col("bv")[None])
    if C // fx["heads"] > 1:
        mut["q_not_scaled"] = mha_plain(fx, qs + col("bq"), k, v)
        if fx["heads"] > 1:
            mut["head_of_a_channel_taken_modulo_heads"] = mha_plain(fx, q, k, v, head_of="mod")
    mut["k_and_v_halves_swapped"] = mha_plain(fx, q, kv[:, C:] + col("bk")[None], kv[:, :C] + col("bv")[None])
    return mut


DISCO_MUTANTS = ["bias_added_before_sampling", "out_of_reach_agent_dropped_from_the_softmax", "ego_left_out_of_the_softmax",
                 "w3_transposed", "relu_missing_on_the_last_layer", "taps_of_agent_a_from_row_a_minus_1"]
MHA_MUTANTS = ["bias_added_before_sampling", "out_of_reach_agent_dropped_from_the_softmax", "ego_left_out_of_the_softmax",
               "q_not_scaled", "k_and_v_halves_swapped", "head_of_a_channel_taken_modulo_heads", "taps_of_agent_a_from_row_a_minus_1"]
_RATIOS = {}


def mutant_ratios(kernel):
    """mutant -> {case: largest err / bound over the outputs}, the fp32-rounded mutant against the reference; computed once."""
    if kernel not in _RATIOS:
        table = {}
        for name in (R.DISCO_CASES if kernel == "disco" else R.MHA_CASES):
            if kernel == "disco":
                fx, ref = R.disco_fixture(name), R.disco_ref(name)
                want = ((ref["out"], ref["B"]), (ref["logit"], ref["B_logit"]))
                muts = disco_mutants(fx)
            else:
                fx, ref = R.mha_fixture(name), R.mha_ref(name)
                want = ((ref["ctx"], ref["B_ctx"]), (ref["logits"], ref["B_logits"]))
                muts = mha_mutants(fx)
            for m, got in muts.items():
                table.setdefault(m, {})[name] = max(R.max_ratio(f32(g), r, b) for g, (r, b) in zip(got, want))
        _RATIOS[kernel] = table
    return _RATIOS[kernel]


@pytest.mark.parametrize("kernel", ["disco", "mha"])
def test_the_plain_restatement_is_within_the_bound_on_every_fixture(kernel):
    r = mutant_ratios(kernel)["plain"]
    assert len(r) == len(R.DISCO_CASES if kernel == "disco" else R.MHA_CASES) and max(r.values()) <= 1.0, r


@pytest.mark.parametrize("kernel,mutant", [("disco", m) for m in DISCO_MUTANTS] + [("mha", m) for m in MHA_MUTANTS])
def test_mutant_exceeds_the_bound(kernel, mutant):
    r = mutant_ratios(kernel)[mutant]
    caught = {name: v for name, v in r.items() if v > 1.0}
    print(f"{kernel} {mutant}: caught on {len(caught)} of {len(r)} fixtures it applies to; largest err / bound {max(r.values()):.3g}")
    assert caught, (kernel, mutant, r)
    assert any(name.startswith("n") and name[1:].isdigit() for name in caught), "no every-agent-count fixture catches it"
