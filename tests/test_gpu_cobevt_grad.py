"""CoBEVT's agent-window attention under autograd on the MI355X: heal_agent_window_attention_backward (ops.AgentWindowAttention)
against float64 autograd of the reference's composition (swap_fusion_modules.py:86-131 without the projections, restated below) on
the CPU, the deterministic dbias sum over parts, masked agents, refusals, and the opt-in module path (Attention.grad_kernel /
CoBEVT's `grad_kernel`) against the library composition and the same module in float64."""
import copy
import functools

import pytest
import torch

from tests.attention_refs import swap_groups as _groups, swap_ungroup as _ungroup
from tests.golden.detfill import fill_module

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

D, WS = 32, 4
BOUND = 2e-5        # what test_window_attention_backward_kernel_vs_float64_autograd holds the window backward to (T <= 256, d = 32)


def reference_fp64(qkv, bias, gout, n_valid, mode, heads, scale):
    """The composition in float64 on the CPU and its autograd -> (out, dqkv, dbias | None)."""
    L, H, W, _ = qkv.shape
    C = heads * D
    q64 = qkv.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True) if bias is not None else None
    g = _groups(q64, mode, L, H, W)                                # [G, T, 3 C]
    G, T = g.shape[:2]
    q, k, v = (g[..., i * C:(i + 1) * C].reshape(G, T, heads, D).permute(0, 2, 1, 3) for i in range(3))
    sim = torch.einsum("bhid,bhjd->bhij", q * scale, k)
    if b64 is not None:
        sim = sim + b64[None]
    key_ok = (torch.arange(T) // 16) < n_valid
    sim = sim.masked_fill(~key_ok[None, None, None, :], -float("inf"))
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), v)
    out = _ungroup(out.permute(0, 2, 1, 3).reshape(G, T, C), mode, L, H, W)
    (out * gout.detach().double().cpu()).sum().backward()
    return out.detach(), q64.grad, (b64.grad if b64 is not None else None)


def _inputs(L, H, W, heads, use_bias, seed):
    from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import _relative_position_index
    gen = torch.Generator().manual_seed(seed)
    C = heads * D
    qkv = torch.randn((L, H, W, 3 * C), generator=gen).cuda()
    gout = torch.randn((L, H, W, C), generator=gen).cuda()
    bias = None
    if use_bias:
        table = torch.randn(((2 * L - 1) * 49, heads), generator=gen)
        bias = table[_relative_position_index(L, WS)].permute(2, 0, 1).contiguous().cuda()
    return qkv, bias, gout


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _check(got_out, got_dqkv, got_dbias, ref, L, n_valid, heads, label):
    """out, the q / k / v thirds of dqkv per agent, and dbias: max-abs error over the max-abs of the float64 value, each within BOUND.
    dK / dV of masked agents are zero in the reference: there the kernel's must be exactly zero."""
    want_out, want_dqkv, want_dbias = ref
    C = heads * D
    figures = []
    if got_out is not None:
        figures.append(("out", _err(got_out, want_out)))
    for l in range(L):
        for i, third in enumerate("qkv"):
            g, w = got_dqkv[l, ..., i * C:(i + 1) * C], want_dqkv[l, ..., i * C:(i + 1) * C]
            if third != "q" and l >= n_valid:
                assert float(w.abs().max()) == 0.0
                assert bool((g == 0).all()), (label, f"d{third}[{l}] of a masked agent is not exactly zero")
            else:
                figures.append((f"d{third}[{l}]", _err(g, w)))
    if want_dbias is not None:
        figures.append(("dbias", _err(got_dbias, want_dbias)))
        assert bool((got_dbias[:, :, n_valid * 16:] == 0).all()), (label, "dbias columns of masked keys are not exactly zero")
    print(label, " ".join(f"{n}={e:.2e}" for n, e in figures))
    for name, e in figures:
        assert e <= BOUND, (label, name, e)


PAIRS = [(1, 1), (2, 1), (2, 2), (3, 2), (5, 3), (5, 5), (8, 5), (8, 8)]
KERNEL_CASES = [(mode, L, n, hw, 2, ub) for mode in ("window", "grid") for (L, n) in PAIRS for hw in ((4, 4), (8, 12))
                for ub in (True, False)] + [("window", 5, 3, (8, 12), 8, True), ("grid", 5, 3, (8, 12), 8, True)]


@pytest.mark.parametrize("mode,L,n_valid,hw,heads,use_bias", KERNEL_CASES)
def test_backward_kernel_vs_float64_autograd(mode, L, n_valid, hw, heads, use_bias):
    """ops.AgentWindowAttention (forward kernel + heal_agent_window_attention_backward) against float64 autograd of the reference's
    composition: out, dQ / dK / dV per agent (padded agents' dQ included) and dbias within 2e-5 of their own scale."""
    from heal_amd import ops
    H, W = hw
    qkv, bias, gout = _inputs(L, H, W, heads, use_bias, 1000 * L + 10 * n_valid + H + (1 if mode == "grid" else 0))
    scale = D ** -0.5
    qkv.requires_grad_(True)
    if bias is not None:
        bias.requires_grad_(True)
    out = ops.AgentWindowAttention.apply(qkv, bias, n_valid, mode, heads, D, WS, scale)
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    ref = reference_fp64(qkv, bias, gout, n_valid, mode, heads, scale)
    assert bool(torch.isfinite(qkv.grad).all())
    _check(out.detach(), qkv.grad, bias.grad if bias is not None else None, ref, L, n_valid, heads,
           f"{mode} L={L} n={n_valid} {H}x{W} heads={heads} bias={use_bias}")


@functools.lru_cache(maxsize=None)
def _parts_case(L, hw, mode):
    qkv, bias, gout = _inputs(L, hw, hw, 2, True, 77 + L + hw)
    scale = D ** -0.5
    return qkv, bias, gout, scale, reference_fp64(qkv, bias, gout, L, mode, 2, scale)


@pytest.mark.parametrize("mode", ["window", "grid"])
def test_parts_change_only_the_order_of_the_dbias_sum(mode):
    """16 x 16 (16 groups), L = 3, parts 1, 3 (uneven: 6 + 5 + 5) and 16: dqkv does not depend on the parts, dbias stays within the
    bound for each, and two launches with the same parts give the same bits (no atomics)."""
    from heal_amd import ops
    qkv, bias, gout, scale, ref = _parts_case(3, 16, mode)
    res = {}
    for parts in (1, 3, 16):
        dqkv, dbias = ops.agent_window_attention_backward(qkv, bias, gout, 3, mode, 2, D, WS, scale, parts=parts)
        again = ops.agent_window_attention_backward(qkv, bias, gout, 3, mode, 2, D, WS, scale, parts=parts)
        torch.cuda.synchronize()
        assert torch.equal(dbias, again[1]) and torch.equal(dqkv, again[0]), parts
        _check(None, dqkv, dbias, ref, 3, 3, 2, f"{mode} parts={parts}")
        res[parts] = dqkv
    assert torch.equal(res[1], res[3]) and torch.equal(res[1], res[16])


def test_policy_parts_on_a_larger_map():
    """32 x 32 at L = 5 with the library's own number of parts (a pure function of the shape, never more than the 64 groups)."""
    from heal_amd import _capi, ops
    qkv, bias, gout, scale, ref = _parts_case(5, 32, "grid")
    parts = _capi.lib().heal_agent_window_attention_backward_parts(5, 32, 32, 2)
    assert 1 <= parts <= 64
    dqkv, dbias = ops.agent_window_attention_backward(qkv, bias, gout, 5, "grid", 2, D, WS, scale)
    same = ops.agent_window_attention_backward(qkv, bias, gout, 5, "grid", 2, D, WS, scale, parts=parts)
    torch.cuda.synchronize()
    assert torch.equal(dbias, same[1]) and torch.equal(dqkv, same[0])
    _check(None, dqkv, dbias, ref, 5, 5, 2, f"grid policy parts={parts}")


@pytest.mark.parametrize("mode", ["window", "grid"])
@pytest.mark.parametrize("L,n_valid", [(5, 3), (5, 1), (2, 1)])
def test_masked_agents_reach_no_output(mode, L, n_valid):
    """K and V of the agents >= n_valid set to NaN: every output finite, their dK / dV rows and dbias columns exactly zero, the rest
    within the bound of the unpoisoned float64 reference."""
    from heal_amd import ops
    H, W, heads = 8, 12, 2
    qkv, bias, gout = _inputs(L, H, W, heads, True, 31 * L + n_valid)
    scale = D ** -0.5
    ref = reference_fp64(qkv, bias, gout, n_valid, mode, heads, scale)
    qkv[n_valid:, :, :, heads * D:] = float("nan")
    out = ops.agent_window_attention(qkv, bias, n_valid, mode, heads, D, WS, scale)
    dqkv, dbias = ops.agent_window_attention_backward(qkv, bias, gout, n_valid, mode, heads, D, WS, scale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dbias).all())
    _check(out, dqkv, dbias, ref, L, n_valid, heads, f"masked {mode} L={L} n={n_valid}")


def test_refusals(monkeypatch):
    """A wrong shape, a CPU tensor, n_valid out of range and an unsupported window raise HealAmdError before anything is launched."""
    from heal_amd import _capi, ops
    heads = 2
    qkv = torch.zeros((2, 8, 8, 3 * heads * D), device="cuda")
    out = torch.zeros((2, 8, 8, heads * D), device="cuda")
    bias = torch.zeros((heads, 32, 32), device="cuda")
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    bad = [
        dict(grad_out=out[:, :, :4]), dict(grad_out=out[:1]),  # grad_out of another shape
        dict(qkv=qkv[..., :-4]),                              # not 3 * heads * dim_head channels
        dict(bias=bias[:, :16]),                              # bias not [heads, T, T]
        dict(qkv=qkv.cpu()), dict(grad_out=out.cpu()),        # CPU tensors
        dict(n_valid=0), dict(n_valid=3),                     # outside 1..L
        dict(window=5), dict(window=8),                       # not instantiated
        dict(mode="diagonal"), dict(parts=5), dict(parts=-1),  # unknown grouping; more parts than the 4 groups
    ]
    for change in bad:
        kw = dict(qkv=qkv, bias=bias, grad_out=out, n_valid=1, mode="window", heads=heads, dim_head=D, window=WS, scale=1.0)
        kw.update(change)
        with pytest.raises(_capi.HealAmdError):
            ops.agent_window_attention_backward(**kw)
    assert launched == []
    assert not ops.agent_window_attention_train_supported(2, 5, D, 8, 8)
    assert not ops.agent_window_attention_train_supported(9, WS, D, 8, 8)
    assert ops.agent_window_attention_train_supported(8, WS, D, 8, 12)


# ---------------------------------------------------------------------------------------------------------------- module level
MODULE_ARGS = {"input_dim": 64, "mlp_dim": 64, "agent_size": 3, "window_size": 4, "dim_head": 32, "drop_out": 0.0, "depth": 2}


def _module_run(model, x, aff, dev, dtype):
    model = model.to(dev).to(dtype).train()
    model.zero_grad()
    xi = x.to(dev).to(dtype).requires_grad_(True)
    out = model(xi, torch.tensor([3, 1]), aff.to(dev).to(dtype))
    out.square().mean().backward()
    res = {"out": out.detach().double().cpu(), "x.grad": xi.grad.double().cpu()}
    res.update({n: p.grad.double().cpu() for n, p in model.named_parameters()})
    return res


def _module_case():
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import CoBEVT
    torch.manual_seed(23)
    on = fill_module(CoBEVT(dict(MODULE_ARGS, grad_kernel=True)))
    off = fill_module(CoBEVT(dict(MODULE_ARGS)))
    assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), off.state_dict().values()))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((4, 64, 8, 12), generator=gen)                # two scenes: 3 agents and 1 agent
    aff = torch.eye(2, 3)[None, None, None].repeat(2, 3, 3, 1, 1)
    aff[:, :, :, 0, 2] = 0.05                                     # a small shift: the warp interpolates
    return on, off, x, aff


class _CountBackward:
    def __init__(self, monkeypatch):
        from heal_amd import ops
        self.n = 0
        real = ops.agent_window_attention_backward

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, "agent_window_attention_backward", counted)


def test_module_kernel_path_against_float64(monkeypatch):
    """CoBEVT (64 channels = 2 heads, agent_size 3, depth 2, no dropout) in train(), scenes of 3 and 1 agents on 8 x 12 maps, loss
    mean(out^2): output, input gradient and every parameter gradient of the kernel path are as close to the float64 module as the
    library's fp32 composition is, within a factor 2 (two fp32 paths that differ in summation order; a wrong gradient is off by its
    own size), with a floor of 1e-6 relative.  The backward kernel ran for every attention of every scene.

    Measured on the MI355X: kernel / composition error ratios of 0.6 .. 1.7 over the 46 tensors above the floor (the largest:
    layers.1.grid_attention.fn.relative_position_bias_table.weight, 9.1e-6 against 5.3e-6), every error below 1.2e-5 of its tensor's
    scale.  The ratio of two errors of a few ulps scatters: with the softmax gradient's row term taken as rowsum(dO o O) from the
    saved output, three tensors were at 2.0 .. 2.6; the kernel forms it as sum_j P_j dP_j from its own tiles instead."""
    on, off, x, aff = _module_case()
    calls = _CountBackward(monkeypatch)
    ref = _module_run(copy.deepcopy(off), x, aff, "cpu", torch.float64)
    assert calls.n == 0
    torch_path = _module_run(off, x, aff, "cuda", torch.float32)
    assert calls.n == 0
    kernel_path = _module_run(on, x, aff, "cuda", torch.float32)
    assert calls.n == 2 * 2 * 2                                   # window + grid, depth 2, two scenes
    names = list(ref)
    assert any("relative_position_bias_table" in n for n in names) and len([n for n in names if "relative_position_bias_table" in n]) == 4
    failures = []
    for name in names:
        scale = float(ref[name].abs().max())
        assert scale > 0, name
        e_kernel = float((kernel_path[name] - ref[name]).abs().max()) / scale
        e_torch = float((torch_path[name] - ref[name]).abs().max()) / scale
        print(f"{name}: kernel {e_kernel:.3e} torch {e_torch:.3e}")
        if not e_kernel <= max(2.0 * e_torch, 1e-6):
            failures.append((name, e_kernel, e_torch))
    assert not failures, failures


def test_default_never_calls_the_backward_kernel(monkeypatch):
    """grad_kernel left at its default: the same training step runs the library's composition only."""
    from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import Attention
    _, off, x, aff = _module_case()
    assert Attention.grad_kernel is False and off.grad_kernel is False
    calls = _CountBackward(monkeypatch)
    res = _module_run(off, x, aff, "cuda", torch.float32)
    assert calls.n == 0 and bool(torch.isfinite(res["x.grad"]).all())
