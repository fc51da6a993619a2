"""CoBEVT's agent-window attention kernels element by element, every instantiation: k_agent_window_attn<L, 32> (heal_amd/csrc/
swap_attn.hip) and k_agent_window_attn_bwd<L, 32> with k_sum_parts (heal_amd/csrc/swap_attn_bwd.hip) for L = 1..8, both token orders,
with and without the per-head position bias, with 1, some and all agents valid.

Every assertion is one of: the per-element bound |got - ref| <= SAFETY * EPS * (k * T + E) + TINY on random floats, with k, T and E
derived in tests/attention_refs.py from the kernels' operation sequence (swap_k and the module docstring; proven to have teeth on the
CPU in tests/test_swap_refs_cpu.py); torch.equal on a fixture that needs nothing from expf beyond expf(0) == 1 and expf(x) == 0 for
x <= -200; or an exact zero.  Nothing is normalised by a tensor-wide maximum.  Operands lie inside NaN-poisoned buffers, the K and V
thirds of the masked agents hold NaN, and every output is NaN-prefilled inside a poisoned buffer: a read past an operand or of a
masked key poisons the result, every output word must have been written, and no word outside may change."""
import functools

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import attention_refs as R
from tests.test_gpu_attention_conformance import Operands, Worst, all_zero, equal, ratio
from tests.test_gpu_conformance import PAD, _assert_poison_outside

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D, WS = R.SWAP_D, R.SWAP_WS
SCALE = R.f32_scale(D)
PAIRS = [(L, n) for L in range(1, R.SWAP_MAX_L + 1) for n in sorted({1, (L + 1) // 2, L})]
CASES = [pytest.param(L, n, mode, id=f"L{L}_valid{n}_{mode}") for L, n in PAIRS for mode in ("window", "grid")]
KINDS = ("dq", "dk", "dv")


class Buffers(Operands):
    """Operands whose values may hold NaN on purpose: `unchanged` is a comparison of the words."""

    def check(self, what):
        for buf, view, src in self.ins:
            _assert_poison_outside(buf, PAD, PAD + src.numel(), what + ": operand")
            assert torch.equal(view.cpu().view(torch.int32), src.view(torch.int32)), what + ": an operand was modified"
        for buf, view in self.outs:
            _assert_poison_outside(buf, PAD, PAD + view.numel(), what + ": output")
            assert not bool(torch.isnan(view).any()), what + ": output words left unwritten (or NaN read)"


def poison_masked(qkv, n_valid, heads):
    """K and V of the agents >= n_valid set to NaN: the kernels never read a masked key tile."""
    q = qkv.copy()
    q[n_valid:, :, :, heads * D:] = np.nan
    return q


@functools.lru_cache(maxsize=None)
def case(L, n_valid, mode, regime, use_bias, heads=2, hw=(8, 12), parts=None):
    """Fixture and float64 reference, computed once and shared by the forward and the backward tests (never modified)."""
    fx = R.swap_data(L, regime, seed=10 * L + n_valid, n_valid=n_valid, H=hw[0], W=hw[1], heads=heads, use_bias=use_bias)
    ref = R.swap_reference(fx["qkv"], fx["bias"], fx["grad_out"], n_valid, mode, heads, SCALE, parts=parts)
    keep = ("out", "B_out", "grad_qkv", "B_grad_qkv", "grad_bias", "B_grad_bias", "T_grad_bias", "E_grad_bias")
    return fx, {k: ref[k] for k in keep}


def run_fwd(fx, n_valid, mode, heads, what):
    op = Buffers()
    qkv, b = op.put(poison_masked(fx["qkv"], n_valid, heads)), op.put(fx["bias"])
    L, H, W, _ = fx["qkv"].shape
    out = op.out((L, H, W, heads * D))
    res = ops.agent_window_attention(qkv, b, n_valid, mode, heads, D, WS, SCALE, out=out)
    assert res.data_ptr() == out.data_ptr()
    op.check(what)
    return out


def run_bwd(fx, n_valid, mode, heads, what, parts=None):
    op = Buffers()
    qkv, b, g = op.put(poison_masked(fx["qkv"], n_valid, heads)), op.put(fx["bias"]), op.put(fx["grad_out"])
    gq = op.out(fx["qkv"].shape)
    gb = None if fx["bias"] is None else op.out(fx["bias"].shape)
    rq, rb = ops.agent_window_attention_backward(qkv, b, g, n_valid, mode, heads, D, WS, SCALE, parts=parts, grad_qkv=gq, grad_bias=gb)
    assert rq.data_ptr() == gq.data_ptr() and (rb is None) == (gb is None) and (gb is None or rb.data_ptr() == gb.data_ptr())
    op.check(what)
    return gq, gb


def thirds(t, heads):
    C = heads * D
    return {k: t[..., i * C:(i + 1) * C] for i, k in enumerate(KINDS)}


def add_backward(worst, gq, gb, ref, n_valid, heads, tag, bias_bound=None):
    """The per-element bounds of dq / dk / dv (each third on its own) and grad_bias; exact zeros for the masked agents."""
    got, want, bound = thirds(gq, heads), thirds(ref["grad_qkv"], heads), thirds(ref["B_grad_qkv"], heads)
    for k in KINDS:
        worst.add(k, ratio(got[k], want[k], bound[k]), tag)
    assert all_zero(got["dk"][n_valid:]) and all_zero(got["dv"][n_valid:]), tag + ": dK / dV of a masked agent"
    if gb is not None:
        worst.add("grad_bias", ratio(gb, ref["grad_bias"], ref["B_grad_bias"] if bias_bound is None else bias_bound), tag)
        assert all_zero(gb[:, :, 16 * n_valid:]), tag + ": grad_bias columns of masked keys"


VARIANTS = [(regime, ub) for regime in ("spread", "large") for ub in (True, False)]


@pytest.mark.parametrize("L,n_valid,mode", CASES)
def test_forward_within_the_bound(L, n_valid, mode):
    """k_agent_window_attn<L, 32> on an 8 x 12 map (6 groups: both group indices reach a non-zero value, H != W), 2 heads: spread
    softmax and large logits, with and without the bias; two launches give the same bits."""
    worst = Worst("swap_forward", L=L, n_valid=n_valid, mode=mode)
    for regime, ub in VARIANTS:
        fx, ref = case(L, n_valid, mode, regime, ub)
        tag = f"{regime}{'' if ub else '_nobias'}"
        out = run_fwd(fx, n_valid, mode, 2, tag)
        worst.add("out", ratio(out, ref["out"], ref["B_out"]), tag)
        if regime == "spread":
            assert torch.equal(out, run_fwd(fx, n_valid, mode, 2, tag + " again")), "two launches differ"
    worst.done()


@pytest.mark.grad
@pytest.mark.parametrize("L,n_valid,mode", CASES)
def test_backward_within_the_bound(L, n_valid, mode):
    """k_agent_window_attn_bwd<L, 32> (+ k_sum_parts) with the library's own parts (6: one group each): dq, dk, dv and grad_bias
    element by element; masked agents' dK / dV rows and grad_bias columns are exact zeros; two launches give the same bits."""
    worst = Worst("swap_backward", L=L, n_valid=n_valid, mode=mode)
    for regime, ub in VARIANTS:
        fx, ref = case(L, n_valid, mode, regime, ub)
        tag = f"{regime}{'' if ub else '_nobias'}"
        gq, gb = run_bwd(fx, n_valid, mode, 2, tag)
        add_backward(worst, gq, gb, ref, n_valid, 2, tag)
        if regime == "spread":
            gq2, gb2 = run_bwd(fx, n_valid, mode, 2, tag + " again")
            assert torch.equal(gq, gq2) and (gb is None or torch.equal(gb, gb2)), "two launches differ"
    worst.done()


@pytest.mark.grad
@pytest.mark.parametrize("heads,hw", [(8, (8, 12)), (2, (4, 4))], ids=["heads8", "one_group"])
@pytest.mark.parametrize("mode", ["window", "grid"])
def test_eight_heads_and_a_single_group(mode, heads, hw):
    """L = 5 with 3 valid agents: 8 heads (h * D and the per-head bias up to h = 7), and a 4 x 4 map (one group, one part)."""
    worst = Worst("swap_shapes", heads=heads, hw=list(hw), mode=mode)
    for regime in ("spread", "large"):
        fx, ref = case(5, 3, mode, regime, True, heads, hw)
        out = run_fwd(fx, 3, mode, heads, regime)
        worst.add("out", ratio(out, ref["out"], ref["B_out"]), regime)
        gq, gb = run_bwd(fx, 3, mode, heads, regime)
        add_backward(worst, gq, gb, ref, 3, heads, regime)
    worst.done()


@pytest.mark.grad
@pytest.mark.parametrize("mode", ["window", "grid"])
def test_parts_change_only_the_order_of_the_grad_bias_sum(mode):
    """6 groups in 1 part, 4 parts (2 + 2 + 1 + 1) and 6 parts: grad_qkv does not depend on the parts, grad_bias is within the bound
    of each (k_bias follows the parts) and two launches with the same parts give the same bits (no atomics)."""
    L, n_valid = 3, 2
    worst = Worst("swap_parts", L=L, n_valid=n_valid, mode=mode)
    fx, ref = case(L, n_valid, mode, "spread", True)
    first = None
    for parts in (1, 4, 6):
        gq, gb = run_bwd(fx, n_valid, mode, 2, f"parts={parts}", parts=parts)
        gq2, gb2 = run_bwd(fx, n_valid, mode, 2, f"parts={parts} again", parts=parts)
        assert torch.equal(gq, gq2) and torch.equal(gb, gb2), parts
        add_backward(worst, gq, gb, ref, n_valid, 2, f"parts={parts}", R.swap_bias_bound(ref, L, n_valid, D, 6, parts))
        first = gq if first is None else first
        assert torch.equal(first, gq), f"grad_qkv depends on parts ({parts})"
    worst.done()


@pytest.mark.grad
@pytest.mark.parametrize("L,n_valid,mode", CASES)
def test_exact_uniform_and_selector(L, n_valid, mode):
    """q = 0 and integer k, v, dO.  uniform (no bias; n_valid a power of two): out is the mean of the valid v rows, dV_j the mean of dO
    over all queries for every valid key, dK = 0.  selector (bias 0 at (i, pi_h(i)), -256 elsewhere; pi_h crosses agent tiles, is not
    symmetric and differs between the heads): out_i == v_pi(i), dV_j == the sum of the dO_i that selected j, dQ == dK == grad_bias
    == 0.  All bit for bit; a bias read transposed or from the other head, a V row of another token or agent, or window order for
    grid selects other integers."""
    C = 2 * D
    for regime in ("uniform", "selector"):
        if regime == "uniform" and n_valid & (n_valid - 1):
            continue
        fx = R.swap_data(L, regime, seed=1, n_valid=n_valid)
        ex = R.swap_exact(fx, n_valid, mode, 2, regime)
        assert ex["units"] < R.EXACT_LIMIT
        out = run_fwd(fx, n_valid, mode, 2, regime)
        assert equal(out, ex["out"]), regime + ": out"
        gq, gb = run_bwd(fx, n_valid, mode, 2, regime)
        got = thirds(gq, 2)
        assert equal(got["dk"], ex["dk"]) and equal(got["dv"], ex["dv"]), regime + ": dK / dV"
        if regime == "selector":
            assert all_zero(got["dq"]) and all_zero(gb), "selector: dQ / grad_bias"
        assert gq.shape[-1] == 3 * C


def test_new_refusals(monkeypatch):
    """Destinations of another shape, dtype or device, non-contiguous ones, a grad_bias without a bias and a qkv that is not
    4-dimensional raise HealAmdError before anything is launched."""
    heads, L, H, W = 2, 2, 8, 8
    z = lambda *s, **k: torch.zeros(s, device=DEV, **k)      # noqa: E731
    qkv, g, bias = z(L, H, W, 3 * heads * D), z(L, H, W, heads * D), z(heads, 16 * L, 16 * L)
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    bad = pytest.raises(_capi.HealAmdError)
    fwd = lambda qkv=qkv, **kw: ops.agent_window_attention(qkv, bias, 1, "window", heads, D, WS, 1.0, **kw)      # noqa: E731
    for out in (z(L, H, W, heads * D + 4), z(L * H, W, heads * D), z(L, H, W, heads * D, dtype=torch.float64),
                z(L, H, W, heads * D).cpu(), z(L, H, W, 2 * heads * D)[..., ::2], z(L, H, W, heads * D).tolist()):
        with bad:
            fwd(out=out)
    with bad:
        fwd(qkv=qkv.reshape(L * H, W, -1))
    with bad:
        fwd(qkv=qkv[0])
    bwd = lambda b=bias, **kw: ops.agent_window_attention_backward(qkv, b, g, 1, "window", heads, D, WS, 1.0, **kw)      # noqa: E731
    for gq in (z(L, H, W, 3 * heads * D + 4), z(L, H * W, 3 * heads * D), qkv.double(), qkv.cpu(), z(L, H, W, 6 * heads * D)[..., ::2]):
        with bad:
            bwd(grad_qkv=gq)
    for gb in (z(heads, 16 * L, 16 * L + 4), z(heads * 16 * L, 16 * L), bias.half(), bias.cpu(), z(heads, 16 * L, 32 * L)[..., ::2]):
        with bad:
            bwd(grad_bias=gb)
    with bad:
        bwd(b=None, grad_bias=z(heads, 16 * L, 16 * L))
    assert launched == []
    gq, gb = z(L, H, W, 3 * heads * D), z(heads, 16 * L, 16 * L)
    rq, rb = bwd(grad_qkv=gq, grad_bias=gb)
    assert rq is gq and rb is gb and launched == ["heal_agent_window_attention_backward"]
