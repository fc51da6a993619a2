"""The V2X-ViT attention kernels element by element, every instantiation: K6b (heal_amd/csrc/window_attn.hip: all seven
(window, dim_head) pairs of HEAL_WA / HEAL_WAB, forward and backward, with and without the position bias) and K6
(heal_amd/csrc/agent_attn.hip: 4 head counts x 8 agent counts x 2 layouts, forward and backward).

Every assertion is one of: the per-element bound |got - ref| <= SAFETY * EPS * (k * T + E) + TINY on random floats, with k, T and E
derived in tests/attention_refs.py from the kernel's operation sequence (window_k, agent_k and the module docstring; proven to
have teeth on the CPU in tests/test_attention_refs_cpu.py); torch.equal on a fixture that needs nothing from expf beyond
expf(0) == 1 and expf(x) == 0 for x <= -200; or an exact zero.  Nothing is normalised by a tensor-wide maximum.  Operands lie inside
NaN-poisoned buffers and every output is NaN-prefilled inside one: a read past an operand poisons the result, every output word
must have been written, and no word outside may change.  The operators are called directly; no autograd graph is recorded.

A behaviour that differs from a `safe` softmax on purpose: with EVERY key masked the row maximum is -inf and the kernels produce
NaN, as the reference's masked_fill(-inf).softmax does.  No test here masks every key."""
import functools

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import attention_refs as R
from tests.report import note
from tests.test_gpu_conformance import PAD, POISON, _assert_poison_outside, _poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------ buffers
class Operands:
    """Poisoned operands and outputs of one launch: check() holds the launch to `every output word written, nothing else touched`."""

    def __init__(self):
        self.ins, self.outs = [], []

    def put(self, a):
        if a is None:
            return None
        src = torch.from_numpy(np.ascontiguousarray(a))
        if src.dtype == torch.int32:            # the key mask: the same layout as _poisoned, in int32 words
            buf = torch.full((PAD + (src.numel() + 3) // 4 * 4 + PAD,), POISON, dtype=torch.int32, device=DEV)
            view = buf[PAD:PAD + src.numel()]
            view.copy_(src.to(DEV))
        else:
            buf, view = _poisoned(src)
        self.ins.append((buf, view, src))
        return view

    def out(self, shape):
        buf, view = _poisoned(torch.full(tuple(shape), float("nan")))
        self.outs.append((buf, view))
        return view

    def check(self, what):
        for buf, view, src in self.ins:
            _assert_poison_outside(buf, PAD, PAD + src.numel(), what + ": operand")
            assert torch.equal(view.cpu(), src), what + ": an operand was modified"
        for buf, view in self.outs:
            _assert_poison_outside(buf, PAD, PAD + view.numel(), what + ": output")
            assert not bool(torch.isnan(view).any()), what + ": output words left unwritten (or NaN read)"


def ratio(got, ref, bound):
    return R.max_ratio(got.detach().cpu().double().numpy(), ref, bound)


def equal(got, ref64):
    """Bit for bit: the float64 value is an fp32 number (checked) and equals the kernel's output."""
    ref64 = torch.from_numpy(np.ascontiguousarray(ref64, np.float64))
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64)
    return torch.equal(got.detach().cpu(), ref32)


def all_zero(t):
    return int(torch.count_nonzero(t)) == 0


class Worst:
    """The largest err / bound per output over the variants of one parametrised case: recorded, then asserted."""

    def __init__(self, name, **tags):
        self.name, self.tags, self.r = name, tags, {}

    def add(self, output, value, variant):
        if value > self.r.get(output, (-1.0, None))[0]:
            self.r[output] = (value, variant)

    def done(self):
        for output, (value, variant) in self.r.items():
            print(f"{self.name}:{output} {self.tags}: largest err / bound = {value:.4f} at {variant}")
            note(f"{self.name}:{output}", ratio=value, at=str(variant), **self.tags)
        bad = {o: v for o, v in self.r.items() if not v[0] <= 1.0}
        assert not bad, (self.name, self.tags, bad)


# ================================================================================================================ K6b
M_HEADS, L_AGENTS = 2, 2


@functools.lru_cache(maxsize=None)
def window_case(ws, d, regime, use_bias):
    """Fixture and float64 reference, computed once and shared by the forward and the backward test (never modified)."""
    fx = R.window_data(ws, d, regime, seed=ws + d, L=L_AGENTS, m=M_HEADS)
    bias = fx["bias"] if use_bias else None
    ref = R.window_reference(fx["qkv"], bias, fx["grad_out"], M_HEADS, d, ws, R.f32_scale(d))
    keep = ("out", "B_out", "grad_qkv", "B_grad_qkv", "grad_bias", "B_grad_bias")
    return fx, bias, {k: ref[k] for k in keep}


def run_window_fwd(fx, bias, ws, d, what):
    op = Operands()
    qkv, b = op.put(fx["qkv"]), op.put(bias)
    L, H, W, _ = fx["qkv"].shape
    out = op.out((L, H, W, M_HEADS * d))
    res = ops.window_attention(qkv, b, M_HEADS, d, ws, R.f32_scale(d), out=out)
    assert res.data_ptr() == out.data_ptr()
    op.check(what)
    return out


def run_window_bwd(fx, bias, out, ws, d, what):
    op = Operands()
    qkv, b, o, g = op.put(fx["qkv"]), op.put(bias), op.put(out.cpu().numpy()), op.put(fx["grad_out"])
    gq = op.out(fx["qkv"].shape)
    res, gb = ops.window_attention_backward(qkv, b, o, g, M_HEADS, d, ws, R.f32_scale(d), grad_qkv=gq)
    assert res.data_ptr() == gq.data_ptr() and (gb is None) == (bias is None)
    op.check(what)
    return gq, gb


WINDOW_CASES = [pytest.param(ws, d, b, id=f"ws{ws}_d{d}_{'bias' if b else 'nobias'}") for ws, d in R.WINDOW_SHAPES for b in (True, False)]


@pytest.mark.parametrize("ws,d,use_bias", WINDOW_CASES)
def test_window_attention_forward_within_the_bound(ws, d, use_bias):
    """k_window_attn<ws, d> on a (2 ws) x (3 ws) map, 2 agents, 2 heads (6 windows per agent: row and column index non-zero, H != W;
    ws = 16 is the only size whose waves own two query slabs each).  Spread softmax and large logits (finite, within the bound);
    two launches give the same bits."""
    worst = Worst("k6b_forward", ws=ws, d=d, bias=use_bias)
    for regime in ("spread", "large"):
        fx, bias, ref = window_case(ws, d, regime, use_bias)
        out = run_window_fwd(fx, bias, ws, d, f"forward {regime}")
        worst.add("out", ratio(out, ref["out"], ref["B_out"]), regime)
        assert torch.equal(out, run_window_fwd(fx, bias, ws, d, f"forward {regime} again")), "two launches differ"
    worst.done()


@pytest.mark.parametrize("ws,d,use_bias", WINDOW_CASES)
def test_window_attention_backward_within_the_bound(ws, d, use_bias):
    """k_window_attn_bwd_q / _bwd_kv<ws, d> on the forward's own output.  grad_qkv is deterministic (two launches: the same bits);
    grad_bias is summed by atomics over 2 agents x 6 windows x 2 heads in any order and is held to its bound both times."""
    worst = Worst("k6b_backward", ws=ws, d=d, bias=use_bias)
    for regime in ("spread", "large"):
        fx, bias, ref = window_case(ws, d, regime, use_bias)
        out = run_window_fwd(fx, bias, ws, d, f"forward {regime}")
        assert ratio(out, ref["out"], ref["B_out"]) <= 1.0
        gq, gb = run_window_bwd(fx, bias, out, ws, d, f"backward {regime}")
        gq2, gb2 = run_window_bwd(fx, bias, out, ws, d, f"backward {regime} again")
        worst.add("grad_qkv", ratio(gq, ref["grad_qkv"], ref["B_grad_qkv"]), regime)
        assert torch.equal(gq, gq2), "two launches differ"
        if use_bias:
            for t in (gb, gb2):
                worst.add("grad_bias", ratio(t, ref["grad_bias"], ref["B_grad_bias"]), regime)
    worst.done()


def window_parts(t, ws, parts, d):
    """[L,H,W,parts*m*d] device tensor -> [parts, B, T, d] float64 numpy."""
    return R.window_split(t.detach().cpu().double().numpy(), ws, parts, M_HEADS, d)


@pytest.mark.parametrize("ws,d", R.WINDOW_SHAPES)
def test_window_attention_exact_uniform(ws, d):
    """q = 0, no bias, integer k, v, dO: e = expf(0) = 1, sum = T, inv = 1 / T (a power of two).  out is the window mean of v, dV the
    window mean of dO (the same in every row), dK = scale * sum_q 0 * dS = 0 -- bit for bit."""
    T = ws * ws
    fx = R.window_data(ws, d, "uniform", seed=1, L=L_AGENTS, m=M_HEADS)
    assert R.window_exact_units(fx, T, d, "uniform") < R.EXACT_LIMIT
    v = R.window_split(fx["qkv"].astype(np.float64), ws, 3, M_HEADS, d)[2]
    g = R.window_split(fx["grad_out"].astype(np.float64), ws, 1, M_HEADS, d)[0]
    L, H, W, _ = fx["qkv"].shape
    out = run_window_fwd(fx, None, ws, d, "uniform forward")
    mean = lambda t: np.broadcast_to(t.sum(1, keepdims=True) / T, t.shape)[None]      # noqa: E731
    assert equal(out, R.window_merge(mean(v), L, H, W, ws, M_HEADS, d))
    gq, gb = run_window_bwd(fx, None, out, ws, d, "uniform backward")
    dq, dk, dv = window_parts(gq, ws, 3, d)
    assert gb is None and np.array_equal(dv, mean(g)[0]) and not dk.any()
    assert float(np.abs(v.sum(1)).max()) > 0 and float(np.abs(g.sum(1)).max()) > 0


@pytest.mark.parametrize("ws,d", R.WINDOW_SHAPES)
def test_window_attention_exact_bias_selector(ws, d):
    """q = 0, bias[i, pi(i)] = 0 and -256 elsewhere for the non-symmetric permutation pi(i) = (5 i + 3) mod T: the probabilities are
    exactly one-hot, out[i] == v[pi(i)], dV[pi(i)] == dO[i] (pi is a bijection) and dQ == dK == grad_bias == 0, bit for bit.  A bias
    read transposed, from another row, or a V row of another token selects a different integer row."""
    T = ws * ws
    pi = R.window_perm(T)
    fx = R.window_data(ws, d, "selector", seed=1, L=L_AGENTS, m=M_HEADS)
    assert R.window_exact_units(fx, T, d, "selector") < R.EXACT_LIMIT
    v = R.window_split(fx["qkv"].astype(np.float64), ws, 3, M_HEADS, d)[2]
    g = R.window_split(fx["grad_out"].astype(np.float64), ws, 1, M_HEADS, d)[0]
    L, H, W, _ = fx["qkv"].shape
    out = run_window_fwd(fx, fx["bias"], ws, d, "selector forward")
    assert equal(out, R.window_merge(v[None][:, :, pi], L, H, W, ws, M_HEADS, d))
    gq, gb = run_window_bwd(fx, fx["bias"], out, ws, d, "selector backward")
    dq, dk, dv = window_parts(gq, ws, 3, d)
    assert np.array_equal(dv[:, pi], g), "dV[pi(i)] != dO[i]"
    assert not dq.any() and not dk.any() and all_zero(gb)


# ================================================================================================================= K6
def agent_rows(L):
    return sorted({1, L} | ({(L + 1) // 2} if L >= 3 else set()))


@functools.lru_cache(maxsize=None)
def agent_plan(heads, L):
    """The variants of one (heads, L) and their float64 references in pixel-major layout, computed once and shared by both
    layouts and by the forward and the backward test.  -> [(tag, data, key_mask, out_rows, reference or None for an exact one)]"""
    scale = R.f32_scale(R.C_AGENT // heads)
    plan = []

    def add(tag, fx, km, rows, exact=False):
        ref = None if exact else R.agent_reference(fx["q"], fx["k"], fx["v"], fx["grad_out"][:, :rows], heads, scale, km, rows)
        plan.append((tag, fx, km, rows, ref))

    spread = R.agent_data(heads, L, 5, "spread", seed=heads * 10 + L)          # one full block of 4 pixels + a block of 1
    ints = R.agent_data(heads, L, 5, "ints", seed=heads * 10 + L)
    large = R.agent_data(heads, L, 5, "large", seed=heads * 10 + L)
    one = R.agent_data(heads, L, 1, "spread", seed=heads * 10 + L + 1)
    masks = R.agent_masks(L, spread["q"], spread["k"], heads, scale) if L >= 2 else {}
    for rows in agent_rows(L):
        add(f"spread_rows{rows}", spread, None, rows, exact=L == 1)
        for name in ("first", "top"):
            if name in masks:
                add(f"spread_rows{rows}_mask-{name}", spread, masks[name], rows)
        if L >= 2:
            add(f"ints_rows{rows}_mask-single", ints, masks["single"], rows, exact=True)
        else:
            add(f"ints_rows{rows}", ints, None, rows, exact=True)
        add(f"large_rows{rows}", large, None, rows, exact=L == 1)
    add("spread_1pixel", one, None, L, exact=L == 1)
    return plan


def agent_launch(fx, km, rows, heads, am, backward, what):
    op = Operands()
    lay = lambda a: R.to_layout(a, am)      # noqa: E731
    q, k, v, mask = op.put(lay(fx["q"])), op.put(lay(fx["k"])), op.put(lay(fx["v"])), op.put(km)
    scale = R.f32_scale(R.C_AGENT // heads)
    P, L, C = fx["q"].shape
    if not backward:
        out = op.out((rows, P, C) if am else (P, rows, C))
        res = (ops.agent_attention(q, k, v, heads, scale, key_mask=mask, out_rows=rows, agent_major=am, out=out),)
    else:
        g = op.put(lay(fx["grad_out"][:, :rows]))
        grads = tuple(op.out(q.shape) for _ in range(3))
        res = ops.agent_attention_backward(q, k, v, g, heads, scale, key_mask=mask, agent_major=am, grads=grads)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, grads))
    op.check(what)
    return [R.from_layout(t.cpu().numpy(), am) for t in res]          # pixel-major float32 numpy


AGENT_CASES = [pytest.param(h, L, am, id=f"h{h}_L{L}_{'agent' if am else 'pixel'}-major")
               for h in R.AGENT_HEADS for L in range(1, R.AGENT_MAX_L + 1) for am in (False, True)]


def the_key(km, L):
    return 0 if km is None else int(np.flatnonzero(km)[0])


@pytest.mark.parametrize("heads,L,am", AGENT_CASES)
def test_agent_attention_forward_every_instantiation(heads, L, am):
    """k_agent_attn<64 / heads, L, am> at 5 pixels (a full block of 4 and a block of 1) and at 1 pixel; out_rows in {1, ceil(L / 2), L};
    no mask, key 0 masked, the highest-scoring key masked (spread data), all but key L // 2 masked (out == v_j exactly in every
    row); large logits; L = 1: out == v exactly."""
    worst = Worst("k6_forward", heads=heads, L=L, agent_major=am)
    for i, (tag, fx, km, rows, ref) in enumerate(agent_plan(heads, L)):
        out, = agent_launch(fx, km, rows, heads, am, False, tag)
        if ref is None:
            assert np.array_equal(out, np.repeat(fx["v"][:, the_key(km, L)][:, None], rows, 1)), tag
        else:
            worst.add("out", R.max_ratio(out, ref["out"], ref["B_out"]), tag)
        if i == 0:
            assert np.array_equal(out, agent_launch(fx, km, rows, heads, am, False, tag + " again")[0]), "two launches differ"
    worst.done()


@pytest.mark.parametrize("heads,L,am", AGENT_CASES)
def test_agent_attention_backward_every_instantiation(heads, L, am):
    """k_agent_attn_bwd<64 / heads, L, am> on the variants of the forward test.  grad_q rows at or beyond out_rows are exactly 0;
    a masked key's grad_k and grad_v are exactly 0 (their bound is 0); one unmasked key: dq == dk == 0 and dv_j == sum_i dO_i on
    integer dO, bit for bit."""
    worst = Worst("k6_backward", heads=heads, L=L, agent_major=am)
    for i, (tag, fx, km, rows, ref) in enumerate(agent_plan(heads, L)):
        gq, gk, gv = agent_launch(fx, km, rows, heads, am, True, tag)
        assert not gq[:, rows:].any(), tag + ": grad_q beyond out_rows"
        if ref is None:
            j = the_key(km, L)
            want = np.zeros_like(gv)
            want[:, j] = fx["grad_out"][:, :rows].astype(np.float64).sum(1)
            if tag.startswith("ints"):
                assert np.array_equal(gv, want), tag
            else:               # L == 1 on floats: out_rows == 1, dv = 1 * dO
                assert rows == 1 and np.array_equal(gv, fx["grad_out"][:, :1]), tag
            assert not gq.any() and not gk.any(), tag
        else:
            for name, got in (("grad_q", gq), ("grad_k", gk), ("grad_v", gv)):
                worst.add(name, R.max_ratio(got, ref[name], ref["B_" + name]), tag)
            if km is not None:
                assert not gk[:, km == 0].any() and not gv[:, km == 0].any(), tag + ": gradient of a masked key"
        if i == 0:
            again = agent_launch(fx, km, rows, heads, am, True, tag + " again")
            assert all(np.array_equal(a, b) for a, b in zip((gq, gk, gv), again)), "two launches differ"
    worst.done()


# ========================================================================================================== refusals
def test_attention_wrappers_reject_bad_inputs():
    """Every operand the kernels read from a bare pointer is checked against q (qkv) before anything is launched: each call here
    must raise, none may reach the device."""
    bad = pytest.raises(_capi.HealAmdError)
    z = lambda *s: torch.zeros(s, device=DEV)      # noqa: E731
    L, P = 3, 6
    q, k, v = z(P, L, 256), z(P, L, 256), z(P, L, 256)
    ones = lambda n: torch.ones(n, dtype=torch.int32, device=DEV)      # noqa: E731
    for fwd in (True, False):
        def call(q=q, k=k, v=v, g=None, **kw):
            if fwd:
                return ops.agent_attention(q, k, v, 8, 0.17, **kw)
            kw.pop("out_rows", None)
            return ops.agent_attention_backward(q, k, v, z(P, L, 256) if g is None else g, 8, 0.17, **kw)
        with bad:
            call(k=z(P, L - 1, 256))                    # fewer keys than queries
        with bad:
            call(v=z(P - 1, L, 256))                    # a v with fewer pixels
        with bad:
            call(v=z(L, P, 256))                        # the other layout's shape
        with bad:
            call(key_mask=ones(L - 1))
        with bad:
            call(key_mask=ones(L + 1))
        with bad:
            call(key_mask=ones(L).long())
        with bad:
            call(q=z(P, 9, 256), k=z(P, 9, 256), v=z(P, 9, 256), g=z(P, 9, 256))        # L above AGENT_ATTENTION_MAX_AGENTS
        with bad:
            call(q=z(P, L, 128), k=z(P, L, 128), v=z(P, L, 128), g=z(P, L, 128))        # a last dimension other than 256
        with bad:
            call(q=z(P * L, 256), k=z(P * L, 256), v=z(P * L, 256))
        with bad:
            call(q=q.double())
    assert ops.AGENT_ATTENTION_MAX_AGENTS == 8
    for rows in (0, L + 1, -1):
        with bad:
            ops.agent_attention(q, k, v, 8, 0.17, out_rows=rows)
    with bad:
        ops.agent_attention(q, k, v, 3, 0.17)                                            # heads: refused by the library before a launch
    with bad:
        ops.agent_attention(q, k, v, 8, 0.17, out=z(P, L - 1, 256))
    with bad:
        ops.agent_attention(q, k, v, 8, 0.17, agent_major=True, out=z(L, P, 256))          # q is [L = 6, n_pix = 3] there
    for g in (z(P, L + 1, 256), z(P, 0, 256), z(P - 1, L, 256), z(P, L, 128), z(P * L, 256), z(L, P, 256)[:, :P - 1]):
        with bad:
            ops.agent_attention_backward(q, k, v, g, 8, 0.17)
    with bad:
        ops.agent_attention_backward(q, k, v, z(L + 1, P, 256), 8, 0.17, agent_major=True)
    with bad:
        ops.agent_attention_backward(q, k, v, z(P, L, 256), 8, 0.17, grads=(z(P, L, 256), z(P, L, 256), z(P, L - 1, 256)))

    ws, d, m = 4, 16, 2
    H, W, T = 2 * ws, 3 * ws, ws * ws
    qkv, out, g, b = z(2, H, W, 3 * m * d), z(2, H, W, m * d), z(2, H, W, m * d), z(T, T)
    wab = lambda qkv=qkv, b=b, out=out, g=g, **kw: ops.window_attention_backward(qkv, b, out, g, m, d, ws, 0.25, **kw)      # noqa: E731
    for kw in (dict(out=z(1, H, W, m * d)), dict(out=z(2, H, W, d)), dict(g=z(2, H, W - ws, m * d)), dict(g=z(2, H * W, m * d)),
               dict(b=z(T, T - 1)), dict(b=z(T * T)), dict(b=z(2 * T, 2 * T)), dict(qkv=z(2, H, W, 3 * m * d + 4)),
               dict(qkv=z(2, H, W + 1, 3 * m * d)), dict(qkv=z(2 * H, W, 3 * m * d)), dict(grad_qkv=z(2, H, W, m * d)),
               dict(out=out.double()), dict(g=g.half())):
        with bad:
            wab(**kw)
    with bad:
        ops.window_attention_backward(qkv, b, out, g, m, d, 5, 0.25)                      # a window that is not instantiated
