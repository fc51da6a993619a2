"""The float64 numpy references of tests/attention_refs.py against float64 torch autograd of the reference compositions
(mswin.py:64-78 for K6b, hmsa.py:131-146 for K6, as written out in tests/test_gpu_train.py), the properties of the fixtures that
tests/test_gpu_attention_conformance.py relies on, and the TEETH of its per-element bounds: seeded defects of the kind a kernel
can have, applied to the fp32-rounded reference, must break the bound of at least one element.  No GPU: this must pass before a
kernel is compared with any of these references."""
import numpy as np
import pytest
import torch

from tests import attention_refs as R

pytestmark = pytest.mark.grad         # float64 torch autograd is the witness here: the tests record graphs (on the CPU)

RTOL = 1e-12


def close(a, b):
    """1e-12 relative per element (an element whose reference is below 1 in magnitude is held to 1e-12 absolute)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= RTOL * np.maximum(np.abs(b), 1.0)).all())


# ---------------------------------------------------------------------------------------------------------------- (a)
def window_autograd(qkv, bias, gout, m, d, ws, scale):
    L, H, W, _ = qkv.shape
    T, C = ws * ws, m * d
    q64 = torch.from_numpy(np.asarray(qkv, np.float64)).requires_grad_(True)
    b64 = None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)).requires_grad_(True)
    nh, nw = H // ws, W // ws
    t = q64.view(L, nh, ws, nw, ws, 3, m, d).permute(5, 0, 6, 1, 3, 2, 4, 7).reshape(3, L * m * nh * nw, T, d)
    dots = torch.matmul(t[0], t[1].transpose(1, 2)) * scale
    if b64 is not None:
        dots = dots + b64[None]
    ref = torch.matmul(dots.softmax(-1), t[2]).view(L, m, nh, nw, ws, ws, d).permute(0, 2, 4, 3, 5, 1, 6).reshape(L, H, W, C)
    (ref * torch.from_numpy(np.asarray(gout, np.float64))).sum().backward()
    return ref.detach().numpy(), q64.grad.numpy(), None if b64 is None else b64.grad.numpy()


@pytest.mark.parametrize("regime", ["spread", "large"])
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ws,d", R.WINDOW_SHAPES)
def test_window_reference_equals_float64_autograd(ws, d, use_bias, regime):
    m = 2
    fx = R.window_data(ws, d, regime, seed=ws + d)
    bias = fx["bias"] if use_bias else None
    scale = R.f32_scale(d)
    ref = R.window_reference(fx["qkv"], bias, fx["grad_out"], m, d, ws, scale)
    out, gq, gb = window_autograd(fx["qkv"], bias, fx["grad_out"], m, d, ws, scale)
    assert close(ref["out"], out) and close(ref["grad_qkv"], gq)
    if use_bias:
        assert close(ref["grad_bias"], gb)
    for name in ("out", "grad_qkv", "grad_bias"):
        assert np.isfinite(ref[name]).all() and np.isfinite(ref["B_" + name]).all()
        assert (np.abs(ref[name]) <= ref["T_" + name] * (1 + 1e-12) + 1e-300).all()      # a sum is no larger than its absolute terms
    assert ref["grad_qkv"].shape == fx["qkv"].shape


def agent_autograd(q, k, v, gout, heads, scale, mask, R_):
    P, L, C = q.shape
    dh = C // heads
    q64, k64, v64 = (torch.from_numpy(np.asarray(t, np.float64)).reshape(P, L, heads, dh).requires_grad_(True) for t in (q, k, v))
    att = torch.einsum("pihd,pjhd->phij", q64, k64) * scale
    if mask is not None:
        att = att.masked_fill(torch.from_numpy(np.asarray(mask) == 0)[None, None, None, :], float("-inf"))
    ref = torch.einsum("phij,pjhd->pihd", att.softmax(-1), v64)[:, :R_]
    (ref * torch.from_numpy(np.asarray(gout, np.float64)).reshape(P, R_, heads, dh)).sum().backward()
    return [t.reshape(P, -1, C).numpy() for t in (ref.detach(), q64.grad, k64.grad, v64.grad)]


AGENT_CASES = [(1, 1, 1, None), (1, 3, 1, None), (4, 2, 2, "first"), (8, 5, 3, "top"), (16, 8, 8, "single"), (16, 8, 4, None),
               (4, 7, 4, "first"), (8, 6, 1, "top"), (1, 8, 8, "top")]


@pytest.mark.parametrize("regime", ["spread", "large"])
@pytest.mark.parametrize("heads,L,R_,mask", AGENT_CASES)
def test_agent_reference_equals_float64_autograd(heads, L, R_, mask, regime):
    fx = R.agent_data(heads, L, 5, regime, seed=heads * 10 + L)
    scale = R.f32_scale(R.C_AGENT // heads)
    km = None if mask is None else R.agent_masks(L, fx["q"], fx["k"], heads, scale)[mask]
    go = fx["grad_out"][:, :R_]
    ref = R.agent_reference(fx["q"], fx["k"], fx["v"], go, heads, scale, km, R_)
    want = agent_autograd(fx["q"], fx["k"], fx["v"], go, heads, scale, km, R_)
    for name, w in zip(("out", "grad_q", "grad_k", "grad_v"), want):
        assert ref[name].shape == w.shape and close(ref[name], w), name
        assert np.isfinite(ref["B_" + name]).all()
        assert (np.abs(ref[name]) <= ref["T_" + name] * (1 + 1e-12) + 1e-300).all()
    if R_ < L:
        assert not ref["grad_q"][:, R_:].any() and not ref["B_grad_q"][:, R_:].any()
    if km is not None:
        assert not ref["grad_k"][:, km == 0].any() and not ref["grad_v"][:, km == 0].any()


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("ws,d", R.WINDOW_SHAPES)
def test_window_fixture_properties(ws, d):
    T = ws * ws
    pi = R.window_perm(T)
    assert sorted(pi) == list(range(T)) and (pi != np.arange(T)).all() and (pi[pi] != np.arange(T)).all()
    for regime in ("uniform", "selector"):
        fx = R.window_data(ws, d, regime, seed=1)
        assert R.window_exact_units(fx, T, d, regime) < R.EXACT_LIMIT
        for a in (fx["qkv"], fx["grad_out"]):
            assert np.array_equal(a, np.round(a))
        assert not fx["qkv"].reshape(2, 2 * ws, 3 * ws, 3, 2, d)[:, :, :, 0].any()          # q == 0
        assert float(np.abs(fx["qkv"]).max()) == 3 and float(np.abs(fx["grad_out"]).max()) == 3
    b = fx["bias"].astype(np.float64)
    sel = b[np.arange(T), pi]
    assert (sel == 0).all() and not np.array_equal(b, b.T)
    rest = np.where(np.arange(T)[None] == pi[:, None], -np.inf, b)
    assert float((sel - rest.max(1)).min()) >= 200                                        # the selector margin (scores are 0: q = 0)
    assert float(np.exp(np.float32(R.SELECT))) < 2.0 ** -149 / 2                         # below half the smallest fp32 denormal
    # the selector's reference is the gather up to float64's exp(-256) = 1e-111 (fp32: 0), the uniform one's IS the window mean
    ref = R.window_reference(fx["qkv"], fx["bias"], fx["grad_out"], 2, d, ws, R.f32_scale(d))
    v = R.window_split(fx["qkv"].astype(np.float64), ws, 3, 2, d)[2]
    g = R.window_split(fx["grad_out"].astype(np.float64), ws, 1, 2, d)[0]
    dq, dk, dv = R.window_split(ref["grad_qkv"], ws, 3, 2, d)
    assert float(np.abs(R.window_split(ref["out"], ws, 1, 2, d)[0] - v[:, pi]).max()) < 1e-100
    assert float(np.abs(dv[:, pi] - g).max()) < 1e-100
    assert max(float(np.abs(t).max()) for t in (ref["grad_bias"], dq, dk)) < 1e-100
    fu = R.window_data(ws, d, "uniform", seed=1)
    ru = R.window_reference(fu["qkv"], None, None, 2, d, ws, R.f32_scale(d))
    vu = R.window_split(fu["qkv"].astype(np.float64), ws, 3, 2, d)[2]
    assert np.array_equal(R.window_split(ru["out"], ws, 1, 2, d)[0], np.broadcast_to(vu.sum(1, keepdims=True) / T, vu.shape))
    # the large-logit fixture reaches the range where expf needs the max subtraction
    fl = R.window_data(ws, d, "large", seed=ws + d)
    q, k, _ = R.window_split(fl["qkv"].astype(np.float64), ws, 3, 2, d)
    s = R.f32_scale(d) * np.einsum("bqd,bkd->bqk", q, k) + fl["bias"][None]
    assert 70 <= float(s.max()) and float(s.min()) <= -70 and float(np.abs(s).max()) < 140


def test_agent_fixture_properties():
    for heads in R.AGENT_HEADS:
        for L in range(2, R.AGENT_MAX_L + 1):
            fx = R.agent_data(heads, L, 5, "spread", seed=heads * 10 + L)
            masks = R.agent_masks(L, fx["q"], fx["k"], heads, R.f32_scale(R.C_AGENT // heads))
            assert masks["first"][0] == 0 and masks["first"].sum() == L - 1
            assert masks["top"].sum() == L - 1 and masks["single"].sum() == 1 and masks["single"][L // 2] == 1
            fi = R.agent_data(heads, L, 5, "ints", seed=3)
            assert all(np.array_equal(fi[n], np.round(fi[n])) and np.abs(fi[n]).max() <= 3 for n in fi)
            assert L * 3 * (R.C_AGENT // heads) * 3 < R.EXACT_LIMIT          # dv = sum_i dO_i and dp = dO . v: integers far below 2^24
            fl = R.agent_data(heads, L, 5, "large", seed=heads * 10 + L)
            s = R.f32_scale(R.C_AGENT // heads) * np.einsum("pihd,pjhd->phij", *(fl[n].astype(np.float64).reshape(5, L, heads, -1)
                                                                                 for n in ("q", "k")))
            assert 40 <= float(np.abs(s).max()) < 200


# ---------------------------------------------------------------------------------------------------------------- (c)
def ratios(mut, ref, names):
    """Largest err / bound of the fp32-rounded `mut` against the reference, per output."""
    return {n: R.max_ratio(np.asarray(mut[n], np.float64).astype(np.float32), ref[n], ref["B_" + n]) for n in names}


W_OUT = ("out", "grad_qkv", "grad_bias")
A_OUT = ("out", "grad_q", "grad_k", "grad_v")
ANY = ()          # the subtlest defect (a relative score error of 2^-12): at least one output must break, whichever


def broken(r, must):
    return all(r[n] > 1.0 for n in must) if must else max(r.values()) > 1.0


def window_case(ws, d, regime):
    fx = R.window_data(ws, d, regime, seed=ws + d)
    return fx, R.window_reference(fx["qkv"], fx["bias"], fx["grad_out"], 2, d, ws, R.f32_scale(d))


def window_mutants(fx, ref, ws, d):
    """name -> (the defective result, the outputs in which it must show)."""
    m, sc = 2, R.f32_scale(d)
    L, H, W, _ = fx["qkv"].shape
    run = lambda qkv=fx["qkv"], bias=fx["bias"], scale=sc: R.window_reference(qkv, bias, fx["grad_out"], m, d, ws, scale)      # noqa: E731
    six = lambda a: a.copy().reshape(L, H, W, 3, m, d)      # noqa: E731
    out = {}
    x = six(fx["qkv"])
    x[1, ws, 2 * ws + 1, 2], x[1, ws + 1, 2 * ws, 2] = x[1, ws + 1, 2 * ws, 2].copy(), x[1, ws, 2 * ws + 1, 2].copy()
    out["v_rows_swapped"] = (run(qkv=x.reshape(fx["qkv"].shape)), W_OUT)
    out["bias_transposed"] = (run(bias=np.ascontiguousarray(fx["bias"].T)), W_OUT)
    out["bias_dropped"] = (dict(run(bias=None), grad_bias=ref["grad_bias"]), ("out", "grad_qkv"))
    out["scale_off_by_2^-12"] = (run(scale=sc * (1 + 2.0 ** -12)), ANY)
    x = six(fx["qkv"])
    x[:, :, :, 1] = np.roll(x[:, :, :, 1], -1, axis=3)
    out["head_reads_next_heads_k"] = (run(qkv=x.reshape(fx["qkv"].shape)), ("out",))
    short = dict(ref)
    short["grad_bias"] = ref["grad_bias"] - ref["dS"][-1]
    out["one_window_missing_from_grad_bias"] = (short, ("grad_bias",))
    return out


# (16, 64) is a quarter of a minute of float64 einsums per regime here: it runs the spread regime only
@pytest.mark.parametrize("ws,d,regime", [(ws, d, r) for ws, d in R.WINDOW_SHAPES for r in ("spread", "large") if (ws, r) != (16, "large")])
def test_window_bounds_have_teeth(ws, d, regime):
    fx, ref = window_case(ws, d, regime)
    clean = ratios(ref, ref, W_OUT)
    assert all(v <= 1.0 for v in clean.values()), clean          # rounding the reference to fp32 stays inside
    for name, (mut, must) in window_mutants(fx, ref, ws, d).items():
        r = ratios(mut, ref, W_OUT)
        print(ws, d, regime, name, {k: round(v, 2) for k, v in r.items()})
        assert broken(r, must), (name, r)


def agent_case(heads, L, R_, regime, masked):
    fx = R.agent_data(heads, L, 5, regime, seed=heads * 10 + L)
    km = None
    if masked:
        km = np.ones(L, np.int32)
        km[-2:] = 0
    sc = R.f32_scale(R.C_AGENT // heads)
    return fx, km, sc, R.agent_reference(fx["q"], fx["k"], fx["v"], fx["grad_out"][:, :R_], heads, sc, km, R_)


def agent_mutants(fx, km, sc, ref, heads, L, R_):
    go = fx["grad_out"][:, :R_]
    run = lambda q=fx["q"], k=fx["k"], v=fx["v"], scale=sc, mask=km: R.agent_reference(q, k, v, go, heads, scale, mask, R_)      # noqa: E731
    out = {}
    v = fx["v"].copy()
    v[:, [0, 1]] = v[:, [1, 0]]
    out["v_rows_swapped"] = (run(v=v), ("out", "grad_q", "grad_k"))          # grad_v = P^T dO does not read v
    out["scale_off_by_2^-12"] = (run(scale=sc * (1 + 2.0 ** -12)), ANY)
    if heads > 1:
        k = np.roll(fx["k"].reshape(5, L, heads, -1), -1, axis=2).reshape(fx["k"].shape)
        out["head_reads_next_heads_k"] = (run(k=k), ("out",))
    if km is not None:
        m2 = km.copy()
        m2[-1] = 1
        out["last_masked_key_unmasked"] = (run(mask=m2), A_OUT)
    if R_ < L:
        # the rows from the wrong end: queries L - R_ .. L - 1 answer in place of 0 .. R_ - 1
        w = run(q=np.ascontiguousarray(np.roll(fx["q"], R_ - L, axis=1)))
        out["out_rows_from_the_wrong_end"] = (dict(w, grad_q=np.roll(w["grad_q"], L - R_, axis=1)), A_OUT)
    return out


@pytest.mark.parametrize("regime", ["spread", "large"])
@pytest.mark.parametrize("heads,L,R_,masked", [(1, 3, 1, False), (4, 2, 1, False), (8, 5, 3, True), (16, 8, 4, True), (4, 8, 8, True),
                                               (1, 6, 3, True), (16, 3, 2, False)])
def test_agent_bounds_have_teeth(heads, L, R_, masked, regime):
    fx, km, sc, ref = agent_case(heads, L, R_, regime, masked)
    clean = ratios(ref, ref, A_OUT)
    assert all(v <= 1.0 for v in clean.values()), clean
    for name, (mut, must) in agent_mutants(fx, km, sc, ref, heads, L, R_).items():
        r = ratios(mut, ref, A_OUT)
        print(heads, L, R_, regime, name, {k: round(v, 2) for k, v in r.items()})
        assert broken(r, must), (name, r)
