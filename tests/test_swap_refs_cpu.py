"""The float64 numpy reference of CoBEVT's agent-window attention (tests/attention_refs.py: swap_reference) against float64 torch
autograd of the reference's composition (reference_fp64 of tests/test_gpu_cobevt_grad.py), the properties of the fixtures that
tests/test_gpu_swap_conformance.py relies on, and the TEETH of its per-element bounds: seeded defects of the kind the kernels can
have, applied to the fp32-rounded reference, must break the bound of at least one element of the outputs they touch.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import attention_refs as R
from tests.test_gpu_cobevt_grad import reference_fp64

pytestmark = pytest.mark.grad         # float64 torch autograd is the witness here: the tests record graphs (on the CPU)

RTOL = 1e-12
HEADS, D = 2, R.SWAP_D
SCALE = R.f32_scale(D)
PAIRS = [(1, 1), (2, 1), (3, 2), (4, 4), (5, 3), (6, 1), (7, 4), (8, 5), (8, 8)]


def close(a, b):
    """1e-12 relative per element (an element whose reference is below 1 in magnitude is held to 1e-12 absolute)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= RTOL * np.maximum(np.abs(b), 1.0)).all())


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("mode", ["window", "grid"])
def test_split_and_merge_are_inverse_and_follow_the_token_order(mode):
    L, H, W, heads, d = 3, 8, 12, 2, 4
    x = np.arange(L * H * W * 3 * heads * d, dtype=np.float64).reshape(L, H, W, 3 * heads * d)
    t = R.swap_split(x, mode, 3, heads, d)
    assert t.shape == (3, 6 * heads, 16 * L, d)
    assert np.array_equal(R.swap_merge(t, mode, L, H, W, heads, d), x)
    # group (gx, gy) = (1, 2), head 1, token (l, w1, w2) = (2, 3, 1), the k third, channel 2: the kernel's pix() lambda
    gx, gy, l, w1, w2 = 1, 2, 2, 3, 1
    y, xx = (w1 * (H // 4) + gx, w2 * (W // 4) + gy) if mode == "grid" else (gx * 4 + w1, gy * 4 + w2)
    assert t[1, (gx * 3 + gy) * heads + 1, l * 16 + w1 * 4 + w2, 2] == x[l, y, xx, 1 * heads * d + 1 * d + 2]
    # and the torch form used by the autograd witness
    g = R.swap_groups(torch.from_numpy(x), mode, L, H, W)
    assert np.array_equal(g.numpy(), R.swap_groups(x, mode, L, H, W))
    assert np.array_equal(R.swap_ungroup(g, mode, L, H, W).numpy(), x)


@pytest.mark.parametrize("regime", ["spread", "large"])
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("mode", ["window", "grid"])
@pytest.mark.parametrize("L,n_valid", PAIRS)
def test_swap_reference_equals_float64_autograd(L, n_valid, mode, use_bias, regime):
    fx = R.swap_data(L, regime, seed=10 * L + n_valid, n_valid=n_valid, use_bias=use_bias)
    ref = R.swap_reference(fx["qkv"], fx["bias"], fx["grad_out"], n_valid, mode, HEADS, SCALE)
    tt = lambda a: None if a is None else torch.from_numpy(a)      # noqa: E731
    out, gq, gb = reference_fp64(tt(fx["qkv"]), tt(fx["bias"]), tt(fx["grad_out"]), n_valid, mode, HEADS, SCALE)
    assert close(ref["out"], out.numpy()) and close(ref["grad_qkv"], gq.numpy())
    if use_bias:
        assert close(ref["grad_bias"], gb.numpy())
    else:
        assert not ref["grad_bias"].any() and not ref["B_grad_bias"].any()
    for name in ("out", "grad_qkv", "grad_bias"):
        assert np.isfinite(ref[name]).all() and np.isfinite(ref["B_" + name]).all()
        assert (np.abs(ref[name]) <= ref["T_" + name] * (1 + 1e-12) + 1e-300).all()      # a sum is no larger than its absolute terms
    C = HEADS * D
    assert not ref["grad_qkv"][n_valid:, :, :, C:].any() and not ref["B_grad_qkv"][n_valid:, :, :, C:].any()      # masked dK, dV
    assert not ref["grad_bias"][:, :, 16 * n_valid:].any() and not ref["B_grad_bias"][:, :, 16 * n_valid:].any()
    # K and V of the masked agents are never read
    poisoned = fx["qkv"].copy()
    poisoned[n_valid:, :, :, C:] = np.nan
    again = R.swap_reference(poisoned, fx["bias"], fx["grad_out"], n_valid, mode, HEADS, SCALE)
    assert all(np.array_equal(again[n], ref[n]) for n in ("out", "grad_qkv", "grad_bias", "B_out", "B_grad_qkv", "B_grad_bias"))


def test_counts_follow_the_shapes():
    k = R.swap_k(5, 3, 32, groups=6, parts=4)
    assert k["p"] == 12 + 12 and k["out"] == k["p"] + 48 + 1 and k["dk"] - k["dq"] == 80 - 48 and k["dv"] == k["p"] + 81
    assert k["bias"] == k["dS"] + 1 + 3                          # the largest of 4 parts of 6 groups holds 2; 4 parts
    assert R.swap_k(5, 3, 32, 6, 1)["bias"] == k["dS"] + 5 and R.swap_k(5, 3, 32, 6, 6)["bias"] == k["dS"] + 5
    assert R.swap_policy_parts(8, 12, 2) == 6 and R.swap_policy_parts(128, 128, 8) == 128 and R.swap_policy_parts(4, 4, 2000) == 1


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("L,n_valid", [(L, n) for L in range(1, 9) for n in sorted({1, L, (L + 1) // 2})])
def test_fixture_properties(L, n_valid):
    T, Tk = 16 * L, 16 * n_valid
    for h in range(HEADS):
        pi = R.swap_perm(T, Tk, h)
        assert sorted(pi[:Tk]) == list(range(Tk)) and (pi != np.arange(T)).all() and pi.max() < Tk
        inside = np.arange(T) < Tk
        assert (pi[pi[inside]] != np.arange(T)[inside]).all()
        if n_valid > 1:
            assert len(set(pi[:16] // 16)) > 1                                            # one query tile selects keys of several agents
    assert not np.array_equal(R.swap_perm(T, Tk, 0), R.swap_perm(T, Tk, 1))
    assert float(np.exp(np.float32(R.SELECT))) < 2.0 ** -149 / 2
    for mode in ("window", "grid"):
        for regime in ("uniform", "selector"):
            fx = R.swap_data(L, regime, seed=1, n_valid=n_valid)
            for a in (fx["qkv"], fx["grad_out"]):
                assert np.array_equal(a, np.round(a)) and float(np.abs(a).max()) == 3
            assert not fx["qkv"].reshape(L, 8, 12, 3, HEADS, D)[:, :, :, 0].any()          # q == 0
            ex = R.swap_exact(fx, n_valid, mode, HEADS, regime)
            assert ex["units"] < R.EXACT_LIMIT
            if regime == "uniform" and n_valid & (n_valid - 1):
                continue                                                                  # 1 / Tk is no fp32 number: not asserted exactly
            ref = R.swap_reference(fx["qkv"], fx["bias"], fx["grad_out"], n_valid, mode, HEADS, SCALE)
            C = HEADS * D
            # the selector's reference is the gather up to float64's exp(-256) = 1e-111 (fp32: 0); the uniform one's is the mean
            assert float(np.abs(ref["out"] - ex["out"]).max()) < 1e-100
            assert float(np.abs(ref["grad_qkv"][..., C:2 * C] - ex["dk"]).max()) < 1e-100
            assert float(np.abs(ref["grad_qkv"][..., 2 * C:] - ex["dv"]).max()) < 1e-12
            assert float(np.abs(ex["out"]).max()) > 0 and float(np.abs(ex["dv"]).max()) > 0
            if regime == "selector":
                assert float(np.abs(ref["grad_qkv"][..., :C]).max()) < 1e-100 and float(np.abs(ref["grad_bias"]).max()) < 1e-100
                b = fx["bias"].astype(np.float64)
                assert not np.array_equal(b, b.transpose(0, 2, 1)) and not np.array_equal(b[0], b[1])
                assert ((b == 0).sum(-1) == 1).all() and set(np.unique(b)) == {R.SELECT, 0.0}
    fl = R.swap_data(L, "large", seed=10 * L + n_valid, n_valid=n_valid)
    q, k, _ = R.swap_split(fl["qkv"].astype(np.float64), "window", 3, HEADS, D)
    s = SCALE * np.einsum("bqd,bkd->bqk", q, k[:, :Tk])
    assert 60 <= float(s.max()) and float(s.min()) <= -60 and float(np.abs(s).max()) < 140      # expf needs the max subtraction


# ---------------------------------------------------------------------------------------------------------------- (c)
OUT = ("out", "grad_qkv", "grad_bias")
PARTS = 4          # of the 6 groups: 2 + 2 + 1 + 1


def ratios(mut, ref):
    return {n: R.max_ratio(np.asarray(mut[n], np.float64).astype(np.float32), ref[n], ref["B_" + n]) for n in OUT}


def plain(fx, n_valid, mode, D_without_inv=False, dk_without_scale=False):
    """The operator written out once more in float64 with two of the kernel's possible slips: D = sum_j e_j dP_j left unnormalised,
    and dK without `* scale`.  (Without a slip it is a second witness of swap_reference.)"""
    qkv = fx["qkv"].astype(np.float64)
    L, H, W, _ = qkv.shape
    T = 16 * L
    q, k, v = R.swap_split(qkv, mode, 3, HEADS, D)
    dO = R.swap_split(fx["grad_out"].astype(np.float64), mode, 1, HEADS, D)[0]
    s = SCALE * np.einsum("bqd,bkd->bqk", q, k)
    if fx["bias"] is not None:
        s = s + np.tile(fx["bias"].astype(np.float64), (s.shape[0] // HEADS, 1, 1))
    s[:, :, 16 * n_valid:] = -np.inf
    e = np.exp(s - s.max(-1, keepdims=True))
    den = e.sum(-1, keepdims=True)
    P = e / den
    dP = np.einsum("bqd,bkd->bqk", dO, v)
    Drow = (P * dP).sum(-1, keepdims=True) * (den if D_without_inv else 1.0)
    dS = P * (dP - Drow)
    dq = SCALE * np.einsum("bqk,bkd->bqd", dS, k)
    dk = (1.0 if dk_without_scale else SCALE) * np.einsum("bqk,bqd->bkd", dS, q)
    dv = np.einsum("bqk,bqd->bkd", P, dO)
    put = lambda t: R.swap_merge(t, mode, L, H, W, HEADS, D)      # noqa: E731
    gb = dS.reshape(-1, HEADS, T, T).sum(0) if fx["bias"] is not None else np.zeros((HEADS, T, T))
    return dict(out=put(np.einsum("bqk,bkd->bqd", P, v)[None]), grad_qkv=put(np.stack([dq, dk, dv])), grad_bias=gb)


@functools.lru_cache(maxsize=None)
def case(L, n_valid, mode, regime, use_bias):
    fx = R.swap_data(L, regime, seed=10 * L + n_valid, n_valid=n_valid, use_bias=use_bias)
    return fx, R.swap_reference(fx["qkv"], fx["bias"], fx["grad_out"], n_valid, mode, HEADS, SCALE, parts=PARTS)


def mutants(fx, ref, L, n_valid, mode):
    """name -> (the defective result, the outputs in which it must show)."""
    run = lambda bias=fx["bias"], n=n_valid, md=mode: R.swap_reference(fx["qkv"], bias, fx["grad_out"], n, md, HEADS, SCALE, parts=PARTS)      # noqa: E731
    out = {}
    if n_valid > 1:
        out["last_valid_key_tile_dropped"] = (run(n=n_valid - 1), OUT if fx["bias"] is not None else OUT[:2])
    out["window_order_in_grid_mode" if mode == "grid" else "grid_order_in_window_mode"] = (
        run(md="window" if mode == "grid" else "grid"), OUT if fx["bias"] is not None else OUT[:2])
    out["D_without_inv"] = (plain(fx, n_valid, mode, D_without_inv=True), ("grad_qkv",) + (("grad_bias",) if fx["bias"] is not None else ()))
    out["dK_without_scale"] = (plain(fx, n_valid, mode, dk_without_scale=True), ("grad_qkv",))
    if fx["bias"] is not None:
        out["bias_transposed"] = (run(bias=np.ascontiguousarray(fx["bias"].transpose(0, 2, 1))), OUT)
        out["bias_of_head_0_for_head_1"] = (run(bias=np.ascontiguousarray(fx["bias"][[0, 0]])), OUT)
        short = dict(ref)
        short["grad_bias"] = ref["grad_bias"] - ref["dS"][-1]          # the last of the PARTS parts holds the last group alone
        out["grad_bias_missing_its_last_part"] = (short, ("grad_bias",))
    return out


@pytest.mark.parametrize("regime", ["spread", "large"])
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("mode", ["window", "grid"])
@pytest.mark.parametrize("L,n_valid", [(1, 1), (2, 2), (3, 2), (5, 3), (8, 1), (8, 8)])
def test_swap_bounds_have_teeth(L, n_valid, mode, use_bias, regime):
    fx, ref = case(L, n_valid, mode, regime, use_bias)
    clean = ratios(ref, ref)
    assert all(v <= 1.0 for v in clean.values()), clean          # rounding the reference to fp32 stays inside
    second = ratios(plain(fx, n_valid, mode), ref)
    assert all(v <= 1.0 for v in second.values()), second
    for name, (mut, must) in mutants(fx, ref, L, n_valid, mode).items():
        r = ratios(mut, ref)
        print(L, n_valid, mode, regime, name, {k: round(v, 2) for k, v in r.items()})
        assert all(r[n] > 1.0 for n in must), (name, r)
