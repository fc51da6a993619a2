"""Float64 numpy references, per-element error bounds and hand-built fixtures of the attention conformance suites
(tests/test_gpu_attention_conformance.py): K6 (heal_amd/csrc/agent_attn.hip: k_agent_attn, k_agent_attn_bwd) and K6b
(heal_amd/csrc/window_attn.hip: k_window_attn, k_window_attn_bwd_q, k_window_attn_bwd_kv), and (tests/test_gpu_swap_conformance.py)
CoBEVT's agent-window attention (heal_amd/csrc/swap_attn.hip: k_agent_window_attn; swap_attn_bwd.hip: k_agent_window_attn_bwd,
k_sum_parts) -- numpy only and closed-form gradients, so that tests/test_attention_refs_cpu.py and tests/test_swap_refs_cpu.py can
prove every reference against float64 torch autograd on a machine without a GPU.

All of them compute, per problem b (K6b: one (agent, window, head); K6: one (pixel, head); CoBEVT: one (group, head)),
    s = scale Q K^T (+ bias)  [masked keys: -inf],   P = softmax_rows(s),   O = P V
    dP = dO V^T,  D_q = sum_j P_qj dP_qj (= dO_q . O_q),  dS = P o (dP - D),
    dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO,  grad_bias = sum_b dS_b.

PER-ELEMENT BOUND.  Every output comes with T, the sum of the absolute values of its terms (the same formula on |q|, |k|, |v|,
|dO|, |bias| with the probabilities kept and dP - D replaced by dP|.| + D|.|), and the tests assert, element by element,
    |got - ref| <= SAFETY * EPS * (k * T + E) + TINY.
EPS = 2^-24 is one fp32 rounding, k counts the roundings of a term on its way into the output (window_k / agent_k derive it from
the kernel's operation sequence; none was tuned on a kernel's output), and E is the score error carried through the softmax, which
is no multiple of T: a score s_qj = scale sum q k + bias is formed with c_s roundings and subtracted from the row maximum with
one more, so its ABSOLUTE error is (c_s + 1) EPS A_qj with A = scale sum |q||k| + |bias|, however small the score itself came out.
To first order expf turns that into a relative error of e_qj; the maximum is the same fp32 number in the numerator and in the
denominator, so its own error cancels and only the rounding of the subtraction stays, |s_qj - max| EPS <= (A_qj + Amax_q) EPS
(the first half is the `+ 1` above).  The normalised probability therefore has the relative error, in EPS,
    pi_qj = Cm_qj + k_p,    Cm_qj = (c_s + 1) A_qj + sum_i P_qi (c_s + 1) A_qi + 2 Amax_q
(numerator: (c_s + 1) A_qj + Amax_q; denominator: the P-weighted mean of the same), where k_p collects the roundings that are
relative to the probability itself (expf twice, the sum, the division).  Cm enters O, dP - D, D, dS, dQ, dK, dV and grad_bias
exactly as P does, which gives every E below as `the formula of T with P replaced by P Cm` (plus the error of D inside dS).

Conventions (those of tests/backward_refs.py): `expf` is taken as 2 ulp = 4 EPS; the library is built with -ffp-contract=off,
so a product followed by an add is two roundings; an MFMA accumulation over n reduction steps is a chain of n sequential adds
(a term passes through at most n of them, after the 1 rounding of its product).  SAFETY = 2 is the one safety factor on the
first-order bound: it covers the second-order terms (at the large-logit fixtures Cm EPS reaches 1e-3) and nothing else.

EXACT.  Fixtures that need nothing from expf beyond expf(0) == 1 and expf(x) == 0 for x <= -200 (uniform softmax over a
power-of-two window, one-hot "selector" softmax through a -256 bias or through the key mask) hold integers such that every term and
partial sum is a multiple of one unit and below 2^24 units: fp32 computes them without rounding, in any order."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
TINY = 1e-30
SAFETY = 2.0
EXACT_LIMIT = 2.0 ** 24
SELECT = -256.0                # bias of a de-selected key: expf(-256 - 0) == 0 in fp32 (it underflows below -104)
LARGE_STD = 20.0 ** 0.5        # q and k of the K6b large-logit fixtures (scores: standard deviation 20)
LARGE_STD_AGENT = 30.0 ** 0.5  # K6 has few scores per case (down to 20): standard deviation 30 puts the extremes near +-80

WINDOW_SHAPES = [(4, 16), (8, 32), (16, 64), (4, 32), (8, 16), (8, 64), (4, 64)]      # HEAL_WA / HEAL_WAB: (window, dim_head)
AGENT_HEADS = (1, 4, 8, 16)
AGENT_MAX_L = 8
C_AGENT = 256


def max_ratio(got, ref, bound):
    """Largest |got - ref| / (bound + TINY) over the elements (NaN or inf in `got` counts as inf): <= 1 means the bound holds."""
    got = np.asarray(got, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - np.asarray(ref, np.float64))
    return float((err / (np.asarray(bound, np.float64) + TINY)).max())


def f32_scale(dim_head):
    """dim_head ** -0.5 as the fp32 number the kernels receive (exact for 16 and 64; rounded for 8, 32, 256)."""
    return float(F32(float(dim_head) ** -0.5))


# =====================================================================================================================
# the shared core: B independent attention problems
# =====================================================================================================================
def _core(Q, K, V, dO, bias, valid, scale, c):
    """Q [B,Tq,d], K, V [B,Tk,d], dO [B,Tq,d] or None, bias [Tq,Tk] (shared by the problems) or [B,Tq,Tk] (one per problem: the
    per-head bias of swap_reference) or None, valid [Tk] bool or None (False: key masked to -inf), all float64.  c: the rounding counts of window_k / agent_k.  Returns value / T / E of every output, per problem (the callers
    put them back into the tensors' layouts); E and the k * T products are in units of EPS."""
    aQ, aK, aV = np.abs(Q), np.abs(K), np.abs(V)
    s = scale * np.einsum("bqd,bkd->bqk", Q, K)
    A = scale * np.einsum("bqd,bkd->bqk", aQ, aK)
    if bias is not None:
        bb = bias[None] if bias.ndim == 2 else bias
        s = s + bb
        A = A + np.abs(bb)
    if valid is not None:
        s = np.where(valid[None, None, :], s, -np.inf)
        A = np.where(valid[None, None, :], A, 0.0)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    P = e / e.sum(-1, keepdims=True)
    a = (c["s"] + 1) * A
    Cm = a + (P * a).sum(-1, keepdims=True) + 2.0 * A.max(-1, keepdims=True)
    PC = P * Cm
    r = dict(P=P, A=A, Cm=Cm)
    r["out"] = np.einsum("bqk,bkd->bqd", P, V)
    r["T_out"] = np.einsum("bqk,bkd->bqd", P, aV)
    r["E_out"] = np.einsum("bqk,bkd->bqd", PC, aV)
    if dO is None:
        return r
    aO = np.abs(dO)
    dP = np.einsum("bqd,bkd->bqk", dO, V)
    dPa = np.einsum("bqd,bkd->bqk", aO, aV)
    D = (P * dP).sum(-1, keepdims=True)
    Da = (P * dPa).sum(-1, keepdims=True)
    if c["D_from_out"]:        # K6b: D = dO . O with the forward's own output: O carries k_out T_out + E_out
        ED = (aO * r["E_out"]).sum(-1, keepdims=True)
    else:                      # K6: D = sum_j P_j dP_j
        ED = (PC * dPa).sum(-1, keepdims=True)
    dS = P * (dP - D)
    dSa = P * (dPa + Da)
    EdS = Cm * dSa + P * ED
    r.update(dS=dS, dSa=dSa, EdS=EdS)
    r["dq"] = scale * np.einsum("bqk,bkd->bqd", dS, K)
    r["T_dq"] = scale * np.einsum("bqk,bkd->bqd", dSa, aK)
    r["E_dq"] = scale * np.einsum("bqk,bkd->bqd", EdS, aK)
    r["dk"] = scale * np.einsum("bqk,bqd->bkd", dS, Q)
    r["T_dk"] = scale * np.einsum("bqk,bqd->bkd", dSa, aQ)
    r["E_dk"] = scale * np.einsum("bqk,bqd->bkd", EdS, aQ)
    r["dv"] = np.einsum("bqk,bqd->bkd", P, dO)
    r["T_dv"] = np.einsum("bqk,bqd->bkd", P, aO)
    r["E_dv"] = np.einsum("bqk,bqd->bkd", PC, aO)
    return r


def _bound(k, T, E):
    return SAFETY * EPS * (k * T + E)


# =====================================================================================================================
# K6b: heal_window_attention / heal_window_attention_backward
# =====================================================================================================================
def window_k(ws, d, n_problems=1):
    """Roundings per term of k_window_attn, k_window_attn_bwd_q and k_window_attn_bwd_kv in EPS; T = ws * ws tokens, d = dim_head,
    n_problems = agents * windows * heads (the atomic adds into one grad_bias element).

    s      : S^T = K Q^T is d MFMA reduction steps: product 1 + d adds; `* scale` 1; `+ bias` 1 (without a bias the kernel adds
             0.0f: exact, the count stays an upper bound).                                              c_s  = d + 3
    e      = expf(s - mx): the subtraction 1 (-> (c_s + 1) A and Amax in Cm, module docstring), expf 4.
    sum    : a lane adds its T / 4 values in sequence, two xor-shuffle adds across the lane groups: T / 4 + 1 roundings of a
             positive sum, each term carrying its expf (4, first order: the P-weighted mean of the e errors).
    inv    = 1 / sum: 1.  The backward kernels form p = e * inv: 1 more; the forward multiplies the accumulated O by inv instead
             -- one product either way.        k_p = 4 + 4 + (T / 4 + 1) + 1 + 1 = T / 4 + 11, taken as       k_p  = T / 4 + 12
             (the +1: bwd_kv rebuilds p from the saved (mx, inv) as expf(sc * scale + bv - mx) * inv -- the same count -- but from
             a second evaluation of the score whose error need not be the one inside `sum`; first order, the same formula.)
    out    : O^T = V^T P^T is T reduction steps: product 1 + T adds.                                     k_out = k_p + T + 1
    D      = dO . O from the SAVED output, per lane group d / 16 iterations of `dsum += (g o + g o) + (g o + g o)`: product 1,
             two adds, the running add d / 16, two shuffle adds -> d / 16 + 5 of D|.| = sum |dO| T_out; the saved O is within
             k_out T_out + E_out (first order) of the exact one.                                          k_D  = k_out + d / 16 + 5
    dP     = V dO^T (bwd_q) / dO V^T (bwd_kv): d reduction steps.                                        c_dp = d + 1
    dS     = p * (dp - D): the subtraction 1 of dP|.| + D|.|, the product 1, p within pi, dp within c_dp dP|.|, D within
             k_D D|.| + E_D:  |err| <= P [(pi + 2)(dP|.| + D|.|) + c_dp dP|.| + k_D D|.| + E_D]
                                    <= (k_p + 2 + max(c_dp, k_D)) dS|.| + Cm dS|.| + P E_D.             k_dS = k_p + 2 + max(c_dp, k_D)
    dQ, dK : K^T dS^T / Q^T dS over T reduction steps (T + 1), then `* scale` 1.                         k_dq = k_dk = k_dS + T + 2
    dV     = dO^T P over T reduction steps.                                                              k_dv = k_p + T + 1
    bias   : grad_bias[q, j] += dS by atomicAdd from every (agent, window, head): n_problems terms in any order, each add
             rounding a partial sum of at most T_bias = sum |dS|.                                        k_bias = k_dS + n_problems - 1"""
    T = ws * ws
    k_p = T // 4 + 12
    k_out = k_p + T + 1
    k_D = k_out + d // 16 + 5
    c_dp = d + 1
    k_dS = k_p + 2 + max(c_dp, k_D)
    return dict(s=d + 3, p=k_p, out=k_out, D=k_D, dp=c_dp, dS=k_dS, dq=k_dS + T + 2, dk=k_dS + T + 2, dv=k_p + T + 1,
                bias=k_dS + n_problems - 1, D_from_out=True)


def window_split(x, ws, parts, m, d):
    """[L,H,W,parts*m*d] -> [parts, B, T, d] with B = (agent, head, window row, window column): the re-layout of mswin.py:64-70."""
    L, H, W, _ = x.shape
    nh, nw = H // ws, W // ws
    t = x.reshape(L, nh, ws, nw, ws, parts, m, d).transpose(5, 0, 6, 1, 3, 2, 4, 7)
    return t.reshape(parts, L * m * nh * nw, ws * ws, d)


def window_merge(t, L, H, W, ws, m, d):
    """The inverse of window_split: [parts, B, T, d] -> [L,H,W,parts*m*d]."""
    parts = t.shape[0]
    nh, nw = H // ws, W // ws
    x = t.reshape(parts, L, m, nh, nw, ws, ws, d).transpose(1, 3, 5, 4, 6, 0, 2, 7)
    return np.ascontiguousarray(x).reshape(L, H, W, parts * m * d)


def window_reference(qkv, bias, grad_out, m, d, ws, scale):
    """qkv [L,H,W,3*m*d] (q | k | v, each [m, d]), bias [T,T] or None, grad_out [L,H,W,m*d] or None; scale: the fp32 number passed
    to the kernel.  -> dict: out, T_out, B_out (the bound, SAFETY and EPS included) in the output's layout; with grad_out also
    grad_qkv / T_grad_qkv / B_grad_qkv in qkv's layout, grad_bias / T_grad_bias / B_grad_bias [T,T] (zeros without a bias: the
    kernel then writes none), and dS [B,T,T] per problem, B = (agent, head, window row, window column)."""
    qkv = np.asarray(qkv, np.float64)
    L, H, W, _ = qkv.shape
    q, k, v = window_split(qkv, ws, 3, m, d)
    dO = None if grad_out is None else window_split(np.asarray(grad_out, np.float64), ws, 1, m, d)[0]
    b = None if bias is None else np.asarray(bias, np.float64)
    kk = window_k(ws, d, q.shape[0])
    r = _core(q, k, v, dO, b, None, float(scale), kk)
    put = lambda t: window_merge(t, L, H, W, ws, m, d)      # noqa: E731
    res = dict(k=kk, P=r["P"])
    res["out"], res["T_out"] = put(r["out"][None]), put(r["T_out"][None])
    res["B_out"] = _bound(kk["out"], res["T_out"], put(r["E_out"][None]))
    if dO is None:
        return res
    res["grad_qkv"] = put(np.stack([r["dq"], r["dk"], r["dv"]]))
    res["T_grad_qkv"] = put(np.stack([r["T_dq"], r["T_dk"], r["T_dv"]]))
    res["B_grad_qkv"] = put(np.stack([_bound(kk[n], r["T_" + n], r["E_" + n]) for n in ("dq", "dk", "dv")]))
    res["dS"] = r["dS"]
    res["grad_bias"], res["T_grad_bias"] = r["dS"].sum(0), r["dSa"].sum(0)
    res["B_grad_bias"] = _bound(kk["bias"], res["T_grad_bias"], r["EdS"].sum(0))
    return res


def window_data(ws, d, regime, seed, L=2, m=2):
    """The K6b fixtures on a (2 ws) x (3 ws) map: window row and column indices both reach a non-zero value, H != W, L = 2 and
    m = 2 heads exercise l * H * W, h * D and MD.  -> dict(qkv, bias or None, grad_out), float32.
      spread    : qkv N(0, 0.8), bias N(0, 1) -- a softmax with many comparable weights.
      large     : q and k N(0, LARGE_STD): scale * sqrt(d) = 1, so the scores have a standard deviation of LARGE_STD^2 = 20 whatever
                  d is, and their extremes reach about +-80 in a 4 x 4 window and +-100 in a 16 x 16 one (beyond +-88 expf
                  overflows without the max subtraction); bias N(0, 1).
      uniform   : q = 0, no bias, integer k, v and grad_out: every probability is 1 / T exactly (T a power of two).
      selector  : q = 0, bias[i, pi(i)] = 0 and SELECT elsewhere for the permutation pi of window_perm: P[i, pi(i)] == 1 exactly."""
    g = np.random.default_rng(seed)
    H, W, T = 2 * ws, 3 * ws, ws * ws
    shape = (L, H, W, 3, m, d)
    if regime in ("spread", "large"):
        qkv = g.standard_normal(shape) * 0.8
        if regime == "large":
            qkv[:, :, :, :2] *= LARGE_STD / 0.8
        bias = g.standard_normal((T, T))
        gout = g.standard_normal((L, H, W, m * d))
    else:
        qkv = g.integers(-3, 4, shape).astype(np.float64)
        qkv[:, :, :, 0] = 0.0
        gout = g.integers(-3, 4, (L, H, W, m * d)).astype(np.float64)
        bias = None
        if regime == "selector":
            bias = np.full((T, T), SELECT)
            bias[np.arange(T), window_perm(T)] = 0.0
    f = lambda a: None if a is None else np.ascontiguousarray(a, F32)      # noqa: E731
    return dict(qkv=f(qkv.reshape(L, H, W, 3 * m * d)), bias=f(bias), grad_out=f(gout))


def window_perm(T):
    """A fixed permutation of the T tokens that is no involution (pi(pi(i)) != i: the selector bias is not symmetric, so a
    transposed bias read selects another key), has no fixed point and maps neighbours far apart: pi(i) = (5 i + 3) mod T."""
    return (5 * np.arange(T) + 3) % T


def window_exact_units(data, T, d, regime):
    """Largest sum of absolute terms behind the outputs that the exact K6b fixtures assert, in units of the fixture's grid.
    uniform (unit 1 / T; e = 1, sum = T, inv = 1 / T, a power of two): out = (sum_j v_j) * inv and dV = sum_q dO_q * (1 * inv): at most
        T max|v| (T max|dO|) units; dK = scale * sum_q q_q dS = 0 because q = 0.  dQ is NOT asserted: it is a real gradient there.
    selector (unit 1; e in {0, 1}, sum = inv = 1): out = v_pi(i); D = dO_i . v_pi(i) and dP_j = dO_i . v_j are integers of at most
        d max|v| max|dO|; dS = 1 * (dP - D) = 0 or 0 * (...) = 0, so dQ = dK = grad_bias = 0, and dV_pi(i) = dO_i."""
    vmax = float(np.abs(data["qkv"]).max())
    gmax = float(np.abs(data["grad_out"]).max())
    return T * max(vmax, gmax) if regime == "uniform" else 2.0 * d * vmax * gmax


# =====================================================================================================================
# K6: heal_agent_attention / heal_agent_attention_backward
# =====================================================================================================================
def agent_k(heads, L, out_rows):
    """Roundings per term of k_agent_attn and k_agent_attn_bwd in EPS.  A head is LPH = 64 / heads lanes of 4 channels each;
    lg = log2(LPH) butterfly steps; L keys, out_rows query rows.

    s      : d = qx kx + qy ky + qz kz + qw kw, left to right: product 1, adds 3; lg xor-shuffle adds; `* scale` 1.   c_s  = lg + 5
    e      = expf(s - mx): the subtraction 1 (-> (c_s + 1) A and Amax in Cm, module docstring), expf 4.
    den    : `den += e` over the L keys from 0: L - 1 roundings of a positive sum, each term carrying its expf 4.
    p      = e / den: 1.                                                     k_p = 4 + 4 + (L - 1) + 1                = L + 8
    out    : `acc += p * v`: product 1, L - 1 rounded adds.                                                           k_out = k_p + L
    dp     = dO . v_j: as the score without the scale.                                                                c_dp = lg + 4
    D      = `dsum += p * dp` over L keys: p within pi, dp within c_dp, product 1, L - 1 adds: (k_p + c_dp + L) D|.| + E_D with
             E_D = sum_j P_j Cm_j dP|.|_j.                                                                            k_D  = k_p + c_dp + L
    dS     = p * (dp - D) * scale: the subtraction 1, two products 2:
             |err| <= (k_p + 3 + max(c_dp, k_D)) dS|.| + Cm dS|.| + P E_D  (the scale factored out, as in T).         k_dS = k_p + 3 + k_D
    dq     = `dq += ds * k` over L keys: product 1, L - 1 adds.                                                       k_dq = k_dS + L
    dk     = `dk[j] += ds * q` over the out_rows query rows.                                                          k_dk = k_dS + out_rows
    dv     = `dv[j] += p * dO` over the out_rows query rows.                                                          k_dv = k_p + out_rows
    One unmasked key (L = 1 or all but one masked): s - mx = 0, e = den = p = 1 exactly, every masked p = expf(-inf) = 0: out = v_j,
    dp - D = 0, dq = dk = 0 and dv_j = sum_i dO_i with no rounding on integer dO -- asserted exactly, not through these counts."""
    lg = {1: 6, 4: 4, 8: 3, 16: 2}[heads]
    k_p = L + 8
    c_dp = lg + 4
    k_D = k_p + c_dp + L
    k_dS = k_p + 3 + k_D
    return dict(s=lg + 5, p=k_p, out=k_p + L, D=k_D, dp=c_dp, dS=k_dS, dq=k_dS + L, dk=k_dS + out_rows, dv=k_p + out_rows,
                D_from_out=False)


def agent_split(x, heads):
    """[P, R, 256] -> [P * heads, R, 256 / heads]."""
    P, R, C = x.shape
    return x.reshape(P, R, heads, C // heads).transpose(0, 2, 1, 3).reshape(P * heads, R, C // heads)


def agent_merge(t, P, heads):
    """[P * heads, R, dh] -> [P, R, 256]."""
    _, R, dh = t.shape
    return np.ascontiguousarray(t.reshape(P, heads, R, dh).transpose(0, 2, 1, 3)).reshape(P, R, heads * dh)


def agent_reference(q, k, v, grad_out, heads, scale, key_mask=None, out_rows=None):
    """q, k, v [P, L, 256] (pixel-major), grad_out [P, out_rows, 256] or None, key_mask [L] (0: the key is masked) or None;
    scale: the fp32 number passed to the kernel.  Only the first out_rows query rows are produced; grad_q of the others is 0
    with a bound of 0.  -> dict: out / T_out / B_out [P, out_rows, 256]; grad_q, grad_k, grad_v with T_* and B_* [P, L, 256]."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    P, L, _ = q.shape
    R = L if out_rows is None else int(out_rows)
    valid = None if key_mask is None else (np.asarray(key_mask) != 0)
    dO = None if grad_out is None else agent_split(np.asarray(grad_out, np.float64), heads)
    kk = agent_k(heads, L, R)
    r = _core(agent_split(q[:, :R], heads), agent_split(k, heads), agent_split(v, heads), dO, None, valid, float(scale), kk)
    put = lambda t: agent_merge(t, P, heads)      # noqa: E731
    res = dict(k=kk, P=r["P"])
    res["out"], res["T_out"] = put(r["out"]), put(r["T_out"])
    res["B_out"] = _bound(kk["out"], res["T_out"], put(r["E_out"]))
    if dO is None:
        return res
    pad = lambda t: np.concatenate([t, np.zeros((P, L - R, t.shape[2]))], 1)      # noqa: E731
    for n, name, full in (("dq", "grad_q", pad), ("dk", "grad_k", lambda t: t), ("dv", "grad_v", lambda t: t)):
        res[name], res["T_" + name] = full(put(r[n])), full(put(r["T_" + n]))
        res["B_" + name] = _bound(kk[n], res["T_" + name], full(put(r["E_" + n])))
    return res


def agent_data(heads, L, n_pix, regime, seed):
    """q, k, v [n_pix, L, 256] and grad_out [n_pix, L, 256] (the tests slice its first out_rows rows), float32.
      spread : N(0, 1.5), as tests/test_gpu_train.py.
      large  : q and k N(0, LARGE_STD_AGENT): scores with a standard deviation of 30 for every head count, extremes near +-80.
      ints   : integers in [-3, 3] (the exact cases: one unmasked key)."""
    g = np.random.default_rng(seed)
    shape = (n_pix, L, C_AGENT)
    if regime == "ints":
        q, k, v, go = (g.integers(-3, 4, shape).astype(np.float64) for _ in range(4))
    else:
        std = LARGE_STD_AGENT if regime == "large" else 1.5
        q, k = g.standard_normal(shape) * std, g.standard_normal(shape) * std
        v, go = g.standard_normal(shape) * 1.5, g.standard_normal(shape)
    f = lambda a: np.ascontiguousarray(a, F32)      # noqa: E731
    return dict(q=f(q), k=f(k), v=f(v), grad_out=f(go))


def agent_top_key(q, k, heads, scale):
    """The key with the largest mean probability over pixels, heads and query rows: masking it moves the most weight."""
    s = float(scale) * np.einsum("bqd,bkd->bqk", agent_split(np.asarray(q, np.float64), heads), agent_split(np.asarray(k, np.float64), heads))
    e = np.exp(s - s.max(-1, keepdims=True))
    return int((e / e.sum(-1, keepdims=True)).mean((0, 1)).argmax())


def agent_masks(L, q, k, heads, scale):
    """The key masks of the suite for L >= 2 -> {name: int32 [L]}: key 0 masked; the highest-scoring key masked; all but one key
    masked (the survivor is key L // 2, neither first nor -- for L > 2 -- last)."""
    masks = {}
    m = np.ones(L, np.int32); m[0] = 0
    masks["first"] = m
    m = np.ones(L, np.int32); m[agent_top_key(q, k, heads, scale)] = 0
    masks["top"] = m
    m = np.zeros(L, np.int32); m[L // 2] = 1
    masks["single"] = m
    return masks


def to_layout(x, agent_major):
    """Pixel-major [P, R, C] -> the kernel's layout ([R, P, C] when agent_major)."""
    return np.ascontiguousarray(np.transpose(x, (1, 0, 2))) if agent_major else np.ascontiguousarray(x)


def from_layout(x, agent_major):
    return np.transpose(x, (1, 0, 2)) if agent_major else x


# =====================================================================================================================
# CoBEVT: heal_agent_window_attention / heal_agent_window_attention_backward (swap_attn.hip, swap_attn_bwd.hip)
# =====================================================================================================================
SWAP_WS, SWAP_D = 4, 32
SWAP_MAX_L = 8
SWAP_PARTS_BLOCKS = 1024       # SWAPB_BLOCKS of swap_attn_bwd.hip: the parts policy aims at this many blocks


def _permute(t, axes):
    return t.permute(*axes) if hasattr(t, "permute") else t.transpose(axes)


def swap_groups(t, mode, L, H, W):
    """[L, H, W, c] -> [groups, T = 16 L, c] in the reference's (l w1 w2) token order; numpy arrays and torch tensors alike (the
    float64 autograd witnesses regroup tensors that record a graph).  window: 'b m d (x w1) (y w2) -> (b x y) (m w1 w2) d', a group
    is one 4 x 4 tile of every agent; grid: 'b m d (w1 x) (w2 y) -> ..', a group is a dilated 4 x 4 grid (swap_fusion_modules.py)."""
    c = t.shape[-1]
    X, Y = H // SWAP_WS, W // SWAP_WS
    if mode == "window":
        return _permute(t.reshape(L, X, SWAP_WS, Y, SWAP_WS, c), (1, 3, 0, 2, 4, 5)).reshape(X * Y, L * 16, c)
    return _permute(t.reshape(L, SWAP_WS, X, SWAP_WS, Y, c), (2, 4, 0, 1, 3, 5)).reshape(X * Y, L * 16, c)


def swap_ungroup(o, mode, L, H, W):
    """The inverse of swap_groups: [groups, T, c] -> [L, H, W, c]."""
    c = o.shape[-1]
    X, Y = H // SWAP_WS, W // SWAP_WS
    if mode == "window":
        return _permute(o.reshape(X, Y, L, SWAP_WS, SWAP_WS, c), (2, 0, 3, 1, 4, 5)).reshape(L, H, W, c)
    return _permute(o.reshape(X, Y, L, SWAP_WS, SWAP_WS, c), (2, 3, 0, 4, 1, 5)).reshape(L, H, W, c)


def swap_split(x, mode, parts, heads, d):
    """[L,H,W,parts*heads*d] -> [parts, B, T, d] with B = (group, head) and T = 16 L tokens in (l w1 w2) order."""
    L, H, W, _ = x.shape
    g = swap_groups(np.asarray(x), mode, L, H, W)                               # [G, T, parts * heads * d]
    G, T = g.shape[:2]
    return g.reshape(G, T, parts, heads, d).transpose(2, 0, 3, 1, 4).reshape(parts, G * heads, T, d)


def swap_merge(t, mode, L, H, W, heads, d):
    """The inverse of swap_split: [parts, B, T, d] -> [L,H,W,parts*heads*d]."""
    parts, T = t.shape[0], t.shape[2]
    G = t.shape[1] // heads
    g = np.ascontiguousarray(t.reshape(parts, G, heads, T, d).transpose(1, 3, 0, 2, 4)).reshape(G, T, parts * heads * d)
    return np.ascontiguousarray(swap_ungroup(g, mode, L, H, W))


def swap_policy_parts(H, W, heads):
    """heal_agent_window_attention_backward_parts restated: min(groups, max(1, 1024 / heads))."""
    G = (H // SWAP_WS) * (W // SWAP_WS)
    return min(G, max(1, SWAP_PARTS_BLOCKS // heads))


def swap_k(L, n_valid, d, groups=1, parts=1):
    """Roundings per term of k_agent_window_attn<L, d> and k_agent_window_attn_bwd<L, d> (+ k_sum_parts) in EPS.  T = 16 L query tokens,
    Tk = 16 n_valid unmasked keys (a masked agent is a key tile that is neither staged nor multiplied: it adds nothing to any count),
    groups = (H / 4) (W / 4), parts = the ranges the groups are cut into for grad_bias.  The differences from window_k:

    s      : S^T = K Q^T is d MFMA reduction steps: product 1 + d adds; `* scale` 1; `+ bias` 1 (without a bias 0.0f is added:
             exact, the count stays an upper bound).                                                    c_s  = d + 3
    e      = expf(s - mx): the subtraction 1 (-> (c_s + 1) A and Amax in Cm, module docstring), expf 4.
    sum    : a lane adds its 4 values of every valid tile in sequence (Tk / 4 values from 0.f: Tk / 4 - 1 roundings), two xor-shuffle
             adds: Tk / 4 + 1, each term carrying its expf 4.
    inv    = 1 / sum: 1.  p = e * inv (backward; the forward multiplies the accumulated O by inv): 1.
             k_p = 4 + 4 + (Tk / 4 + 1) + 1 + 1 = Tk / 4 + 11, taken as                                 k_p  = Tk / 4 + 12
             (the + 1: phase 2 rebuilds p as expf(sc * scale + bv - mx) * inv from the saved (mx, inv) and a second evaluation of
             the score -- the same count, but an error that need not be the one inside `sum`; first order, the same formula.)
    out    : O^T = V^T P^T is Tk reduction steps: product 1 + Tk adds (`* inv` is in k_p).               k_out = k_p + Tk + 1
    dP     = V dO^T (phase 1) / dO V^T (phase 2): d reduction steps.                                     c_dp = d + 1
    D      = sum_j P_j dP_j from the recomputed tiles: per valid tile `(e dp + e dp) + (e dp + e dp)`: product 1, two adds 2; the
             running `dsum +=` over n_valid tiles: n_valid; two shuffle adds 2; `* inv` is the product that makes e a p (in k_p).
             e within pi - 1, dp within c_dp of dP|.|: (k_p + c_dp + n_valid + 5) D|.| + E_D with D|.| = sum_j P_j dP|.|_j and
             E_D = sum_j P_j Cm_j dP|.|_j (`D_from_out=False` in _core).                                 k_D  = k_p + c_dp + n_valid + 5
    dS     = (e * inv) * (dp - D): the subtraction 1 of dP|.| + D|.|, the product 1, p within pi, dp within c_dp dP|.|, D within
             k_D D|.| + E_D: as in window_k                                                              k_dS = k_p + 2 + max(c_dp, k_D)
    dQ     = K^T dS^T over the Tk valid keys (Tk + 1), then `* scale` 1.                                 k_dq = k_dS + Tk + 2
    dK     = Q^T dS over ALL T queries (queries are not masked), then `* scale`.                         k_dk = k_dS + T + 2
    dV     = dO^T P over the T queries.                                                                  k_dv = k_p + T + 1
    bias   : a lane's `db += ds` over the groups of its part in group order from 0.f (the largest part holds
             ceil(groups / parts) groups: one rounding less than that), then k_sum_parts adds the parts in part order (parts - 1).
             No atomics and no sum over heads (the bias is per head).                 k_bias = k_dS + ceil(groups / parts) - 1 + parts - 1"""
    T, Tk = 16 * L, 16 * n_valid
    k_p = Tk // 4 + 12
    k_out = k_p + Tk + 1
    c_dp = d + 1
    k_D = k_p + c_dp + n_valid + 5
    k_dS = k_p + 2 + max(c_dp, k_D)
    per_part = -(-groups // parts)
    return dict(s=d + 3, p=k_p, out=k_out, D=k_D, dp=c_dp, dS=k_dS, dq=k_dS + Tk + 2, dk=k_dS + T + 2, dv=k_p + T + 1,
                bias=k_dS + per_part - 1 + parts - 1, D_from_out=False)


def swap_reference(qkv, bias, grad_out, n_valid, mode, heads, scale, parts=None):
    """qkv [L,H,W,3*heads*d] (q | k | v, each [heads, d]), bias [heads,T,T] or None, grad_out [L,H,W,heads*d] or None; n_valid:
    agents >= n_valid are masked keys (their K and V are never read: whatever they hold, NaN included, is replaced by 0 here);
    scale: the fp32 number passed to the kernel; parts: of the grad_bias sum (None: the library's policy).
    -> dict: out / T_out / B_out in the output's layout; with grad_out also grad_qkv / T_grad_qkv / B_grad_qkv in qkv's layout,
    grad_bias / T_grad_bias / E_grad_bias / B_grad_bias [heads,T,T] (zeros without a bias), dS [G, heads, T, T]."""
    qkv = np.asarray(qkv, np.float64)
    L, H, W, C3 = qkv.shape
    d = C3 // (3 * heads)
    T, G = 16 * L, (H // SWAP_WS) * (W // SWAP_WS)
    valid = np.arange(T) < 16 * n_valid
    q, k, v = swap_split(qkv, mode, 3, heads, d)
    k, v = (np.where(valid[None, :, None], t, 0.0) for t in (k, v))
    dO = None if grad_out is None else swap_split(np.asarray(grad_out, np.float64), mode, 1, heads, d)[0]
    b = None if bias is None else np.tile(np.asarray(bias, np.float64), (G, 1, 1))          # problem (g, h) -> bias[h]
    parts = swap_policy_parts(H, W, heads) if parts is None else int(parts)
    kk = swap_k(L, n_valid, d, G, parts)
    r = _core(q, k, v, dO, b, valid, float(scale), kk)
    put = lambda t: swap_merge(t, mode, L, H, W, heads, d)      # noqa: E731
    res = dict(k=kk, P=r["P"])
    res["out"], res["T_out"] = put(r["out"][None]), put(r["T_out"][None])
    res["B_out"] = _bound(kk["out"], res["T_out"], put(r["E_out"][None]))
    if dO is None:
        return res
    res["grad_qkv"] = put(np.stack([r["dq"], r["dk"], r["dv"]]))
    res["T_grad_qkv"] = put(np.stack([r["T_dq"], r["T_dk"], r["T_dv"]]))
    res["B_grad_qkv"] = put(np.stack([_bound(kk[n], r["T_" + n], r["E_" + n]) for n in ("dq", "dk", "dv")]))
    per = lambda t: t.reshape(G, heads, T, T)      # noqa: E731
    res["dS"] = per(r["dS"])
    res["grad_bias"], res["T_grad_bias"], res["E_grad_bias"] = per(r["dS"]).sum(0), per(r["dSa"]).sum(0), per(r["EdS"]).sum(0)
    if bias is None:
        for n in ("grad_bias", "T_grad_bias", "E_grad_bias"):
            res[n] = np.zeros((heads, T, T))
    res["B_grad_bias"] = swap_bias_bound(res, L, n_valid, d, G, parts)
    return res


def swap_bias_bound(ref, L, n_valid, d, groups, parts):
    """The grad_bias bound of a launch with `parts` parts (only the order of the sum, hence only k_bias, depends on them)."""
    return _bound(swap_k(L, n_valid, d, groups, parts)["bias"], ref["T_grad_bias"], ref["E_grad_bias"])


def swap_perm(T, Tk, h=0):
    """The key selected by each of the T queries of head h among the Tk = 16 n_valid valid keys: pi_h(i) = (11 i + 3 + 8 h) mod Tk.
    11 is coprime to 16 n for n <= 8, so the first Tk queries select every key once (and T / Tk of the queries, rounded either
    way, select one key); neighbouring queries select keys 11 apart: the selection crosses agent tiles whenever Tk > 16.
    10 i + 3 + 8 h is odd: no query selects its own index; pi(pi(i)) - i = 4 (30 i + 9 + 24 h) is no multiple of 16: the bias is not
    symmetric anywhere, a transposed read selects another key; the heads differ by 8 keys."""
    return (11 * np.arange(T) + 3 + 8 * h) % Tk


def swap_data(L, regime, seed, n_valid=None, H=8, W=12, heads=2, d=SWAP_D, use_bias=True):
    """The CoBEVT fixtures on an H x W map -> dict(qkv, bias or None, grad_out), float32.  K and V of the agents >= n_valid hold
    ordinary values here; the GPU tests poison them.
      spread    : qkv N(0, 0.8), bias N(0, 1) per head -- a softmax with many comparable weights.
      large     : q and k N(0, LARGE_STD): scores with a standard deviation of 20 (scale * sqrt(d) = 1), extremes beyond +-60; bias N(0, 1).
      uniform   : q = 0, no bias, integer k, v and grad_out: every probability is 1 / (16 n_valid) -- exactly when n_valid is a power
                  of two (T = 16 L itself is one only for L in {1, 2, 4, 8}).
      selector  : q = 0, bias[h, i, pi_h(i)] = 0 and SELECT elsewhere (swap_perm): P[i, pi_h(i)] == 1 exactly, for every n_valid.
    use_bias=False drops the bias of spread / large."""
    g = np.random.default_rng(seed)
    n_valid = L if n_valid is None else n_valid
    T, Tk = 16 * L, 16 * n_valid
    shape = (L, H, W, 3, heads, d)
    if regime in ("spread", "large"):
        qkv = g.standard_normal(shape) * 0.8
        if regime == "large":
            qkv[:, :, :, :2] *= LARGE_STD / 0.8
        bias = g.standard_normal((heads, T, T)) if use_bias else None
        gout = g.standard_normal((L, H, W, heads * d))
    else:
        qkv = g.integers(-3, 4, shape).astype(np.float64)
        qkv[:, :, :, 0] = 0.0
        gout = g.integers(-3, 4, (L, H, W, heads * d)).astype(np.float64)
        bias = None
        if regime == "selector":
            bias = np.full((heads, T, T), SELECT)
            for h in range(heads):
                bias[h, np.arange(T), swap_perm(T, Tk, h)] = 0.0
    f = lambda a: None if a is None else np.ascontiguousarray(a, F32)      # noqa: E731
    return dict(qkv=f(qkv.reshape(L, H, W, 3 * heads * d)), bias=f(bias), grad_out=f(gout))


def swap_exact(data, n_valid, mode, heads, regime):
    """What the exact CoBEVT fixtures assert bit for bit, and the largest sum of absolute terms behind it in units of the grid.
    uniform (n_valid a power of two; unit 1 / Tk): e = 1, sum = Tk, inv = 1 / Tk: out = (sum_j v_j) * inv and dV_j = sum_q dO_q * (1 * inv)
        for the valid keys j (the same row for all of them); dK = scale * sum_q 0 * dS = 0.  dQ is NOT asserted: a real gradient.
    selector (unit 1): e in {0, 1}, sum = inv = 1: out_i = v_pi(i); dP_j = dO_i . v_j and D = dP_pi(i) are integers of at most
        d max|v| max|dO|, dS = 1 * (dP - D) = 0 or 0 * (..) = 0: dQ = dK = grad_bias = 0, dV_j = sum_{i: pi(i) = j} dO_i.
    dK and dV of masked agents are zeros in both.
    -> dict(out, dk, dv [L,H,W,heads*d] float64, dq (selector only), units)."""
    qkv = data["qkv"].astype(np.float64)
    L, H, W, C3 = qkv.shape
    d = C3 // (3 * heads)
    T, Tk = 16 * L, 16 * n_valid
    v = swap_split(qkv, mode, 3, heads, d)[2]
    g = swap_split(data["grad_out"].astype(np.float64), mode, 1, heads, d)[0]
    put = lambda t: swap_merge(t[None], mode, L, H, W, heads, d)      # noqa: E731
    vmax, gmax = float(np.abs(v).max()), float(np.abs(g).max())
    dv = np.zeros_like(v)
    if regime == "uniform":
        out = np.broadcast_to(v[:, :Tk].sum(1, keepdims=True) / Tk, v.shape)
        dv[:, :Tk] = g.sum(1, keepdims=True) / Tk
        return dict(out=put(out), dk=put(np.zeros_like(v)), dv=put(dv), units=T * max(vmax, gmax))
    out = np.empty_like(v)
    for b in range(v.shape[0]):
        pi = swap_perm(T, Tk, b % heads)
        out[b] = v[b, pi]
        np.add.at(dv[b], pi, g[b])
    return dict(out=put(out), dq=put(np.zeros_like(v)), dk=put(np.zeros_like(v)), dv=put(dv), units=max(2.0 * d * vmax * gmax, T * gmax))
