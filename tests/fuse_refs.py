"""References, per-element error bounds, fp32 emulations and fixtures of the single-level fusion conformance suite
(tests/test_gpu_fuse_conformance.py): k_disco_fuse<n> of heal_amd/csrc/disco_fuse.hip (DiscoNet) and k_warp_mha_fuse<n> of
heal_amd/csrc/warp_mha.hip (Where2comm) -- numpy only, so that tests/test_fuse_refs_cpu.py can prove them against the modules' own
float64 torch arithmetic, and prove that the bounds have teeth, on a machine without a GPU.

Both kernels sample every agent's map bilinearly in the ego frame (agent 0, the ego, through its own affine row) and reduce over
the agents with a softmax in which an agent whose footprint misses the pixel takes part as a ZERO map:
    DiscoNet    h1 = relu(W1n x_j + E0), h2 = relu(W2 h1 + b2), h3 = relu(W3 h2 + b3), l_j = relu(w4 . h3 + b4)       per pixel
                p = softmax_j(l_j),  out[c] = sum_j p_j x_j[c]                              (out of reach: l_j = the MLP of E0 alone)
    Where2comm  q = (S_0(q_map) + bq) scale,  k_j = S_j(k_map_j) + bk,  v_j = S_j(v_map_j) + bv           (biases AFTER sampling)
                per head h of d = C / heads channels (channel c belongs to head c // d):
                l_jh = q_h . k_jh,  p = softmax_j(l_jh),  ctx[c] = sum_j p_j v_j[c]         (out of reach: l_jh = q_h . bk_h, v = bv)

The taps come from backward_refs.k5_taps, which forms them with the kernels' own fp32 operations, so they carry no error;
coalign_refs.sample_f32 repeats `tap4` operation for operation (ego_warped, and every output of one agent, are compared bit for
bit), and everything else is evaluated in float64 ON those fp32 taps and held, element by element, to
    |got - ref| <= SAFETY * EPS * (k * T + E) + TINY
with the conventions of tests/attention_refs.py (EPS = 2^-24 per rounding, expf = 4 EPS, -ffp-contract=off so that a product and
an add are two roundings while an explicit fmaf is one, an MFMA accumulation over n reduction steps a chain of n adds, SAFETY = 2 on
the first-order bound).  T = sum_j p_j |x_j| is the sum of the absolute terms of the output, k counts the roundings on a term's way
into it (disco_k, mha_k: derived from the kernels' statements, nothing tuned on a kernel's output) and E carries the ABSOLUTE
logit error L_j (in EPS) through the softmax exactly as coalign_refs.att_reference carries Cm: the subtraction of the maximum adds
EPS |l_j - max| <= EPS (|l_j| + lmax), the maximum is the same fp32 number in numerator and denominator, so
    a_j = L_j + |l_j|,      Cm_j = a_j + sum_i p_i a_i + 2 lmax,      E[c] = sum_j p_j Cm_j |x_j|[c].
Nothing is normalised by a tensor-wide maximum.

A documented difference: the reference SKIPS a tap outside the map; the kernels multiply element 0 of the plane by a weight of 0
(warp_taps.h: flat_taps), so a non-finite value at element 0 of a plane reaches pixels whose taps all lie outside.  Inputs here
are finite."""
import functools

import numpy as np

from tests.attention_refs import EPS, F32, SAFETY, TINY, max_ratio      # noqa: F401  (re-exported for the tests)
from tests.backward_refs import k5_taps      # noqa: F401
from tests.coalign_refs import poses, reached, sample_f32, sample_f64      # noqa: F401

M1, M2, M3 = 128, 32, 8          # PixelWeightLayer widths (disco_fuse.hip: DF_M1, DF_M2, DF_M3)
UNDERFLOW_GAP = 104.0            # expf(-104) = 6.8e-46 < 2^-150: rounds (or flushes) to 0
DOMINANT_GAP = UNDERFLOW_GAP + 1.0      # a lead of 105 in float64 is a lead of more than 104 in the kernel's fp32 logits (asserted)


def relu(a):
    return np.maximum(a, 0.0)


# =====================================================================================================================
# DiscoNet
# =====================================================================================================================
def disco_k(n, C):
    """Roundings per term of k_disco_fuse<n> in EPS, statement by statement.

    x      phase 1: `v = raw[u][0] * wt[0]; v += raw[u][1] * wt[1]; ..`, phase 2: tap4 -- the same four products and three adds in
           the same order: a tap's term takes its product 1 and at most 3 adds.                                  c_x  = 4
    h1     `acc = mfma(a, b, acc)` over C / 4 k-steps of 4: a chain of C adds from 0; the term W1n[m, c] x[c] carries x's c_x, its
           product 1 and at most C adds; `fmaxf(acc + e, 0.f)`: the add rounds once more, for the terms and for E0 alike (past the
           last channel of a chunk both operands are zero: exact).      err(h1) = l1 |W1n| |x| + |E0|,           l1   = c_x + C + 2
    h2     two chains c2[.][ks & 1] of 16 MFMAs = 64 reduction steps each, `(c2[0] + c2[1]) + b2[row]`: product 1, chain 64, the
           sum of the chains 1, the bias add 1; b2 passes the last add alone.
                                          err(h2) = l2 |W2| h1 + |b2| + |W2| err(h1),                            l2   = 128 / 2 + 3
    h3     `s = b3[o]; s = fmaf(w3[o][k], h2[k], s)` over 32 k: one rounding per fmaf, each relative to a partial sum of at most
           |b3| + |W3| h2.                err(h3) = l3 (|W3| h2 + |b3|) + |W3| err(h2),                          l3   = 32
    logit  `logit = b4; logit = fmaf(w4[o], fmaxf(s, 0.f), logit)` over 8 o; `fmaxf(logit, 0.f)`.
                                          L       = l4 (|w4| h3 + |b4|) + |w4| err(h3),                          l4   = 8
           (ReLU is 1-Lipschitz and rounds nothing: an error passes it unchanged or shrinks.)
    p      softmax_agents: `expf(p[a] - mx)`: the subtraction 1 (in a_j and lmax, module docstring), expf 4 in the numerator and 4
           in the denominator; `den += p[a]` from 0.f: n - 1 roundings; `p[a] / den`: 1.                        k_p  = n + 8
    out    `acc += prob[a] * tap4(..)` from 0.f over the agents in reach: p within k_p (+ Cm, in E), x within c_x, the product 1,
           at most n - 1 rounded adds.                                                                           k_out = 2 n + 12
    One agent: prob = 1.f and out = 0.f + 1.f * x: the sample itself (asserted bit for bit, not through k)."""
    c_x = 4
    k_p = n + 8
    return dict(x=c_x, l1=c_x + C + 2, l2=M1 // 2 + 3, l3=M2, l4=M3, p=k_p, out=k_p + c_x + 1 + (n - 1))


def disco_layers(x, xa, e0, w1n, w2, b2, w3, b3, w4, b4, k):
    """The four layers in float64 with their running absolute error bound (in EPS): x, xa [n, C, P] the samples and the samples of
    the absolute maps, e0 [128, P] -> (logit [n, P], L [n, P])."""
    a = np.abs
    h1 = relu(np.einsum("mc,ncp->nmp", w1n, x) + e0[None])
    e1 = k["l1"] * np.einsum("mc,ncp->nmp", a(w1n), xa) + a(e0)[None]
    h2 = relu(np.einsum("om,nmp->nop", w2, h1) + b2[None, :, None])
    e2 = k["l2"] * np.einsum("om,nmp->nop", a(w2), h1) + a(b2)[None, :, None] + np.einsum("om,nmp->nop", a(w2), e1)
    h3 = relu(np.einsum("om,nmp->nop", w3, h2) + b3[None, :, None])
    e3 = k["l3"] * (np.einsum("om,nmp->nop", a(w3), h2) + a(b3)[None, :, None]) + np.einsum("om,nmp->nop", a(w3), e2)
    logit = relu(np.einsum("o,nop->np", w4, h3) + b4[0])
    L = k["l4"] * (np.einsum("o,nop->np", a(w4), h3) + a(b4[0])) + np.einsum("o,nop->np", a(w4), e3)
    return logit, L


def softmax_sum(logit, L, x, xa, k_out):
    """softmax over axis 0 of logit [n, G, P] (absolute error L, in EPS) and the weighted sum of x [n, G, D, P] (|x|: xa)
    -> (out, T, E, B [G, D, P], p [n, G, P]): the module docstring's Cm / E."""
    e = np.exp(logit - logit.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    aj = L + np.abs(logit)
    Cm = aj + (p * aj).sum(0, keepdims=True) + 2.0 * np.abs(logit).max(0, keepdims=True)
    out = (p[:, :, None] * x).sum(0)
    T = (p[:, :, None] * xa).sum(0)
    E = ((p * Cm)[:, :, None] * xa).sum(0)
    return out, T, E, SAFETY * EPS * (k_out * T + E), p


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def disco_reference(feats, e0, w1n, w2, b2, w3, b3, w4, b4, rows, grid_f64=True):
    """k_disco_fuse in float64 on the fp32 taps -> dict(out, T, E, B [C, H, W]; logit, B_logit, p [n, H, W]; k).  The bounds hold
    SAFETY and EPS; max_ratio adds TINY."""
    n, C, H, W = np.asarray(feats).shape
    k = disco_k(n, C)
    x, xa = sample_f64(feats, rows, grid_f64)
    e0, w1n, w2, b2, w3, b3, w4, b4 = _f64(e0, w1n, w2, b2, w3, b3, w4, b4)
    P = H * W
    x, xa = x.reshape(n, C, P), xa.reshape(n, C, P)
    logit, L = disco_layers(x, xa, e0.reshape(M1, P), w1n, w2, b2, w3, b3, w4, b4, k)
    out, T, E, B, p = softmax_sum(logit[:, None], L[:, None], x[:, None], xa[:, None], k["out"])
    shp = lambda t: t.reshape(C, H, W)      # noqa: E731
    return dict(out=shp(out), T=shp(T), E=shp(E), B=shp(B), logit=logit.reshape(n, H, W), B_logit=SAFETY * EPS * L.reshape(n, H, W),
                p=p.reshape(n, H, W), k=k)


def disco_out_given_scores(feats, scores, rows, grid_f64=True):
    """Phase 2 alone: the float64 softmax-and-sum of the kernel's OWN fp32 logits (`scores`, taken as exact: L = 0) on the fp32 taps
    -> (out, B [C, H, W]).  The bound of disco_reference is dominated by the worst-case error of four layers; this one holds the
    second gather, the softmax and the accumulation to their own few roundings."""
    n, C, H, W = np.asarray(feats).shape
    x, xa = sample_f64(feats, rows, grid_f64)
    lg = np.asarray(scores, np.float64).reshape(n, 1, H * W)
    out, _, _, B, _ = softmax_sum(lg, np.zeros_like(lg), x.reshape(n, 1, C, -1), xa.reshape(n, 1, C, -1), disco_k(n, C)["out"])
    return out.reshape(C, H, W), B.reshape(C, H, W)


def _chain32(terms):
    """((t0 + t1) + t2) + .. in fp32 from 0.f over the first axis of fp32 terms."""
    acc = np.zeros(terms.shape[1:], F32)
    for t in terms:
        acc = (acc + t).astype(F32)
    return acc


def _fmaf(a, b, c):
    """fmaf on fp32 operands: the product of two fp32 numbers is exact in float64, the sum is rounded to 53 bits and then to 24."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _softmax32(logit):
    """softmax_agents in fp32 over axis 0: max, expf, `den += e` from 0.f, divide.  numpy's fp32 exp stands in for expf."""
    with np.errstate(under="ignore"):
        e = np.exp((logit - logit.max(0, keepdims=True)).astype(F32)).astype(F32)
    return (e / _chain32(e)[None]).astype(F32)


def emulate_disco(feats, e0, w1n, w2, b2, w3, b3, w4, b4, rows, grid_f64=True):
    """k_disco_fuse in fp32 numpy, statement for statement (the tap chain, the MFMA k-loops as product-and-add chains in k order,
    layer 2's two chains by the parity of the k-step, the fmaf chains of layers 3 and 4, softmax_agents, `acc += prob * x` in agent
    order) -> (out [C, H, W], scores [n, H, W]) float32.  A map out of reach is a zero sample here and a skipped term there: the
    same value."""
    feats = np.asarray(feats, F32)
    n, C, H, W = feats.shape
    P = H * W
    e0, w1n, w2, b2, w3, b3, w4, b4 = (np.asarray(t, F32) for t in (e0, w1n, w2, b2, w3, b3, w4, b4))
    x = sample_f32(feats, rows, grid_f64).reshape(n, C, P)
    acc = np.zeros((n, M1, P), F32)
    for c in range(C):
        acc = (acc + (w1n[None, :, c, None] * x[:, None, c]).astype(F32)).astype(F32)
    h1 = np.maximum((acc + e0.reshape(1, M1, P)).astype(F32), F32(0))
    chains = [np.zeros((n, M2, P), F32), np.zeros((n, M2, P), F32)]
    for m in range(M1):
        par = (m // 4) & 1
        chains[par] = (chains[par] + (w2[None, :, m, None] * h1[:, None, m]).astype(F32)).astype(F32)
    h2 = np.maximum(((chains[0] + chains[1]).astype(F32) + b2[None, :, None]).astype(F32), F32(0))
    logit = np.broadcast_to(b4[0], (n, P)).astype(F32)
    for o in range(M3):
        s = np.broadcast_to(b3[o], (n, P)).astype(F32)
        for m in range(M2):
            s = _fmaf(np.broadcast_to(w3[o, m], (n, P)), h2[:, m], s)
        logit = _fmaf(np.broadcast_to(w4[o], (n, P)), np.maximum(s, F32(0)), logit)
    logit = np.maximum(logit, F32(0))
    p = np.ones((1, P), F32) if n == 1 else _softmax32(logit)
    out = _chain32((p[:, None] * x).astype(F32))
    return out.reshape(C, H, W), logit.reshape(n, H, W)


# =====================================================================================================================
# Where2comm
# =====================================================================================================================
def mha_k(n, d):
    """Roundings per term of k_warp_mha_fuse<n> in EPS, from its two channel sweeps over the d channels of a head.

    sweep 1, per channel c of the head:
      xe     = tap4(x_ego): stored as it is -- ego_warped is sample_f32 bit for bit.
      q      = tap4(q_map)                       c_x = 4;   `(q + bq[c]) * scale`: 2 more.                        k_q  = c_x + 2
      k_j    = `sample_k(a, c) + bkc`            c_x, 1 more.                                                     k_k  = c_x + 1
      `prob[a] += q * k_j`: the product 1, a chain of d adds from 0.f.
    logit  l_j: its absolute error is c_s EPS A_j with A_j = scale sum_c (|q| + |bq|)(|k_j| + |bk|).               c_s  = k_q + k_k + 1 + d
    p      softmax_agents as in disco_k.                                                                         k_p  = n + 8
    sweep 2: `acc += prob[a] * (sample_k(a, C + c) + bvc)` from 0.f over ALL agents: p within k_p (+ Cm, in E), v_j = the sample
           c_x and the bias add 1, the product 1, n - 1 rounded adds.                                            k_out = 2 n + 13
    One agent: prob = 1.f and ctx = 0.f + 1.f * (S_0(v_map) + bv): asserted bit for bit, not through k."""
    c_x = 4
    c_s = (c_x + 2) + (c_x + 1) + 1 + d
    k_p = n + 8
    return dict(x=c_x, s=c_s, p=k_p, out=k_p + (c_x + 1) + 1 + (n - 1))


def mha_reference(q_map, kv_map, x_ego, bq, bk, bv, heads, scale, rows, grid_f64=True):
    """k_warp_mha_fuse in float64 on the fp32 taps; `scale` is used as given (the GPU suite passes the fp32 number the kernel
    receives) -> dict(ctx, T, E, B_ctx [C, H, W]; ego_warped [C, H, W] float32 = sample_f32; logits, B_logits, p [n, heads, H, W]; k)."""
    n, C2, H, W = np.asarray(kv_map).shape
    C, P = C2 // 2, H * W
    d = C // heads
    k = mha_k(n, d)
    rows = np.asarray(rows, np.float64)
    qs, qa = sample_f64(np.asarray(q_map)[None], rows[:1], grid_f64)
    kv, kva = sample_f64(kv_map, rows, grid_f64)
    bq, bk, bv = _f64(bq, bk, bv)
    col = lambda b: b[:, None, None]      # noqa: E731
    q = (qs[0] + col(bq)) * scale
    qab = (qa[0] + np.abs(col(bq))) * abs(scale)
    kk, kab = kv[:, :C] + col(bk)[None], kva[:, :C] + np.abs(col(bk))[None]
    v, vab = kv[:, C:] + col(bv)[None], kva[:, C:] + np.abs(col(bv))[None]
    hd = lambda t: t.reshape(t.shape[:-3] + (heads, d, P))      # noqa: E731  channel c -> (c // d, c % d)
    logits = (hd(q)[None] * hd(kk)).sum(2)                                            # [n, heads, P]
    A = (hd(qab)[None] * hd(kab)).sum(2)
    ctx, T, E, B, p = softmax_sum(logits, k["s"] * A, hd(v), hd(vab), k["out"])
    shp = lambda t: t.reshape(C, H, W)      # noqa: E731
    return dict(ctx=shp(ctx), T=shp(T), E=shp(E), B_ctx=shp(B), ego_warped=sample_f32(np.asarray(x_ego, F32)[None], rows[:1], grid_f64)[0],
                logits=logits.reshape(n, heads, H, W), B_logits=SAFETY * EPS * k["s"] * A.reshape(n, heads, H, W),
                p=p.reshape(n, heads, H, W), k=k)


def emulate_mha(q_map, kv_map, x_ego, bq, bk, bv, heads, scale, rows, grid_f64=True):
    """k_warp_mha_fuse in fp32 numpy, statement for statement -> (ctx [C, H, W], logits [n, heads, H, W]) float32."""
    kv_map = np.asarray(kv_map, F32)
    n, C2, H, W = kv_map.shape
    C, P = C2 // 2, H * W
    d = C // heads
    rows = np.asarray(rows, np.float64)
    bq, bk, bv = (np.asarray(b, F32)[:, None] for b in (bq, bk, bv))
    qs = sample_f32(np.asarray(q_map, F32)[None], rows[:1], grid_f64)[0].reshape(C, P)
    q = ((qs + bq).astype(F32) * F32(scale)).astype(F32)
    kv = sample_f32(kv_map, rows, grid_f64).reshape(n, 2 * C, P)
    kk = (kv[:, :C] + bk[None]).astype(F32)
    v = (kv[:, C:] + bv[None]).astype(F32)
    prod = (q[None] * kk).astype(F32).reshape(n, heads, d, P)
    logits = _chain32(np.moveaxis(prod, 2, 0))                                        # [n, heads, P]
    p = np.ones((1, heads, P), F32) if n == 1 else _softmax32(logits)
    ctx = _chain32((p[:, :, None] * v.reshape(n, heads, d, P)).astype(F32))
    return ctx.reshape(C, H, W), logits.reshape(n, heads, H, W)


def dominated(logit):
    """logit [n, ...] -> (mask [...]: one agent leads every other by more than DOMINANT_GAP, that agent's index [...])."""
    if logit.shape[0] == 1:
        return np.ones(logit.shape[1:], bool), np.zeros(logit.shape[1:], np.int64)
    srt = np.sort(logit, 0)
    return srt[-1] - srt[-2] > DOMINANT_GAP, logit.argmax(0)


# =====================================================================================================================
# fixtures: one table for the CPU proofs and the GPU suite
# =====================================================================================================================
MAPS = [(1, 1), (4, 16), (5, 17), (3, 5), (37, 9)]      # one pixel; exactly one 16 x 4 tile; one pixel into a second tile on both axes
DISCO_CHANNELS = [4, 8, 28, 32, 36, 68]                # one k-step; ..; a chunk tail; one 32-channel chunk; ..; two chunks and a k-step
MHA_HEADS = [(8, 8), (6, 2), (12, 4), (16, 1), (64, 4)]      # (C, heads): d = 1, 3, 3, 16, 16
LARGE = 256.0                                          # the factor on w4 / on one agent's K map of the large-logit fixtures


def _cases(chan):
    """name -> (n, channels, H, W, pose, seed, large): `chan(kind, value)` picks the channel configuration."""
    t = {}
    for n in range(1, 9):
        t[f"n{n}"] = (n, chan("base", None), 13, 21, "rot" if n > 1 else "ego", n, False)
    for n in (3, 5):
        for pose in ("identity", "offmap", "ego"):
            t[f"{pose}{n}"] = (n, chan("base", None), 13, 21, pose, 20 + n, False)
    for c in (DISCO_CHANNELS if chan("list", None) == "disco" else MHA_HEADS):
        t["C" + "x".join(str(v) for v in np.atleast_1d(c))] = (3, chan("edge", c), 5, 17, "rot", 41, False)
    for H, W in MAPS:
        t[f"{H}x{W}"] = (3, chan("base", None), H, W, "rot", 60 + H, False)
    t["large"] = (4, chan("base", None), 13, 21, "rot", 77, True)
    return t


DISCO_CASES = _cases(lambda kind, v: "disco" if kind == "list" else (12 if kind == "base" else v))
MHA_CASES = _cases(lambda kind, v: "mha" if kind == "list" else ((8, 2) if kind == "base" else tuple(v)))
DISCO_OPERANDS = ("feats", "e0", "w1n", "w2", "b2", "w3", "b3", "w4", "b4")
MHA_OPERANDS = ("q_map", "kv_map", "x_ego", "bq", "bk", "bv")


@functools.lru_cache(maxsize=None)
def disco_fixture(name):
    """Random float operands of one DiscoNet case -> dict(DISCO_OPERANDS.., w1e, rows, n, C, H, W, pose, large); computed once, never
    modified.  The weights are He-scaled, so about half of every layer's pre-activations are clamped; w4 alternates in sign and b4
    is set from the fixture's own float64 pre-activations so that the last ReLU clamps about 30 % of the logits; they are of order 1
    (`large`: w4 times 256, logits of order 100).  E0 = W1e x_0 + b1 is what the module computes from the ego's UNWARPED map:
    here b1 = 0 and every row of W1e has one entry +-2^-s, so that the fp32 E0 the kernel is given is that product exactly."""
    n, C, H, W, pose, seed, large = DISCO_CASES[name]
    g = np.random.default_rng(7000 + 131 * seed + C)
    rnd = lambda *s: g.standard_normal(s)      # noqa: E731
    feats = np.ascontiguousarray(rnd(n, C, H, W), F32)
    sel, sgn = g.integers(0, C, M1), g.choice([-1.0, 1.0], M1) * 2.0 ** g.integers(-2, 1, M1)
    w1e = np.zeros((M1, C), F32)
    w1e[np.arange(M1), sel] = sgn
    s4 = LARGE if large else 1.0
    fx = dict(feats=feats, e0=np.ascontiguousarray(sgn[:, None, None].astype(F32) * feats[0][sel]), w1e=w1e,
              w1n=(rnd(M1, C) * (2.0 / (2 * C)) ** 0.5).astype(F32), w2=(rnd(M2, M1) * (2.0 / M1) ** 0.5).astype(F32),
              b2=(rnd(M2) * 0.1).astype(F32), w3=(rnd(M3, M2) * (2.0 / M2) ** 0.5).astype(F32), b3=(rnd(M3) * 0.1).astype(F32),
              w4=(np.abs(rnd(M3)) * np.tile([1.0, -1.0], M3 // 2) * (2.0 / M3) ** 0.5 * s4).astype(F32), b4=np.array([0.25 * s4], F32),
              rows=poses(pose, n, seed), n=n, C=C, H=H, W=W, pose=pose, large=large)
    # b4 puts the 30 % quantile of w4 . h3 at zero: the last ReLU clamps that share whatever signs w4 drew
    x = sample_f64(feats, fx["rows"])[0].reshape(n, C, -1)
    d = lambda key: fx[key].astype(np.float64)      # noqa: E731
    h1 = relu(np.einsum("mc,ncp->nmp", d("w1n"), x) + d("e0").reshape(1, M1, -1))
    h2 = relu(np.einsum("om,nmp->nop", d("w2"), h1) + d("b2")[None, :, None])
    h3 = relu(np.einsum("om,nmp->nop", d("w3"), h2) + d("b3")[None, :, None])
    fx["b4"] = np.array([-np.quantile(np.einsum("o,nop->np", d("w4"), h3), 0.3)], F32)
    assert np.array_equal(fx["e0"].astype(np.float64), np.einsum("mc,chw->mhw", w1e.astype(np.float64), feats[0].astype(np.float64)))
    return fx


@functools.lru_cache(maxsize=None)
def mha_fixture(name):
    """Random float operands of one Where2comm case -> dict(MHA_OPERANDS.., heads, scale, rows, n, C, H, W, pose, large); computed
    once, never modified.  The projected maps are independent Gaussians, the biases half as wide; `scale` is 1 / sqrt(d) rounded to
    fp32, the number the kernel receives.  `large`: the K map of the last agent times 256."""
    n, (C, heads), H, W, pose, seed, large = MHA_CASES[name]
    g = np.random.default_rng(9000 + 131 * seed + C + heads)
    rnd = lambda *s: np.ascontiguousarray(g.standard_normal(s), F32)      # noqa: E731
    fx = dict(q_map=rnd(C, H, W), kv_map=rnd(n, 2 * C, H, W), x_ego=rnd(C, H, W), bq=rnd(C) * F32(0.5), bk=rnd(C) * F32(0.5),
              bv=rnd(C) * F32(0.5), heads=heads, scale=float(F32((C // heads) ** -0.5)), rows=poses(pose, n, seed), n=n, C=C, H=H, W=W,
              pose=pose, large=large)
    if large:
        fx["kv_map"][n - 1, :C] *= F32(LARGE)
    return fx


_REFS = {}


def disco_ref(name, grid_f64=True):
    """disco_reference of a case, computed once per (case, grid) and never modified."""
    key = ("disco", name, grid_f64)
    if key not in _REFS:
        fx = disco_fixture(name)
        _REFS[key] = disco_reference(*(fx[o] for o in DISCO_OPERANDS), fx["rows"], grid_f64)
    return _REFS[key]


def mha_ref(name, grid_f64=True):
    """mha_reference of a case (with the fixture's fp32 scale), computed once per (case, grid) and never modified."""
    key = ("mha", name, grid_f64)
    if key not in _REFS:
        fx = mha_fixture(name)
        _REFS[key] = mha_reference(*(fx[o] for o in MHA_OPERANDS), fx["heads"], fx["scale"], fx["rows"], grid_f64)
    return _REFS[key]
