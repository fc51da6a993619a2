"""numpy restatement of cross-covariance attention (XCA) in the folded NCHW form of include/heal_amd_align.h, and of one SDTAEncoder
(feature_alignnet_modules.py:33-67, 105-160).  float64 by default: the yardstick of the XCA kernel tests.  `dtype=np.float32` runs
the same expressions in fp32, which the kernel tests use to measure the error of plain fp32 arithmetic on their inputs.

    G_b,h[i,j] = sum_n q[b,h,i,n] k[b,h,j,n]           nq[i] = max(||q_i||, 1e-12), nk[j] likewise
    A_b,h      = softmax_j(G[i,j] / (nq[i] nk[j]) * temperature[h])
    W_b        = (gamma_xca (.) W_proj) blockdiag_h(A_b,h)
    y_b        = t_b + W_b v_b + gamma_xca (.) b_proj

tests/test_align_refs_cpu.py pins it to the reference's own hooked block outputs."""
import numpy as np
from scipy.special import erf

EPS_NORMALIZE = 1e-12


def split_qkv(qkv, heads):
    """qkv [B, 3C, N] -> q, k, v [B, heads, d, N]: channel s C + h d + i is row i of head h."""
    B, C3, N = qkv.shape
    C = C3 // 3
    r = qkv.reshape(B, 3, heads, C // heads, N)
    return r[:, 0], r[:, 1], r[:, 2]


def xca_stats(qkv, heads, dtype=np.float64):
    """-> G [B, heads, d, d], squared norms of the q rows and of the k rows [B, heads, d]."""
    q, k, _ = split_qkv(np.asarray(qkv, dtype), heads)
    return np.matmul(q, np.swapaxes(k, -1, -2)), (q * q).sum(-1), (k * k).sum(-1)


def abs_gram(qkv, heads):
    """sum_n |q_i[n] k_j[n]| [B, heads, d, d] and the same for the norms (= the squared norms): the scale of the summation bound."""
    q, k, _ = split_qkv(np.abs(np.asarray(qkv, np.float64)), heads)
    return np.matmul(q, np.swapaxes(k, -1, -2))


def xca_attention(qkv, temperature, heads, dtype=np.float64):
    """-> A [B, heads, d, d]."""
    G, q2, k2 = xca_stats(qkv, heads, dtype)
    eps = dtype(EPS_NORMALIZE)
    nq, nk = np.maximum(np.sqrt(q2), eps), np.maximum(np.sqrt(k2), eps)
    logits = G / (nq[..., :, None] * nk[..., None, :]) * np.asarray(temperature, dtype).reshape(1, heads, 1, 1)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(dtype)


def xca_weights(qkv, temperature, proj_w_scaled, heads, dtype=np.float64):
    """-> W [B, C, C] with W[b][:, h d : (h + 1) d] = proj_w_scaled[:, h d : (h + 1) d] A_b,h."""
    A = xca_attention(qkv, temperature, heads, dtype)
    B, _, d, _ = A.shape
    pw = np.asarray(proj_w_scaled, dtype)
    C = pw.shape[0]
    W = np.zeros((B, C, C), dtype)
    for h in range(heads):
        W[:, :, h * d:(h + 1) * d] = np.matmul(pw[None, :, h * d:(h + 1) * d], A[:, h])
    return W


def layernorm_c(x, weight, bias, eps):
    """LayerNorm over axis 1 of x [B, C, N] (biased variance, eps inside the square root)."""
    u = x.mean(1, keepdims=True)
    s = ((x - u) ** 2).mean(1, keepdims=True)
    return (x - u) / np.sqrt(s + eps) * weight[None, :, None] + bias[None, :, None]


def gelu(x):
    return 0.5 * x * (1.0 + erf(x * x.dtype.type(0.7071067811865476)))


def sdta_encoder(x, sd, prefix="", heads=4, dtype=np.float64):
    """One SDTAEncoder on x [B, C, H, W] with the parameters sd[prefix + name] (the reference's state-dict names), NCHW throughout."""
    p = {k[len(prefix):]: np.asarray(v, dtype) for k, v in sd.items() if k.startswith(prefix)}
    x = np.asarray(x, dtype)
    B, C, H, W = x.shape
    t = x.reshape(B, C, H * W)
    i = 0
    while f"convs.{i}.weight" in p:                       # depthwise 1x1 + ReLU stages (the ReLU modules sit at the odd indices)
        t = np.maximum(t * p[f"convs.{i}.weight"].reshape(1, C, 1) + p[f"convs.{i}.bias"].reshape(1, C, 1), 0)
        i += 2
    xn = layernorm_c(t, p["norm_xca.weight"], p["norm_xca.bias"], 1e-6)
    qkv = np.matmul(p["xca.qkv.weight"][None], xn) + p["xca.qkv.bias"][None, :, None]
    g = p["gamma_xca"]
    Wb = xca_weights(qkv, p["xca.temperature"].reshape(-1), g[:, None] * p["xca.proj.weight"], heads, dtype)
    y = t + np.matmul(Wb, qkv[:, 2 * C:]) + (g * p["xca.proj.bias"])[None, :, None]
    yn = layernorm_c(y, p["norm.weight"], p["norm.bias"], 1e-6)
    h = gelu(np.matmul(p["pwconv1.weight"][None], yn) + p["pwconv1.bias"][None, :, None])
    o = np.matmul(p["pwconv2.weight"][None], h) + p["pwconv2.bias"][None, :, None]
    return (x.reshape(B, C, H * W) + p["gamma"][None, :, None] * o).reshape(B, C, H, W)
