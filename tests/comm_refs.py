"""Float64 restatements for Where2comm's communication path, shared by tests/test_comm_refs_cpu.py, the GPU suites and the fixture
generator (tests/golden/gen_golden_w2c_comm.py).  numpy only; nothing here imports the package under test.

  mask_chain       comm_modules/where2comm.py:34-78 + the max_pool2d per level of where2comm_attn.py:264-275, in float64: sigmoid,
                   maximum over anchors, k x k filter with zero padding, threshold, the even-agent override, count and rate, the
                   2^l x 2^l maximum per level
  masked_max / masked_att   "premultiply, then fuse": tests/coalign_refs.py's references of heal_warp_att_fuse_levels on x * mask
"""
import numpy as np

from tests import coalign_refs as CR

F32 = np.float32


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def smoothed(psm, weight=None, bias=0.0):
    """psm [n, A, H, W] logits -> s [n, H, W] float64: c = max_a sigmoid(psm[a]); s = bias + sum_t w[t] c[tap t] with zero padding
    of (k - 1) / 2, or c itself when weight is None."""
    c = sigmoid64(psm).max(axis=1)
    if weight is None:
        return c
    w = np.asarray(weight, np.float64)
    k = w.shape[-1]
    w = w.reshape(k, k)
    r = (k - 1) // 2
    n, H, W = c.shape
    pad = np.zeros((n, H + 2 * r, W + 2 * r))
    pad[:, r:r + H, r:r + W] = c
    s = np.full((n, H, W), float(np.asarray(bias, np.float64).reshape(-1)[0]))
    for dy in range(k):
        for dx in range(k):
            s = s + w[dy, dx] * pad[:, dy:dy + H, dx:dx + W]
    return s


def pool_levels(mask, n_levels):
    """mask [n, H, W] of zeros and ones -> [mask of level l]: the maximum over the 2^l x 2^l square, [n, H >> l, W >> l] (floor)."""
    out = [mask]
    n, H, W = mask.shape
    for l in range(1, n_levels):
        q, Hl, Wl = 1 << l, H >> l, W >> l
        out.append(mask[:, :Hl * q, :Wl * q].reshape(n, Hl, q, Wl, q).max(axis=(2, 4)) if Hl and Wl else np.zeros((n, Hl, Wl), mask.dtype))
    return out


def mask_chain(psm, record_len, weight, bias, thre, n_levels=1):
    """-> dict(s [n, H, W] float64, raw [n, H, W] uint8 (before the override), masks [level][n, H_l, W_l] uint8, count [B] int,
    rate float32 (the reference's fp32 chain: count / (H W) per scene, added in scene order, divided by B), margin: the smallest
    |s - thre|)."""
    s = smoothed(psm, weight, bias)
    raw = (s > float(thre)).astype(np.uint8)
    forced = raw.copy()
    count, start = [], 0
    for n in record_len:
        count.append(int(raw[start].sum()))
        forced[start:start + n:2] = 1                       # :69-71: agents 0, 2, 4, ... of the scene
        start += n
    assert start == s.shape[0]
    H, W = s.shape[1:]
    rate = F32(0)
    for c in count:
        rate = F32(rate + F32(F32(c) / F32(H * W)))
    rate = F32(rate / F32(len(count)))
    return dict(s=s, raw=raw, masks=pool_levels(forced, n_levels), count=np.array(count), rate=rate,
                margin=float(np.abs(s - float(thre)).min()))


def premultiply(feats, masks):
    """feats [n, C, H, W] fp32, masks [n, 1, H, W] of zeros and ones -> x * m as fp32 (exact)."""
    return np.ascontiguousarray(np.asarray(feats, F32) * np.asarray(masks, F32))


def masked_max(feats, masks, rows, grid_f64=True):
    return CR.max_reference(premultiply(feats, masks), rows, grid_f64)


def masked_att(feats, masks, rows, sqrt_dim=None, grid_f64=True):
    """-> coalign_refs.att_reference of the premultiplied maps: dict(out, B, layout, ...), B the per-element bound."""
    return CR.att_reference(premultiply(feats, masks), rows, sqrt_dim, grid_f64)
