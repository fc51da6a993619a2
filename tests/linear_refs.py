"""Float64 numpy references, fp32 emulations and per-element error bounds of the linear-algebra layer of the V2X-ViT encoder
(heal_amd/csrc/linear.hip: k_linear, k_ln_stats, k_ln_stats256, k_colsum, k_split_weights), for
tests/test_gpu_linear_conformance.py -- numpy only, so that tests/test_linear_refs_cpu.py can prove the references and the bounds
on a machine without a GPU.

ADDRESSING (heal_linear).  `linear_values` is a plain float64 evaluation of act(norm(x) (W o colscale)^T + bias); `out_rows` and
`scatter` are the header's addressing formula, written out once: token t goes to row (t % inner) * outer + t // inner, column c to
out + (c // part_cols) * part_stride + row * ldo + c % part_cols.  The fixtures of the GPU file keep every intermediate an fp32
number, so the scattered reference is compared bit for bit; `assert_distinct` makes a swapped row or 16-B piece visible.

PER-ELEMENT BOUND (split-attention weights, split_attn.py:43-62).  With u = EPS = 2^-24 one fp32 rounding and the library built
with -ffp-contract=off, the kernels' operation sequence gives, to first order (all quantities per group):
  column sum     a term of a chunk passes ceil(R / (4 rpg)) + 3 additions of its accumulator chain (R <= 512 rows of the chunk,
                 rpg = 1024 / C rows per step, up to three tail steps on chain 0), 2 of the chain merge and rpg - 1 of the LDS
                 merge; then ceil(n / 4) + 3 + 2 additions over the n = n_parts * chunks partial sums; then the product with
                 inv_rows, itself a rounded quotient (2 u).             E_mean = k_sum u mean|x|
  matvec         x.x * v.x, three fmaf, a six-level wave tree: k_mv = 4 + 6 = 10 roundings on the absolute sum, one more for the
                 bias.                                                  E_t = |W| E_mean + (k_mv + 1) u (|W| |mean| + |b|)
  gap            (t0 + t1) + t2.                                        E_gap = sum_p E_t + 2 u sum_p |t_p|
  fc1            E_h = |fc1| E_gap + k_mv u |fc1| |gap|
  LayerNorm      sums: wave tree (6) + up to 4 wave partials + the division = 11.   E_mu = mean(E_h) + 11 u mean|h|,
                 E_d = E_h + E_mu + u |d|,  E_var = mean(2 |d| E_d) + 12 u mean(d^2) + u (var + eps),
                 rstd relative: rho = E_var / (2 (var + eps)) + 2 u  -- the 1 / (2 (var + eps)) sensitivity of 1 / sqrt,
                 y = d rstd g + b: E_y = |g| r (E_d + |d| rho) + 2 u |d r g| + u |y|.   ReLU is 1-Lipschitz: E_relu <= E_y.
  fc2            E_l = |fc2| E_relu + k_mv u |fc2| relu(y)
  softmax        the maximum is the same fp32 number in numerator and denominator, its own error cancels; a logit enters with
                 delta_j = E_l,j + u |l_j - max| + 4 u (expf: 2 ulp).  A ratio of a term to a sum of such terms has the relative
                 error of at most twice the largest delta; the two additions, the reciprocal and the product add 4 u.
                 E_scale = scale (2 max_j delta_j + 4 u)
  bias           E_bias = sum_p E_scale,p |b_p| + 3 u sum_p scale_p |b_p|
and the tests assert |got - ref| <= SAFETY * E + TINY element by element.  SAFETY = 2 covers the second-order terms and nothing
else; no constant here was tuned on a kernel's output.  The fixtures keep the LayerNorm variance of every group >= 0.1, so the
bound is not driven by conditioning.
This is a worst-case bound: every error is carried through |W_out|, |fc1| and |fc2| as if all terms of a row conspired, which
costs about sqrt(C) per dense layer against roundings of random sign.  The fp32 emulation of the kernels' own order (and the
kernels, on the MI355X) sit at 3e-6 .. 5e-5 of it; what it catches is a wrong operand, divisor, chunk or term (the planted
mistakes of tests/test_linear_refs_cpu.py all leave it), not a reordering of the arithmetic.  The reorderings that matter -- the
sharded reduction, the wrapper, a second call -- are held to bit equality instead."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
TINY = 1e-30
SAFETY = 2.0
CHUNK = 512                    # rows per column-sum block (heal_split_attn_colsum)
K_MV = 10                      # roundings of a term of block_matvec: product, three fmaf, six tree levels
MIN_VAR = 0.1


def max_ratio(got, ref, bound):
    """Largest |got - ref| / (bound + TINY) over the elements (NaN or inf in `got` counts as inf): <= 1 means the bound holds."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - np.asarray(ref, np.float64)) / (np.asarray(bound, np.float64) + TINY)).max())


# ================================================================================================ heal_linear: values + addressing
def out_rows(T, inner=0, outer=0, plant=None):
    """Output row of every token: (t % inner) * outer + t // inner; inner = 0: the identity."""
    t = np.arange(T, dtype=np.int64)
    if inner <= 0:
        return t
    if plant == "swap_map":
        inner, outer = outer, inner
    return (t % inner) * outer + t // inner


def linear_values(x, w, bias=None, stats=None, colscale=None, cs_part=0, group_rows=0, bias_per_group=False, act=None,
                  absolute=False, plant=None, plant_rows=None):
    """act(norm(x) (W o colscale)^T + bias) in float64 -> [T, N].  x [T, K] (x parts concatenated along K), w [N, K], stats [T, 2]
    (mean, rstd), colscale [groups, K / cs_part, N], bias [N] or [groups, N].  absolute: the same sum on absolute values and
    without the activation (the magnitude that must stay exactly representable)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    T, K = x.shape
    N = w.shape[0]
    if stats is not None:
        st = np.asarray(stats, np.float64)
        x = (x - st[:, :1]) * st[:, 1:]
    t = np.arange(T)
    grp = t // group_rows if group_rows > 0 else np.zeros(T, np.int64)
    if plant == "group_by_tile" and group_rows > 0:
        grp = t // 128                                   # the tile index, not the tile's group
    if plant == "group_by_out_row" and group_rows > 0:
        grp = np.asarray(plant_rows) // group_rows       # the row the token is written to, not the token
    if absolute:
        x, w = np.abs(x), np.abs(w)
    out = np.zeros((T, N))
    for g in np.unique(grp):
        sel = grp == g
        wg = w
        if colscale is not None:
            part = cs_part if cs_part > 0 else K
            cs = np.asarray(colscale, np.float64)[g]                       # [K / part, N]
            wg = w * np.repeat(np.abs(cs) if absolute else cs, part, axis=0).T
        v = x[sel] @ wg.T
        if bias is not None:
            b = np.asarray(bias, np.float64)
            b = b[g] if bias_per_group else b.reshape(-1)[:N]
            v = v + (np.abs(b) if absolute else b)
        out[sel] = v
    if act == "relu" and not absolute:
        out = np.maximum(out, 0.0)
    return out


def scatter(val, rows, ldo, part_cols, part_stride, size, plant=None):
    """Place val [T, N] (token-indexed) at the header's addresses inside a flat buffer of `size` words -> (flat float64, NaN where
    nothing is written; written mask).  Addresses must be distinct and inside the buffer."""
    T, N = val.shape
    pc = part_cols if part_cols > 0 else N
    if plant == "dense_parts":
        part_stride = T * N
    c = np.arange(N, dtype=np.int64)
    addr = (c // pc)[None, :] * part_stride + np.asarray(rows, np.int64)[:, None] * ldo + (c % pc)[None, :]
    assert addr.min() >= 0 and addr.max() < size, "the reference writes outside its buffer"
    assert np.unique(addr).size == addr.size, "two outputs share an address"
    flat = np.full(size, np.nan)
    flat[addr.reshape(-1)] = val.reshape(-1)
    mask = np.zeros(size, bool)
    mask[addr.reshape(-1)] = True
    return flat, mask


def assert_distinct(val):
    """No two rows of val [T, N] are equal, and no two 16-B column pieces of a row: a swapped row or piece cannot pass."""
    T, N = val.shape
    assert np.unique(val, axis=0).shape[0] == T, "two output rows of the reference are equal"
    p = val.reshape(T, N // 4, 4)
    order = np.lexsort((p[..., 3], p[..., 2], p[..., 1], p[..., 0]), axis=1)
    s = np.take_along_axis(p, order[..., None], axis=1)
    same = (s[:, 1:] == s[:, :-1]).all(-1)
    assert not same.any(), f"two 16-B pieces of reference row {int(np.argwhere(same)[0][0])} are equal"


# ================================================================================================ heal_ln_stats (fp32 emulation)
def _wave_sum(v):
    """wave_sum of common.h on v [..., 64]: v += v[lane ^ o] for o = 32 .. 1, in fp32; every lane ends with the same value."""
    v = np.asarray(v, F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(F32)
    return v[..., 0]


def ln_stats_f32(x, eps):
    """k_ln_stats / k_ln_stats256 in their one arithmetic order: lane l holds the 16-B pieces l, l + 64; the piece sums
    (x + y) + (z + w) are added per lane, then across the wave; deviations are squared and added in element order."""
    x = np.asarray(x, F32)
    T, C = x.shape
    passes = (C + 255) // 256
    xp = np.zeros((T, passes * 256), F32)
    xp[:, :C] = x
    live = np.zeros(passes * 256, bool)
    live[:C] = True
    q = xp.reshape(T, passes, 64, 4)
    lv = live.reshape(passes, 64, 4)[:, :, 0]                              # [passes, 64]: the lane holds a piece in this pass
    s = np.zeros((T, 64), F32)
    for p in range(passes):
        piece = ((q[:, p, :, 0] + q[:, p, :, 1]).astype(F32) + (q[:, p, :, 2] + q[:, p, :, 3]).astype(F32)).astype(F32)
        s = np.where(lv[p][None, :], (s + piece).astype(F32), s)
    cf = F32(C)
    mean = (_wave_sum(s) / cf).astype(F32)
    d = np.zeros((T, 64), F32)
    for p in range(passes):
        for j in range(4):
            dv = (q[:, p, :, j] - mean[:, None]).astype(F32)
            d = np.where(lv[p][None, :], (d + (dv * dv).astype(F32)).astype(F32), d)
    var = (_wave_sum(d) / cf).astype(F32)
    rstd = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    return np.stack([mean, rstd], 1)


def ln_stats_bounds(x, eps):
    """float64 (mean, rstd) of every token and the bounds of tests/test_gpu_conformance.py's
    test_linear_layernorm_stats_per_element_bound: e_m = (C + 8) u mean|x| and, relative, e_v / (2 (var + eps)) + 3 u."""
    xd = np.asarray(x, np.float64)
    C = xd.shape[1]
    mean = xd.mean(1, keepdims=True)
    d = xd - mean
    var = (d * d).mean(1, keepdims=True)
    r = 1.0 / np.sqrt(var + eps)
    e_m = (C + 8) * EPS * np.abs(xd).mean(1, keepdims=True)
    e_d = e_m + EPS * np.abs(d)
    e_v = (2 * (np.abs(d) * e_d).sum(1, keepdims=True) + (C + 8) * EPS * (d * d).sum(1, keepdims=True)) / C
    rel_r = e_v / (2 * (var + eps)) + 3 * EPS
    return mean[:, 0], r[:, 0], e_m[:, 0], (r * rel_r)[:, 0]


# ================================================================================================ column sums
def n_chunks(rows):
    return (rows + CHUNK - 1) // CHUNK


def colsum_exact(branches, groups, rows):
    """int64 per-chunk column sums of integer branches [3, groups * rows, C] -> [groups, 3, chunks, C]."""
    b = np.asarray(branches).astype(np.int64).reshape(3, groups, rows, -1)
    ch = n_chunks(rows)
    pad = np.zeros((3, groups, ch * CHUNK, b.shape[-1]), np.int64)
    pad[:, :, :rows] = b
    return pad.reshape(3, groups, ch, CHUNK, -1).sum(3).transpose(1, 0, 2, 3)


def colsum_f32(branches, groups, rows, plant=None):
    """k_colsum in its summation order, fp32: thread (rg, piece) adds rows r0 + rg + 4 rpg i into four interleaved chains (the
    tail into chain 0), merges them as (s0 + s1) + (s2 + s3), and the rpg row groups are added in order."""
    b = np.asarray(branches, F32).reshape(3, groups, rows, -1)
    C = b.shape[-1]
    rpg = 256 // (C // 4)
    ch = n_chunks(rows)
    out = np.zeros((groups, 3, ch, C), F32)
    for k in range(ch):
        r0, r1 = k * CHUNK, min((k + 1) * CHUNK, rows)
        if plant == "drop_last_chunk" and ch > 1 and k == ch - 1:
            continue
        tot = None
        for rg in range(rpg):
            s = [np.zeros((3, groups, C), F32) for _ in range(4)]
            r = r0 + rg
            while r + 3 * rpg < r1:
                for j in range(4):
                    s[j] = (s[j] + b[:, :, r + j * rpg]).astype(F32)
                r += 4 * rpg
            while r < r1:
                s[0] = (s[0] + b[:, :, r]).astype(F32)
                r += rpg
            part = ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)
            tot = part if tot is None else (tot + part).astype(F32)
        out[:, :, k] = tot.transpose(1, 0, 2)
    return out


# ================================================================================================ split-attention weights
def split_params(C, seed, fc2_zero=False):
    """Random fp32 parameters of the operator: w_out [3, C, C], b_out [3, C], fc1 [C, C], ln_g, ln_b [C], fc2 [3 C, C]."""
    rng = np.random.default_rng(seed)
    p = dict(w_out=(rng.standard_normal((3, C, C)) / np.sqrt(C)).astype(F32),
             b_out=(0.5 * rng.standard_normal((3, C))).astype(F32),
             fc1=(rng.standard_normal((C, C)) / np.sqrt(C)).astype(F32),
             ln_g=rng.uniform(0.5, 1.5, C).astype(F32), ln_b=(0.3 * rng.standard_normal(C)).astype(F32),
             fc2=(rng.standard_normal((3 * C, C)) / np.sqrt(C)).astype(F32))
    if fc2_zero:
        p["fc2"][:] = 0
    return p


def split_branches(C, groups, rows, seed):
    """fp32 branches [3, groups * rows, C]: unit noise around an offset per (branch, group, channel), so that the averages (and
    with them the LayerNorm's variance) are of order one instead of shrinking with the number of rows."""
    rng = np.random.default_rng(seed)
    off = rng.standard_normal((3, groups, 1, C))
    return (off + rng.standard_normal((3, groups, rows, C))).astype(F32).reshape(3, groups * rows, C)


def onehot_fixture(C, groups, rows, seed):
    """(branches, params, winner [groups, C]): channel g of group g's branches carries 1000 (+- 3 of integer noise everywhere),
    w_out = fc1 = identity, so the LayerNorm leaves sqrt(C - 1) >= 7.9 in channel g and ReLU close to nothing elsewhere; fc2 has
    64 in column g of the winner's row for channel c.  The winner's logit is then >= 500 and the others' stay below 1."""
    assert groups <= 8
    rng = np.random.default_rng(seed)
    br = rng.integers(-3, 4, (3, groups, rows, C)).astype(F32)
    for g in range(groups):
        br[:, g, :, g] += 1000.0
    eye = np.eye(C, dtype=F32)
    winner = (np.arange(C)[None, :] * 7 + np.arange(groups)[:, None] + np.arange(C)[None, :] // 5) % 3
    fc2 = np.zeros((3, C, C), F32)
    for g in range(groups):
        fc2[winner[g], np.arange(C), g] = 64.0
    p = dict(w_out=np.stack([eye] * 3), b_out=rng.standard_normal((3, C)).astype(F32), fc1=eye.copy(),
             ln_g=np.ones(C, F32), ln_b=np.zeros(C, F32), fc2=fc2.reshape(3 * C, C))
    return br.reshape(3, groups * rows, C), p, winner


def split_weights_reference(branches, groups, n_parts, rows_per_part, p, eps):
    """float64 evaluation of split_attn.py:43-62 on the projected branches, and the first-order bound of the module docstring.
    -> dict(scale [groups, 3, C], bias [groups, C], B_scale, B_bias, var [groups], logits [groups, 3, C])."""
    rows = n_parts * rows_per_part
    b = np.asarray(branches, np.float64).reshape(3, groups, rows, -1)
    C = b.shape[-1]
    W, bo = p["w_out"].astype(np.float64), p["b_out"].astype(np.float64)
    fc1, fc2 = p["fc1"].astype(np.float64), p["fc2"].astype(np.float64).reshape(3, C, C)
    g_, b_ = p["ln_g"].astype(np.float64), p["ln_b"].astype(np.float64)
    u = EPS
    rpg = 256 // (C // 4)
    R = min(rows_per_part, CHUNK)
    n = n_parts * n_chunks(rows_per_part)
    k_sum = (-(-R // (4 * rpg)) + 3 + 2 + rpg - 1) + (-(-n // 4) + 3 + 2) + 2
    mean = b.mean(2)                                                       # [3, groups, C]
    E_mean = k_sum * u * np.abs(b).mean(2)
    t = np.einsum("pnc,pgc->pgn", W, mean) + bo[:, None, :]
    A_t = np.einsum("pnc,pgc->pgn", np.abs(W), np.abs(mean)) + np.abs(bo)[:, None, :]
    E_t = np.einsum("pnc,pgc->pgn", np.abs(W), E_mean) + (K_MV + 1) * u * A_t
    gap = t.sum(0)                                                         # [groups, C]
    E_gap = E_t.sum(0) + 2 * u * np.abs(t).sum(0)
    h = gap @ fc1.T
    E_h = E_gap @ np.abs(fc1).T + K_MV * u * (np.abs(gap) @ np.abs(fc1).T)
    mu = h.mean(1, keepdims=True)
    E_mu = E_h.mean(1, keepdims=True) + 11 * u * np.abs(h).mean(1, keepdims=True)
    d = h - mu
    E_d = E_h + E_mu + u * np.abs(d)
    var = (d * d).mean(1, keepdims=True)
    E_var = (2 * np.abs(d) * E_d).mean(1, keepdims=True) + 12 * u * var + u * (var + eps)
    r = 1.0 / np.sqrt(var + eps)
    rho = E_var / (2 * (var + eps)) + 2 * u
    y = d * r * g_ + b_
    E_y = np.abs(g_) * r * (E_d + np.abs(d) * rho) + 2 * u * np.abs(d * r * g_) + u * np.abs(y)
    hh = np.maximum(y, 0.0)
    lg = np.einsum("pnc,gc->gpn", fc2, hh)                                 # [groups, 3, C]
    E_l = np.einsum("pnc,gc->gpn", np.abs(fc2), E_y) + K_MV * u * np.einsum("pnc,gc->gpn", np.abs(fc2), hh)
    mx = lg.max(1, keepdims=True)
    e = np.exp(lg - mx)
    scale = e / e.sum(1, keepdims=True)
    delta = E_l + u * np.abs(lg - mx) + 4 * u
    E_scale = scale * (2 * delta.max(1, keepdims=True) + 4 * u)
    bo_g = bo[None, :, :]                                                  # [1, 3, C]
    bias = (scale * bo_g).sum(1)
    E_bias = (E_scale * np.abs(bo_g)).sum(1) + 3 * u * (scale * np.abs(bo_g)).sum(1)
    return dict(scale=scale, bias=bias, B_scale=SAFETY * E_scale, B_bias=SAFETY * E_bias, var=var[:, 0], logits=lg)


def _fma32(a, b, c):
    """fmaf on fp32 operands: the product of two fp32 numbers is exact in float64; the sum is rounded once to float64 and once
    to fp32 (a double rounding that differs from fmaf in rare ties, far below the bound this emulation is held to)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _matvec_f32(w, vec, bias=None):
    """block_matvec: out[r] = wave tree over the lanes of fmaf(x.w, v.w, fmaf(x.z, v.z, fmaf(x.y, v.y, x.x * v.x))) (+ bias[r]);
    w [rows, C], vec [C]; lanes with lane * 4 >= C contribute zero."""
    rows, C = w.shape
    wq = np.zeros((rows, 64, 4), F32)
    wq.reshape(rows, 256)[:, :C] = w
    vq = np.zeros((64, 4), F32)
    vq.reshape(256)[:C] = vec
    acc = (wq[:, :, 0] * vq[None, :, 0]).astype(F32)
    for j in (1, 2, 3):
        acc = _fma32(wq[:, :, j], np.broadcast_to(vq[None, :, j], acc.shape), acc)
    out = _wave_sum(acc)
    return out if bias is None else (out + bias.astype(F32)).astype(F32)


def _block_sum_f32(v, C):
    """The LayerNorm sums of k_split_weights: a wave tree per 64 channels, the wave partials added in order."""
    part = _wave_sum(np.asarray(v, F32).reshape(C // 64, 64))
    tot = F32(0.0)
    for x in part:
        tot = F32(tot + x)
    return tot


def split_weights_f32(colsum, rows_per_part, p, eps, plant=None):
    """k_split_weights in its operation order, fp32: colsum [n_parts, groups, 3, chunks, C] -> (scale, bias).  plant: one of the
    mistakes tests/test_linear_refs_cpu.py holds the bound against."""
    cs = np.asarray(colsum, F32)
    n_parts, groups, _, chunks, C = cs.shape
    rows_f = F32(rows_per_part) if plant == "part_rows" else F32(F32(rows_per_part) * F32(n_parts))
    inv_rows = F32(F32(1.0) / rows_f)
    eps = F32(0.0) if plant == "no_eps" else F32(eps)
    bo = p["b_out"].astype(F32)
    scale = np.zeros((groups, 3, C), F32)
    bias = np.zeros((groups, C), F32)
    for g in range(groups):
        parts = cs[:, g].transpose(1, 0, 2, 3).reshape(3, n_parts * chunks, C)       # part-major, then chunk
        t = [np.zeros((3, C), F32) for _ in range(4)]
        n, k = parts.shape[1], 0
        while k + 3 < n:
            for j in range(4):
                t[j] = (t[j] + parts[:, k + j]).astype(F32)
            k += 4
        while k < n:
            t[0] = (t[0] + parts[:, k]).astype(F32)
            k += 1
        mean = (((t[0] + t[1]).astype(F32) + (t[2] + t[3]).astype(F32)).astype(F32) * inv_rows).astype(F32)
        tt = [_matvec_f32(p["w_out"][q].astype(F32), mean[q], bo[q]) for q in range(3)]
        gap = ((tt[0] + tt[1]).astype(F32) + tt[2]).astype(F32)
        h = _matvec_f32(p["fc1"].astype(F32), gap)
        cf = F32(C)
        mu = F32(_block_sum_f32(h, C) / cf)
        d = (h - mu).astype(F32)
        var = F32(_block_sum_f32((d * d).astype(F32), C) / cf)
        rstd = F32(F32(1.0) / np.sqrt(F32(var + eps)))
        y = ((d * rstd).astype(F32) * p["ln_g"].astype(F32)).astype(F32)
        if plant != "no_ln_b":
            y = (y + p["ln_b"].astype(F32)).astype(F32)
        hh = np.maximum(y, F32(0.0))
        lg = _matvec_f32(p["fc2"].astype(F32), hh).reshape(3, C)
        mx = lg.max(0)
        e = np.exp((lg - mx[None, :]).astype(F32)).astype(F32)
        inv = (F32(1.0) / ((e[0] + e[1]).astype(F32) + e[2]).astype(F32)).astype(F32)
        a = (e * inv[None, :]).astype(F32)
        scale[g] = a
        w = np.ones_like(a) if plant == "bias_unscaled" else a
        bias[g] = (((w[0] * bo[0]).astype(F32) + (w[1] * bo[1]).astype(F32)).astype(F32) + (w[2] * bo[2]).astype(F32)).astype(F32)
    return scale, bias


def stripes(branches, groups, n_parts, rows_per_part):
    """The row stripes of the ranks: branches [3, groups * n_parts * rows_per_part, C] -> n_parts x [3, groups * rows_per_part, C]
    (stripe r holds rows [r, r + 1) * rows_per_part of every group)."""
    C = branches.shape[-1]
    b = branches.reshape(3, groups, n_parts, rows_per_part, C)
    return [np.ascontiguousarray(b[:, :, r]).reshape(3, groups * rows_per_part, C) for r in range(n_parts)]


def emulate(branches, groups, n_parts, rows_per_part, p, eps, plant=None):
    """colsum_f32 per stripe + split_weights_f32: the two kernels end to end, with an optional planted mistake."""
    br = np.asarray(branches, F32)
    if plant == "swap_branches":
        br = br[[1, 0, 2]]
    cs = np.stack([colsum_f32(s, groups, rows_per_part, plant) for s in stripes(br, groups, n_parts, rows_per_part)])
    return split_weights_f32(cs, rows_per_part, p, eps, plant)


# (C, groups, n_parts, rows_per_part, eps): one, two and three chunks, rows_per_part not a multiple of 512, every channel count
# eps = 0.1 beside the model's 1e-5: at a variance of order one, only then does an omitted eps move the result beyond the bound
BOUND_CASES = [(64, 2, 1, 300, 1e-5), (64, 3, 2, 640, 0.1), (128, 2, 1, 1030, 1e-5), (128, 1, 3, 512, 0.1),
               (192, 2, 1, 640, 0.1), (192, 1, 2, 1030, 1e-5), (192, 2, 3, 100, 1e-5), (256, 2, 1, 1030, 0.1),
               (256, 1, 2, 640, 1e-5), (256, 2, 3, 512, 1e-5)]


def bound_fixture(case):
    C, groups, n_parts, rpp, eps = case
    seed = C * 1000 + groups * 100 + n_parts * 10 + rpp % 7
    br = split_branches(C, groups, n_parts * rpp, seed)
    p = split_params(C, seed + 1)
    ref = split_weights_reference(br, groups, n_parts, rpp, p, eps)
    assert float(ref["var"].min()) >= MIN_VAR, f"fixture {case}: LayerNorm variance {float(ref['var'].min())} < {MIN_VAR}"
    return br, p, ref
