"""Per-element conformance of the linear-algebra layer of the V2X-ViT encoder (heal_amd/csrc/linear.hip) against the references
of tests/linear_refs.py: heal_linear in every addressing mode (strides, x parts, colscale groups, bias per group, row map, column
parts), heal_ln_stats at its lane edges, the chunked column sums and the split-attention weights in both entry points.

Every launch works in poisoned memory: operands sit in NaN-filled buffers with PAD poisoned words on each side and must be
unmodified afterwards; an output region is prefilled with a second NaN pattern inside such a buffer, every word the reference
addresses must come back written (and equal), every other word of the region must keep the prefill, and the poison around it
must be intact.

heal_linear is compared BIT FOR BIT: x, W, residual and the handcrafted LayerNorm means are small integers, colscale and rstd
powers of two in [1/4, 2], so every product and partial sum is a multiple of 1/4 below 2^22 (`_exact_bound`) and fp32 computes
it exactly in any order.  The bias carries 16 (c // 4) on top of `_bias`, and every 16-B piece has a column of weight magnitude
zero (`_chan_mag`), so no two pieces of a reference row are equal; `linear_refs.assert_distinct` checks that and the rows."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import linear_refs as R
from tests.report import note
from tests.test_gpu_conformance import (PAD, POISON, _assert_equal, _assert_poison_outside, _bias, _chan_mag, _exact_bound, _ints,
                                        _poisoned)

pytestmark = pytest.mark.gpu

PREFILL = 0x7FC0FEED           # a NaN bit pattern other than POISON: an output region before the launch
TS, KS, NS = (1, 127, 128, 129, 300), (32, 64, 96), (128, 256, 384)    # ragged tiles; 1, 2, 3 K chunks; 1, 2, 3 column tiles


def _seed(*key):
    return zlib.crc32(repr(key).encode())


class _Operands:
    """Operands in poisoned buffers; `unchanged` compares every backing buffer, poison included, with its state at upload."""

    def __init__(self):
        self.items = []

    def _keep(self, buf, view):
        self.items.append((buf, buf.view(torch.int32).clone()))
        return view

    def put(self, src):
        if src is None:
            return None
        return self._keep(*_poisoned(torch.as_tensor(src)))

    def placed(self, mats, ld, stride):
        """mats [rows, width] each: matrix i at i * stride, its rows ld apart, poison in every gap -> flat view."""
        buf, view = _poisoned(torch.zeros(len(mats) * stride))
        view.view(torch.int32).fill_(POISON)
        for i, m in enumerate(mats):
            rows, width = m.shape
            view[i * stride:i * stride + rows * ld].view(rows, ld)[:, :width].copy_(m)
        return self._keep(buf, view)

    def unchanged(self, what):
        torch.cuda.synchronize()
        for i, (buf, snap) in enumerate(self.items):
            assert torch.equal(buf.view(torch.int32), snap), f"{what}: operand {i} (or the poison around it) was modified"


def _region(n):
    buf, view = _poisoned(torch.zeros(n))
    view.view(torch.int32).fill_(PREFILL)
    return buf, view


def _region_check(buf, view, what, mask=None):
    """-> the region on the host.  Words of `mask` (default: all) are written, the others keep the prefill, the poison around the
    region is intact."""
    torch.cuda.synchronize()
    n = view.numel()
    _assert_poison_outside(buf, PAD, PAD + n, what)
    got = view.cpu()
    pre = got.view(torch.int32) == PREFILL
    mask = torch.ones(n, dtype=torch.bool) if mask is None else torch.as_tensor(mask)
    assert not bool(pre[mask].any()), f"{what}: {int(pre[mask].sum())} output words were never written"
    assert bool(pre[~mask].all()), f"{what}: {int((~pre[~mask]).sum())} words between the outputs were written"
    return got


def _ptr(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes) if t is not None else None


# ================================================================================================ 1. heal_linear, bit for bit
def _linear_fixture(T, K, N, act=None, res=False, row_map=None, parts=1, part_gap=0, x_parts=1, x_gap=0, colscale=False, cs_part=0,
                    group_rows=0, bias_per_group=False, stats=False, lda_pad=0, ldo_pad=0, ldr_pad=0):
    """Host tensors, the layout and the scattered reference of one call (no device work)."""
    key = (T, K, N, act, res, row_map, parts, part_gap, x_parts, x_gap, colscale, cs_part, group_rows, bias_per_group, stats,
           lda_pad, ldo_pad, ldr_pad)
    g = torch.Generator().manual_seed(_seed(*key))
    groups = -(-T // group_rows) if group_rows else 1
    fx = dict(zip(("T", "K", "N", "act", "res", "row_map", "parts", "part_gap", "x_parts", "x_gap", "colscale", "cs_part",
                   "group_rows", "bias_per_group", "stats", "lda_pad", "ldo_pad", "ldr_pad"), key))
    x = _ints(g, (T, K), -3, 3)
    w = _ints(g, (N, K), -2, 2) * _chan_mag(N).view(-1, 1)
    nb = groups if bias_per_group else 1
    b = torch.stack([_bias(g, N) for _ in range(nb)])
    b = b + torch.sign(b) * 16.0 * (torch.arange(N) // 4)                 # |b| identifies the 16-B piece
    cs = st = r = None
    if colscale:
        cs = torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0])[torch.randint(0, 5, (groups, K // (cs_part or K), N), generator=g)]
    if stats:
        st = torch.stack([_ints(g, (T,), -2, 2), torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T,), generator=g)]], 1)
    if res:
        r = _ints(g, (T, N), -100, 100)
    inner, outer = row_map if row_map else (0, 0)
    kw = dict(stats=None if st is None else st.numpy(), colscale=None if cs is None else cs.numpy(), cs_part=cs_part,
              group_rows=group_rows, bias_per_group=bias_per_group)
    bn = b.numpy() if bias_per_group else b[0].numpy()
    mag = R.linear_values(x.numpy(), w.numpy(), bn, absolute=True, **kw)
    rows = R.out_rows(T, inner, outer)
    val = R.linear_values(x.numpy(), w.numpy(), bn, act=act, **kw)
    if res:
        mag = mag + r.abs().double().numpy()[rows]
        val = val + r.double().numpy()[rows]
    _exact_bound(torch.from_numpy(mag))
    R.assert_distinct(val)
    pc = N // parts
    ldo = pc + ldo_pad
    ps = T * ldo + part_gap
    flat, mask = R.scatter(val, rows, ldo, pc, ps, parts * ps)
    fx.update(x=x, w=w, b=b if bias_per_group else b[0], cs=cs, st=st, r=r, inner=inner, outer=outer, pc=pc, ldo=ldo, ps=ps,
              flat=torch.from_numpy(flat), mask=torch.from_numpy(mask), what=f"linear {key}")
    return fx


def _linear_run(fx):
    T, K, N, xp = fx["T"], fx["K"], fx["N"], fx["x_parts"]
    xk = K // xp
    lda, ldr = xk + fx["lda_pad"], N + fx["ldr_pad"]
    x_stride = T * lda + fx["x_gap"]
    o = _Operands()
    xv = o.placed([fx["x"][:, p * xk:(p + 1) * xk] for p in range(xp)], lda, x_stride)
    wv, bv, cv, sv = o.put(fx["w"]), o.put(fx["b"]), o.put(fx["cs"]), o.put(fx["st"])
    rv = o.placed([fx["r"]], ldr, T * ldr) if fx["res"] else None
    obuf, ov = _region(fx["parts"] * fx["ps"])
    if any(fx[k] for k in ("part_gap", "x_gap", "lda_pad", "ldo_pad", "ldr_pad")):      # only the ABI can express these
        _capi.call("heal_linear", _ptr(xv), lda, xk if xp > 1 else 0, x_stride, _ptr(sv), _ptr(wv), _ptr(bv),
                   int(fx["bias_per_group"]), _ptr(cv), fx["cs_part"], fx["group_rows"], _ptr(rv), ldr if fx["res"] else 0,
                   _ptr(ov), fx["ldo"], T, N, K, fx["inner"], fx["outer"], fx["pc"], fx["ps"], ops._ACT[fx["act"]], ops._stream())
    else:
        ops.linear(xv.view(xp, T, xk) if xp > 1 else xv.view(T, K), wv, bv, stats=sv, act=fx["act"],
                   residual=rv.view(T, N) if fx["res"] else None, out=ov, row_map=fx["row_map"], parts=fx["parts"], colscale=cv,
                   colscale_part=fx["cs_part"], group_rows=fx["group_rows"], bias_per_group=fx["bias_per_group"], x_parts=xp)
    got = _region_check(obuf, ov, fx["what"], fx["mask"])
    _assert_equal(got[fx["mask"]], fx["flat"][fx["mask"]], fx["what"])
    o.unchanged(fx["what"])


def _linear(*a, **kw):
    _linear_run(_linear_fixture(*a, **kw))


@pytest.mark.parametrize("N,parts", [pytest.param(128, 32, id="N128-32parts-of-4"), pytest.param(384, 4, id="N384-4parts-of-96"),
                                     pytest.param(256, 2, id="N256-2parts")])
def test_linear_column_parts(N, parts):
    """Column parts to separate buffers: parts of one 16-B piece, parts that straddle the 128-column tiles, and a part_stride
    above T * part_cols whose gap stays untouched."""
    for T in TS:
        for K in KS:
            _linear(T, K, N, parts=parts)
        _linear(T, 64, N, parts=parts, part_gap=12, act="relu", res=True)


@pytest.mark.parametrize("mode", ["alone", "residual", "parts"])
@pytest.mark.parametrize("inner,outer", [(128, 1), (128, 3), (256, 2)])
def test_linear_row_map(inner, outer, mode):
    """[outer, inner] -> [inner, outer] rows: alone, with a residual (indexed like the output) and with column parts."""
    kw = {"alone": {}, "residual": dict(res=True, act="relu"), "parts": dict(parts=2)}[mode]
    for K in KS:
        for N in NS:
            _linear(inner * outer, K, N, row_map=(inner, outer), **kw)


@pytest.mark.parametrize("K,xk", [(96, 32), (192, 64), (128, 64)])
def test_linear_x_parts(K, xk):
    """The K loop over several tensors, ragged T, and an x_part_stride above T * x_part_cols with poison between the parts."""
    for T in TS:
        for N in NS:
            _linear(T, K, N, x_parts=K // xk)
            _linear(T, K, N, x_parts=K // xk, x_gap=8, res=True, act="relu")


@pytest.mark.parametrize("name", ["every-chunk-a-part", "one-part", "x-part-width", "other-than-x-part-width"])
def test_linear_colscale(name):
    """colscale[group][k / colscale_part][n] on the weights: a new part at every 32-channel chunk, one part, parts that coincide
    with the x parts and parts that do not (K = 192: x parts of 32, colscale parts of 96)."""
    for T in TS:
        for N in NS:
            if name == "every-chunk-a-part":
                for K in KS:
                    _linear(T, K, N, colscale=True, cs_part=32)
            elif name == "one-part":
                for K in KS:
                    _linear(T, K, N, colscale=True, cs_part=K)
            elif name == "x-part-width":
                _linear(T, 96, N, colscale=True, cs_part=32, x_parts=3)
                _linear(T, 192, N, colscale=True, cs_part=64, x_parts=3)
            else:
                _linear(T, 192, N, colscale=True, cs_part=96, x_parts=6)


@pytest.mark.parametrize("bias_per_group", [False, True])
def test_linear_colscale_groups(bias_per_group):
    """group_rows = 128 at T = 300: three groups, the last ragged, with and without a bias per group."""
    for K in KS:
        for N in NS:
            for cs_part in (32, K):
                _linear(300, K, N, colscale=True, cs_part=cs_part, group_rows=128, bias_per_group=bias_per_group)
    _linear(300, 64, 256, group_rows=128, bias_per_group=bias_per_group, res=True, act="relu")      # groups without colscale
    # the group belongs to the token, not to the row the map writes it to
    _linear(384, 64, 128, row_map=(128, 3), colscale=True, cs_part=32, group_rows=128, bias_per_group=bias_per_group)


@pytest.mark.parametrize("which", ["lda", "ldo", "ldr", "all"])
def test_linear_strides(which):
    """lda = K + 4, ldo = N + 8, ldr = N + 4, singly and together: the words between the rows keep their pattern."""
    kw = {"lda": dict(lda_pad=4), "ldo": dict(ldo_pad=8), "ldr": dict(ldr_pad=4, res=True),
          "all": dict(lda_pad=4, ldo_pad=8, ldr_pad=4, res=True, act="relu")}[which]
    for T in TS:
        for K in KS:
            for N in NS:
                _linear(T, K, N, **kw)
    _linear(384, 64, 256, row_map=(128, 3), parts=2, **kw)


def test_linear_handcrafted_stats_with_three_parts():
    """The LayerNorm prologue on handcrafted statistics (integer mean, rstd in {1/2, 1, 2}, both per token), written as q | k | v:
    the qkv projection's shape of call, ragged and through the row map."""
    for T in TS:
        for K in KS:
            _linear(T, K, 384, stats=True, parts=3)
    _linear(384, 64, 384, stats=True, parts=3, row_map=(128, 3))
    _linear(300, 96, 256, stats=True, res=True, act="relu")


@pytest.mark.parametrize("C", [128, 256])
def test_linear_merged_projection(C):
    """The split-attention merge as the model calls it: three branches as x parts, a colscale part per branch, one group and one
    bias per agent, the residual."""
    for L, HW in ((3, 128), (2, 256)):
        _linear(L * HW, 3 * C, C, x_parts=3, colscale=True, cs_part=C, group_rows=HW, bias_per_group=True, res=True)


# ================================================================================================ error contract
def _raises(name, *args):
    with pytest.raises(_capi.HealAmdError):
        _capi.call(name, *args)


def test_linear_rejects_every_violated_requirement():
    """One call per HEAL_REQUIRE of heal_linear that violates only that condition; all are refused before anything is launched,
    so the prefilled output is untouched at the end."""
    T, K, N = 128, 96, 128
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    x, w, b, r, st, cs = z(T, K + 8), z(N, K), z(N + 4), z(T, N + 8), z(T + 1, 2), z(3, N)
    obuf, out = _region(T * N + 8)
    base = dict(x=_ptr(x), lda=K, xpc=0, xps=0, st=None, w=_ptr(w), b=_ptr(b), bpg=0, cs=None, csp=0, gr=0, r=None, ldr=0,
                out=_ptr(out), ldo=N, T=T, N=N, K=K, mi=0, mo=0, pc=0, ps=0, act=0)

    def call(**kw):
        a = dict(base, **kw)
        return ("heal_linear", a["x"], a["lda"], a["xpc"], a["xps"], a["st"], a["w"], a["b"], a["bpg"], a["cs"], a["csp"], a["gr"],
                a["r"], a["ldr"], a["out"], a["ldo"], a["T"], a["N"], a["K"], a["mi"], a["mo"], a["pc"], a["ps"], a["act"],
                ops._stream())
    bad = [dict(N=64, ldo=64), dict(K=48, lda=48), dict(K=0, lda=0),                                  # N % 128, K % 32, K >= 32
           dict(lda=K + 2), dict(x=_ptr(x, 4)), dict(w=_ptr(w, 4)),                                    # 16-B alignment of x, W
           dict(gr=64), dict(gr=-128),                                                                 # groups of whole tiles
           dict(cs=_ptr(cs), csp=0), dict(cs=_ptr(cs), csp=16), dict(cs=_ptr(cs), csp=64),             # colscale parts
           dict(mi=128, mo=2), dict(mi=64, mo=2), dict(mi=-128, mo=-1), dict(mi=128, mo=0),            # row map
           dict(pc=6, ps=T * 8, ldo=8), dict(ldo=N + 2), dict(r=_ptr(r), ldr=N + 2),                   # 16-B output pieces
           dict(act=3), dict(act=-1),
           dict(xpc=48, xps=T * 48, lda=48), dict(xpc=64, xps=T * 64, lda=64), dict(xpc=-32, xps=T * 32, lda=32),
           dict(xpc=32, xps=T * 32, lda=32, st=_ptr(st)),                                              # x parts carry no LayerNorm
           dict(x=None), dict(w=None), dict(out=None),
           dict(out=_ptr(out, 4)), dict(r=_ptr(r, 4), ldr=N), dict(b=_ptr(b, 4)), dict(st=_ptr(st, 4)),
           dict(xpc=32, xps=T * 32 + 2, lda=32), dict(pc=64, ps=T * 64 + 2, ldo=64),                   # strides of the parts
           dict(lda=K - 4), dict(ldo=N - 4), dict(pc=64, ps=T * 64, ldo=60), dict(r=_ptr(r), ldr=N - 4)]
    for kw in bad:
        _raises(*call(**kw))
    with pytest.raises(_capi.HealAmdError):
        ops.linear(x[:, :K].contiguous(), w, parts=3)                      # 128 columns in three parts
    got = _region_check(obuf, out, "refused heal_linear calls", mask=torch.zeros(out.numel(), dtype=torch.bool))
    assert got.numel() == T * N + 8
    _capi.call(*call(r=_ptr(r), ldr=N + 8, st=_ptr(st), pc=64, ps=T * 64, ldo=64))       # the same operands, used lawfully
    _region_check(obuf, out, "lawful heal_linear call", mask=torch.arange(out.numel()) < T * N)


def test_ln_stats_and_split_attention_reject_every_violated_requirement():
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    s = ops._stream()
    x = z(8, 520)
    sbuf, st = _region(20)
    for args in ((_ptr(x), 8, 6, 1e-5, _ptr(st)), (_ptr(x), 8, 516, 1e-5, _ptr(st)), (_ptr(x), 8, 0, 1e-5, _ptr(st)),
                 (_ptr(x), 8, -4, 1e-5, _ptr(st)), (None, 8, 64, 1e-5, _ptr(st)), (_ptr(x), 8, 64, 1e-5, None),
                 (_ptr(x, 4), 8, 64, 1e-5, _ptr(st)), (_ptr(x), 8, 64, 1e-5, _ptr(st, 4))):
        _raises("heal_ln_stats", *args, s)
    _region_check(sbuf, st, "refused heal_ln_stats calls", mask=torch.zeros(20, dtype=torch.bool))

    C, G, rows = 64, 2, 8
    br = z(3, G * rows + 1, C)
    ps = int(br.stride(0))
    cbuf, col = _region(G * 3 * C + 8)
    cs_ok = dict(br=_ptr(br), ps=ps, G=G, rows=rows, C=C, col=_ptr(col))
    for kw in (dict(C=0), dict(C=-64), dict(C=320), dict(C=96), dict(G=0), dict(G=65536), dict(rows=0), dict(br=None),
               dict(col=None), dict(ps=ps + 2), dict(br=_ptr(br, 4)), dict(col=_ptr(col, 4))):
        a = dict(cs_ok, **kw)
        _raises("heal_split_attn_colsum", a["br"], a["ps"], a["G"], a["rows"], a["C"], a["col"], s)
    _region_check(cbuf, col, "refused heal_split_attn_colsum calls", mask=torch.zeros(col.numel(), dtype=torch.bool))

    wo, bo, f1, lg, lb, f2 = z(3 * C * C + 4), z(3, C), z(C * C + 4), z(C), z(C), z(3 * C * C + 4)
    obuf, out = _region(G * 4 * C)
    sc, bi = out[:G * 3 * C], out[G * 3 * C:]
    colsum = z(1, G, 3, 1, C)
    ptrs = dict(wo=_ptr(wo), bo=_ptr(bo), f1=_ptr(f1), lg=_ptr(lg), lb=_ptr(lb), f2=_ptr(f2), sc=_ptr(sc), bi=_ptr(bi))
    nulls = [{k: None} for k in ptrs] + [dict(wo=_ptr(wo, 4)), dict(f1=_ptr(f1, 4)), dict(f2=_ptr(f2, 4))]
    ok = dict(ptrs, cs=_ptr(colsum), parts=1, G=G, rows=rows, C=C)
    for kw in nulls + [dict(cs=None), dict(C=0), dict(C=320), dict(C=96), dict(parts=0), dict(rows=0), dict(G=0)]:
        a = dict(ok, **kw)
        _raises("heal_split_attn_weights_from_colsum", a["cs"], a["parts"], a["G"], a["rows"], a["C"], a["wo"], a["bo"], a["f1"],
                a["lg"], a["lb"], 1e-5, a["f2"], a["sc"], a["bi"], s)
    ok = dict(ptrs, br=_ptr(br), ps=ps, G=G, rows=rows, C=C, ws=_ptr(col))
    for kw in nulls + [dict(br=None), dict(ws=None), dict(C=0), dict(C=96), dict(G=0), dict(rows=0), dict(ps=ps + 2),
                       dict(br=_ptr(br, 4)), dict(ws=_ptr(col, 4))]:
        a = dict(ok, **kw)
        _raises("heal_split_attn_weights", a["br"], a["ps"], a["G"], a["rows"], a["C"], a["wo"], a["bo"], a["f1"], a["lg"],
                a["lb"], 1e-5, a["f2"], a["ws"], a["sc"], a["bi"], s)
    _region_check(obuf, out, "refused split-attention calls", mask=torch.zeros(out.numel(), dtype=torch.bool))
    _region_check(cbuf, col, "refused split-attention calls (workspace)", mask=torch.zeros(col.numel(), dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.split_attn_weights_from_colsum(z(1, G, 3, 2, C), rows, wo, bo, f1, lg, lb, 1e-5, f2)      # chunks do not match rows


# ================================================================================================ 2. heal_ln_stats at its lane edges
@pytest.mark.parametrize("C,T", [pytest.param(4, 9, id="C4-one-lane"), pytest.param(32, 9, id="C32"), pytest.param(252, 9, id="C252"),
                                 pytest.param(260, 9, id="C260-lane0-two-pieces"), pytest.param(508, 9, id="C508-partial-pass"),
                                 pytest.param(512, 9, id="C512")] +
                         [pytest.param(256, T, id=f"C256-T{T}") for T in (1, 3, 4, 5, 17)])
def test_ln_stats_lane_edges(C, T):
    """(mean, rstd) of tokens with |mean| >> std within the bound of test_linear_layernorm_stats_per_element_bound, and bit for
    bit equal to the fp32 emulation of the kernels' one arithmetic order (k_ln_stats256 claims the general kernel's)."""
    eps = 1e-5
    g = torch.Generator().manual_seed(_seed(C, T))
    x = (50.0 + 0.5 * torch.randn((T, C), generator=g)).float()
    o = _Operands()
    xv = o.put(x)
    sbuf, sv = _region(2 * T)
    _capi.call("heal_ln_stats", _ptr(xv), T, C, eps, _ptr(sv), ops._stream())
    got = _region_check(sbuf, sv, f"ln_stats C={C} T={T}").view(T, 2)
    o.unchanged("ln_stats")
    assert torch.equal(ops.ln_stats(xv, eps).cpu(), got), "ops.ln_stats differs from the direct call"
    mean, r, e_m, e_r = R.ln_stats_bounds(x.numpy(), eps)
    gd = got.double().numpy()
    assert (np.abs(gd[:, 0] - mean) <= e_m).all(), "ln_stats mean beyond its bound"
    assert (np.abs(gd[:, 1] - r) <= e_r).all(), "ln_stats rstd beyond its bound"
    emu = R.ln_stats_f32(x.numpy(), eps)
    assert np.array_equal(got.numpy(), emu), f"ln_stats differs from its fp32 order in {int((got.numpy() != emu).sum())} words"


# ================================================================================================ 3. column sums, exact
def _colsum(o, brv, part_stride, groups, rows, C, what):
    """heal_split_attn_colsum through the ABI into a prefilled region -> [groups, 3, chunks, C] on the host."""
    n = groups * 3 * R.n_chunks(rows) * C
    cbuf, cv = _region(n)
    _capi.call("heal_split_attn_colsum", _ptr(brv), part_stride, groups, rows, C, _ptr(cv), ops._stream())
    got = _region_check(cbuf, cv, what).view(groups, 3, R.n_chunks(rows), C)
    o.unchanged(what)
    return got


def _colsum_rows(C):
    rpg = 1024 // C
    return (1, 3, 4 * rpg - 1, 4 * rpg, 4 * rpg + 1, 511, 512, 513, 1030)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_colsum_exact(C, groups):
    """Per-chunk column sums of integers |v| <= 8 equal the int64 sums: the four-chain interleave and its tail, the 512-row
    chunks and their ragged last one, 48 lanes per row at C = 192.  The wrapper and a second call agree bit for bit."""
    for rows in _colsum_rows(C):
        g = torch.Generator().manual_seed(_seed(C, groups, rows))
        br = _ints(g, (3, groups * rows, C), -8, 8)
        want = torch.from_numpy(R.colsum_exact(br.numpy(), groups, rows))
        o = _Operands()
        brv = o.put(br)
        what = f"colsum C={C} groups={groups} rows={rows}"
        got = _colsum(o, brv, groups * rows * C, groups, rows, C, what)
        assert got.shape == want.shape and torch.equal(got.to(torch.int64), want) and torch.equal(got, got.round()), what
        via_ops = ops.split_attn_colsum(brv, groups, rows).cpu()
        assert torch.equal(via_ops, got), what + ": ops.split_attn_colsum differs from the direct call"
        assert torch.equal(ops.split_attn_colsum(brv, groups, rows).cpu(), via_ops), what + ": two calls differ"


@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_colsum_wide_part_stride(C):
    """A part_stride above groups * rows * C, poison between the branches."""
    groups, rows = 3, 513
    g = torch.Generator().manual_seed(_seed(C, "wide"))
    br = _ints(g, (3, groups * rows, C), -8, 8)
    o = _Operands()
    stride = groups * rows * C + 20
    brv = o.placed([br[i] for i in range(3)], C, stride)
    got = _colsum(o, brv, stride, groups, rows, C, f"colsum wide C={C}")
    assert torch.equal(got.to(torch.int64), torch.from_numpy(R.colsum_exact(br.numpy(), groups, rows)))


# ================================================================================================ 4. split-attention weights
_PARAMS = ("w_out", "b_out", "fc1", "ln_g", "ln_b", "fc2")


def _weights(br, groups, rows, p, eps, what):
    """heal_split_attn_weights through the ABI (workspace, scale and bias in prefilled regions) and through ops.split_attn_weights,
    which must agree bit for bit -> (scale [groups, 3, C], bias [groups, C]) on the host."""
    C = br.shape[-1]
    o = _Operands()
    brv = o.put(br)
    pv = [o.put(p[k]) for k in _PARAMS]
    n_ws = _capi.query("heal_split_attn_workspace", groups, rows, C) // 4
    n_sum = groups * 3 * R.n_chunks(rows) * C
    wbuf, wsv = _region(n_ws)
    sbuf, sv = _region(groups * 3 * C)
    bbuf, bv = _region(groups * C)
    _capi.call("heal_split_attn_weights", _ptr(brv), groups * rows * C, groups, rows, C, *(_ptr(v) for v in pv[:5]), float(eps),
               _ptr(pv[5]), _ptr(wsv), _ptr(sv), _ptr(bv), ops._stream())
    _region_check(wbuf, wsv, what + " workspace", mask=torch.arange(n_ws) < n_sum)
    scale = _region_check(sbuf, sv, what + " scale").view(groups, 3, C)
    bias = _region_check(bbuf, bv, what + " bias").view(groups, C)
    s2, b2 = ops.split_attn_weights(brv, groups, rows, *pv[:5], eps, pv[5])
    assert torch.equal(s2.cpu(), scale) and torch.equal(b2.cpu(), bias), what + ": the wrapper (a second call) differs"
    o.unchanged(what)
    return scale.numpy(), bias.numpy()


def _weights_from_stripes(br, groups, n_parts, rpp, p, eps, what):
    """The two halves as dist.py runs them: a column sum per stripe, stacked [n_parts, groups, 3, chunks, C], then
    heal_split_attn_weights_from_colsum into prefilled regions and through its wrapper."""
    C = br.shape[-1]
    o = _Operands()
    sums = []
    for i, stripe in enumerate(R.stripes(np.asarray(br), groups, n_parts, rpp)):
        sv_ = o.put(torch.from_numpy(stripe))
        sums.append(_colsum(o, sv_, groups * rpp * C, groups, rpp, C, f"{what} stripe {i}"))
        assert torch.equal(ops.split_attn_colsum(sv_, groups, rpp).cpu(), sums[-1])
    cv = o.put(torch.stack(sums))
    pv = [o.put(p[k]) for k in _PARAMS]
    sbuf, sv = _region(groups * 3 * C)
    bbuf, bv = _region(groups * C)
    _capi.call("heal_split_attn_weights_from_colsum", _ptr(cv), n_parts, groups, rpp, C, *(_ptr(v) for v in pv[:5]), float(eps),
               _ptr(pv[5]), _ptr(sv), _ptr(bv), ops._stream())
    scale = _region_check(sbuf, sv, what + " scale").view(groups, 3, C)
    bias = _region_check(bbuf, bv, what + " bias").view(groups, C)
    s2, b2 = ops.split_attn_weights_from_colsum(cv, rpp, *pv[:5], eps, pv[5])
    assert torch.equal(s2.cpu(), scale) and torch.equal(b2.cpu(), bias), what + ": the wrapper (a second call) differs"
    o.unchanged(what)
    return scale.numpy(), bias.numpy()


@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_weights_uniform_gate_exact(C):
    """fc2 = 0: every logit is zero, every scale word float32(1) / float32(3), and bias the fp32 expression
    (a0 b0 + a1 b1) + a2 b2 in the kernel's order (the library is built with -ffp-contract=off)."""
    groups, rows = 3, 600
    br = R.split_branches(C, groups, rows, C)
    p = R.split_params(C, C + 1, fc2_zero=True)
    third = np.float32(1.0) / np.float32(3.0)
    b = p["b_out"]
    want_bias = np.broadcast_to((third * b[0] + third * b[1]) + third * b[2], (groups, C))
    for scale, bias in (_weights(br, groups, rows, p, 1e-5, f"uniform C={C}"),
                        _weights_from_stripes(br, groups, 2, rows // 2, p, 1e-5, f"uniform halves C={C}")):
        assert (scale == third).all() and np.array_equal(bias, want_bias)


@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_weights_one_hot_gate_exact(C):
    """One branch's logit exceeds the others by more than 200 in every channel, the winner varying by channel and group: relying
    only on expf(x) == 0 for x <= -200, scale is exactly one-hot and bias is b_out[winner]."""
    groups, rows = 3, 130
    br, p, winner = R.onehot_fixture(C, groups, rows, C)
    lg = np.sort(R.split_weights_reference(br, groups, 1, rows, p, 1e-5)["logits"], 1)
    assert (lg[:, 2] - lg[:, 1] > 200.0).all()
    want = (np.arange(3)[None, :, None] == winner[:, None, :]).astype(np.float32)
    want_bias = np.take_along_axis(p["b_out"], winner, 0)
    for scale, bias in (_weights(br, groups, rows, p, 1e-5, f"one-hot C={C}"),
                        _weights_from_stripes(br, groups, 2, rows // 2, p, 1e-5, f"one-hot halves C={C}")):
        assert np.array_equal(scale, want) and np.array_equal(bias, want_bias)


@pytest.mark.parametrize("n_parts,m", [(2, 1), (3, 1), (5, 1), (2, 2)])
@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_sharded_equals_unsharded(C, n_parts, m):
    """Stripes of 512 m rows per group, summed per stripe and reduced part-major, give the scale and bias of the unsharded call
    BIT FOR BIT (include/heal_amd.h; what the striped multi-GPU encoder depends on): 2, 3, 4 and 5 partial sums per channel."""
    groups, rpp = 2, 512 * m
    br = R.split_branches(C, groups, n_parts * rpp, _seed(C, n_parts, m) % 10000)
    p = R.split_params(C, C + n_parts)
    whole = _weights(br, groups, n_parts * rpp, p, 1e-5, f"unsharded C={C}")
    halves = _weights_from_stripes(br, groups, n_parts, rpp, p, 1e-5, f"sharded C={C} {n_parts}x{rpp}")
    assert np.array_equal(whole[0], halves[0]) and np.array_equal(whole[1], halves[1])
    assert np.isfinite(whole[0]).all() and np.allclose(whole[0].sum(1), 1.0, atol=1e-6)


@pytest.mark.parametrize("C", [64, 128, 192, 256])
def test_split_attn_weights_per_element_bound(C):
    """Random floats against the float64 evaluation of split_attn.py:43-62, every scale and bias word within the bound derived
    in tests/linear_refs.py from the kernels' operation sequence (nothing normalised by a tensor-wide maximum).  The worst
    ratio per C goes to the parity report (`linear_conformance.split_weights_bound`); measured on the MI355X: 4.6e-5 (C = 64),
    1.0e-5 (128), 6.5e-6 (192), 3.7e-6 (256) of the worst-case bound."""
    worst = 0.0
    for case in (c for c in R.BOUND_CASES if c[0] == C):
        _, groups, n_parts, rpp, eps = case
        br, p, ref = R.bound_fixture(case)
        if n_parts == 1:
            scale, bias = _weights(br, groups, rpp, p, eps, f"bound {case}")
        else:
            scale, bias = _weights_from_stripes(br, groups, n_parts, rpp, p, eps, f"bound {case}")
        rs, rb = R.max_ratio(scale, ref["scale"], ref["B_scale"]), R.max_ratio(bias, ref["bias"], ref["B_bias"])
        print(f"split_weights bound {case}: scale {rs:.3e} bias {rb:.3e} x the bound")
        worst = max(worst, rs, rb)
        assert rs <= 1.0 and rb <= 1.0, f"{case}: {rs:.3f} (scale) / {rb:.3f} (bias) x the per-element bound"
    note("linear_conformance.split_weights_bound", C=C, worst_ratio=worst)
