"""Exact-arithmetic conformance of the sparse 3-D convolution family (K3, heal_amd/csrc/sparse_conv.hip).

The method of tests/test_gpu_conformance.py: features are small integers scaled by 1 or 2, weights small integers scaled per output
channel by 0 / 1 / 2 (the last channel always 2), BatchNorm scales powers of two and shifts nonzero quarter-integers
(tests/sparse_fixtures.py).  Every sum is then exact in fp32 in any order, so a kernel result must equal the fp64 gather-matmul
y[o] = sum_t W[t]^T x[nbr[o, t]] on oracle_np.sparse_conv_rules BIT FOR BIT; `_exact_bound` asserts sum |w||x| * scale + |shift|
< 2^22 before each comparison.  A bug in a rare branch that changes a few rows of a 40 k-site layer cannot hide under a tolerance
normalised by the largest output here.  Operands are views inside NaN-filled buffers: a read outside an operand (row -1, a row past
the end) turns the rows it reaches into NaN, and a write outside one is found in the guard words.

Geometries (case ids; tests/test_sparse_fixtures_cpu.py asserts on the CPU that each reaches its edge):
  dense     filled boxes: whole 64- and 128-site slots with 27 live taps at every site -- 108 pair tiles, k_sp_conv2's MAXT
  isolated  sites 3 cells apart: the centre tap only
  faces     every face, edge and corner of an odd 7 x 9 x 11 grid: out-of-grid taps under stride 2, padding (1,1,1) and (0,1,1)
  seam      adjacent linear keys across batch boundaries, which no pair may cross
  counts    1, 15, 16, 17, 63, 64, 65, 127, 128, 129 sites: tail blocks of M = 64 | 128, tail tiles, partial slots
  sweep     one LiDAR frame voxelised on the SECOND grid (realistic tap occupancy, thousands of blocks)
Kernels: k_sp_conv2 (every instantiated pair, 3x3x3 stride 1 and 2, 3x1x1 stride (2,1,1); all 8 HEAL_SP_M / TPSX / DB block
shapes), k_sp_conv (HEAL_SP_CONV=v1, all 9 pairs), k_sp_tiles + k_sp_nbr_tiles (the 4 thin pairs), the hash / rank / table-only
rulebook paths, the backward (transposed rulebook, transposed instantiations, k_sp_wgrad per 2048-row chunk) and heal_sp_to_bev."""
import zlib

import numpy as np
import pytest
import torch

from tests import sparse_fixtures as F
from tests.test_gpu_conformance import (PAD, POISON, _assert_equal, _assert_poison_outside, _exact_bound, _need_experimental,
                                        _poisoned)

pytestmark = pytest.mark.gpu

PAIRS2 = [(4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (32, 16), (64, 32), (128, 64)]   # k_sp_conv2
PAIRS1 = [(4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (8, 16), (64, 16)]               # k_sp_conv
TILE_PAIRS = [(4, 16), (16, 16), (16, 32), (32, 32)]                                                            # k_sp_tiles
SHAPES = [(m, tx, db) for m in (64, 128) for tx in (1, 2) for db in (0, 1)]
GEOMS = ["dense", "isolated", "faces", "seam", "counts", "sweep"]
SECOND_GRID = [41, 2048, 2048]


def _env(monkeypatch, **kv):
    """Pin every switch that selects a sparse kernel variant or rulebook path."""
    base = {k: None for k in ("HEAL_SP_CONV", "HEAL_SP_M", "HEAL_SP_TPSX", "HEAL_SP_DB", "HEAL_SP_DBG", "HEAL_SP_TILES",
                              "HEAL_SP_TILES_D", "HEAL_SP_TILES_DBG", "HEAL_SP_SLOT_SITES", "HEAL_SP_RULEBOOK", "HEAL_SP_ROOT")}
    base.update(kv)
    for k, v in base.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


_GEOM = {}


def _geoms(name):
    """The Geometry objects of a case id (counts: one per count), built once per session."""
    if name not in _GEOM:
        if name == "counts":
            _GEOM[name] = [F.counts(n) for n in F.COUNTS]
        elif name == "sweep":
            from heal_amd import ops, synth
            R = [-102.4, -102.4, -3.0, 102.4, 102.4, 1.0]
            pts = torch.from_numpy(synth.lidar_frame(77)).cuda()
            _, c, _ = ops.voxelize(pts, R, [0.1, 0.1, 0.1], 5, 70000)
            g = F.Geometry("sweep", c.int().cpu().numpy(), SECOND_GRID, 1)
            assert g.n > 20000
            _GEOM[name] = [g]
        else:
            _GEOM[name] = [getattr(F, name)()]
    return _GEOM[name]


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())          # not hash(): string hashes change from process to process


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _ref(x, nbr, w, scale=None, shift=None, relu=False):
    """fp64 act(scale * sum_t W[t]^T x[nbr[o, t]] + shift) on the device (exact: every value is an integer or a quarter-integer
    far below 2^53); asserts the fp32 exactness bound first."""
    xd, wd = dev(x).double(), dev(w).double()
    nb = dev(np.asarray(nbr, np.int64))
    y = torch.zeros((nb.shape[0], wd.shape[2]), dtype=torch.float64, device="cuda")
    bound = torch.zeros_like(y)
    for t in range(nb.shape[1]):
        rows = (nb[:, t] >= 0).nonzero(as_tuple=True)[0]
        if rows.numel():
            xs = xd.index_select(0, nb[rows, t])
            y.index_add_(0, rows, xs @ wd[t])
            bound.index_add_(0, rows, xs.abs() @ wd[t].abs())
    if scale is not None:
        sc, sh = dev(scale).double(), dev(shift).double()
        y, bound = y * sc + sh, bound * sc.abs() + sh.abs()
    _exact_bound(bound)
    return (torch.relu(y) if relu else y).float().cpu()


def _check(got, ref, nbr, what):
    """_assert_equal, and on a mismatch the first bad row with its live taps."""
    try:
        _assert_equal(got, ref, what)
    except AssertionError as e:
        g = got.detach().cpu()
        bad = ((g != ref) | torch.isnan(g)).any(1).nonzero(as_tuple=True)[0]
        r = int(bad[0])
        taps = np.nonzero(np.asarray(nbr[r]) >= 0)[0].tolist() if r < len(nbr) else []
        raise AssertionError(f"{e}; {bad.numel()} rows differ, first row {r} with live taps {taps}") from None


def _poison_fill(rows, cols):
    """(buffer, view): a [rows, cols] view in the middle of a poisoned buffer, every word of it poisoned too."""
    buf, view = _poisoned(torch.empty((rows, cols)))
    buf.view(torch.int32).fill_(POISON)
    return buf, view


def _values(g, layer, cin, cout, seed):
    out_idx, out_shape, nbr = g.rules(layer)
    rng = np.random.default_rng(seed)
    x = F.features(rng, g.n, cin)
    w = F.weights(rng, nbr.shape[1], cin, cout)
    sc, sh = F.batchnorm(rng, cout)
    return out_idx, out_shape, nbr, x, w, sc, sh


def _conv_table(g, layer, cin, cout, relu, what, twice=False):
    """SparseTensor.conv on the oracle's neighbour table, features and weight poisoned around, against the fp64 reference."""
    from heal_amd import ops
    _, _, nbr, x, w, sc, sh = _values(g, layer, cin, cout, _seed(g.name, layer, cin, cout))
    ref = _ref(x, nbr, w, sc, sh, relu)
    bx, xv = _poisoned(torch.from_numpy(x))
    bw, wv = _poisoned(torch.from_numpy(w))
    st = ops.SparseTensor(xv, dev(g.idx), g.shape, g.batch)
    nb = dev(nbr.astype(np.int32))
    got = st.conv(nb, wv, dev(sc), dev(sh), relu=relu)
    _check(got, ref, nbr, what)
    if twice:
        assert torch.equal(st.conv(nb, wv, dev(sc), dev(sh), relu=relu), got), f"{what}: two runs differ"
    _assert_poison_outside(bx, PAD, PAD + x.size, what + " features")
    _assert_poison_outside(bw, PAD, PAD + w.size, what + " weight")


def _layers(cin, cout):
    return ["subm", "s2", "s2p011"] + (["k311"] if (cin, cout) in ((64, 64), (64, 128)) else [])


# ================================================================================================ k_sp_conv2
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("cin,cout", PAIRS2, ids=[f"{a}to{b}" for a, b in PAIRS2])
@pytest.mark.parametrize("geom", GEOMS)
def test_conv2_default_shape_exact(geom, cin, cout, relu, monkeypatch):
    """k_sp_conv2 at its default block shape on every geometry: 3x3x3 submanifold, stride 2 with padding (1,1,1) and (0,1,1),
    and 3x1x1 stride (2,1,1) (conv_out) for 64 -> 64 / 64 -> 128; two runs bitwise identical."""
    _env(monkeypatch)
    for g in _geoms(geom):
        for layer in _layers(cin, cout):
            _conv_table(g, layer, cin, cout, relu, f"k_sp_conv2 {g.name} {layer} {cin}->{cout}", twice=True)


@pytest.mark.parametrize("cin,cout", PAIRS2, ids=[f"{a}to{b}" for a, b in PAIRS2])
@pytest.mark.parametrize("geom", ["dense", "counts", "faces"])
@pytest.mark.parametrize("m,tx,db", SHAPES, ids=[f"M{m}_tps{tx}_db{db}" for m, tx, db in SHAPES])
def test_conv2_block_shapes_exact(m, tx, db, geom, cin, cout, monkeypatch):
    """All 8 instantiated block shapes (HEAL_SP_M 64|128 x HEAL_SP_TPSX 1|2 x HEAL_SP_DB 0|1) of every pair: the full 27-tap
    slots, the tail blocks and the out-of-grid taps."""
    _env(monkeypatch, HEAL_SP_M=m, HEAL_SP_TPSX=tx, HEAL_SP_DB=db)
    for g in _geoms(geom):
        for layer in ("subm", "s2"):
            _conv_table(g, layer, cin, cout, True, f"k_sp_conv2<M={m},tps x{tx},db={db}> {g.name} {layer} {cin}->{cout}")


# ================================================================================================ k_sp_conv (round 2)
@pytest.mark.parametrize("cin,cout", PAIRS1, ids=[f"{a}to{b}" for a, b in PAIRS1])
@pytest.mark.parametrize("geom", GEOMS)
def test_conv_v1_exact(geom, cin, cout, monkeypatch):
    """The round-2 kernel (HEAL_SP_CONV=v1; 8 -> 16 and 64 -> 16 reach it without the switch: no k_sp_conv2 instantiation)."""
    _env(monkeypatch, HEAL_SP_CONV="v1")
    for g in _geoms(geom):
        for layer in ("subm", "s2", "s2p011"):
            _conv_table(g, layer, cin, cout, layer != "s2", f"k_sp_conv {g.name} {layer} {cin}->{cout}", twice=layer == "subm")


# ================================================================================================ pair tiles
def _sparse_input(g, x):
    """SparseTensor.from_unsorted on already sorted sites (root rank structure): the identity permutation."""
    from heal_amd import ops
    st = ops.SparseTensor.from_unsorted(dev(x), dev(g.idx), g.shape, g.batch)
    assert torch.equal(st.indices.cpu(), torch.from_numpy(g.idx))
    assert torch.equal(st._perm.cpu(), torch.arange(g.n, dtype=torch.int32))
    return st


def _out_sites(st, g, layer):
    ks, stride, pad, subm = F.LAYERS[layer]
    out_idx, out_shape, _ = g.rules(layer)
    if subm:
        return st.indices, list(g.shape), (1, 1, 1), tuple(k // 2 for k in ks), None
    oi, oshape, _, rank = st.out_sites_ex(ks, stride, pad)
    assert list(oshape) == out_shape and torch.equal(oi.cpu(), torch.from_numpy(out_idx)), f"{g.name} {layer}: output sites"
    return oi, oshape, stride, pad, rank


@pytest.mark.parametrize("variant", ["s64", "s128", "d4"])
@pytest.mark.parametrize("cin,cout", TILE_PAIRS, ids=[f"{a}to{b}" for a, b in TILE_PAIRS])
@pytest.mark.parametrize("geom", GEOMS)
def test_pair_tiles_exact(geom, cin, cout, variant, monkeypatch):
    """k_sp_nbr_tiles + k_sp_tiles through SparseTensor.rulebook -> conv: the tiles decode to the oracle's table bit for bit, the
    convolution equals the fp64 reference, two runs are identical; on `dense` a slot reaches the worst case of 27 x 4 = 108 tiles
    (27 x 8 = 216 at 128 sites).  128-site slots and groups of 4 tiles exist only in an experimental build."""
    from heal_amd import ops
    if variant != "s64":
        _need_experimental()
    _env(monkeypatch, HEAL_SP_SLOT_SITES=128 if variant == "s128" else None, HEAL_SP_TILES_D=4 if variant == "d4" else None)
    S = 128 if variant == "s128" else 64
    for g in _geoms(geom):
        for layer in ("subm", "s2"):
            what = f"k_sp_tiles<{variant}> {g.name} {layer} {cin}->{cout}"
            _, _, nbr, x, w, sc, sh = _values(g, layer, cin, cout, _seed(g.name, layer, cin, cout, "tiles"))
            relu = layer == "subm"
            ref = _ref(x, nbr, w, sc, sh, relu)
            st = _sparse_input(g, x)
            oi, oshape, stride, pad, _ = _out_sites(st, g, layer)
            assert st.tiles_ok((3, 3, 3), cin, cout)
            tiles = st.rulebook(oi, oshape, (3, 3, 3), stride, pad, cin, cout)
            assert isinstance(tiles, ops.PairTiles) and tiles.slot_sites == S
            assert torch.equal(tiles.to_neighbors().cpu(), torch.from_numpy(nbr.astype(np.int32))), f"{what}: decoded tiles"
            n_slots = (len(nbr) + S - 1) // S
            words = tiles.buf.numel() // n_slots
            T = tiles.buf.view(n_slots, words)[:, 0].cpu()
            live = np.zeros((n_slots * S, 27), np.int64)
            live[:len(nbr)] = nbr >= 0
            want_T = ((live.reshape(n_slots, S, 27).sum(1) + 15) // 16).sum(1)
            assert np.array_equal(T.numpy(), (want_T + 3) // 4 * 4), f"{what}: tile counts in the slot headers"
            if g.name == "dense" and layer == "subm":
                assert int(T.max()) == 27 * S // 16, f"{what}: no slot reaches the worst case"
            bx, xv = _poisoned(torch.from_numpy(x))
            bw, wv = _poisoned(torch.from_numpy(w))
            st.features = xv
            got = st.conv(tiles, wv, dev(sc), dev(sh), relu=relu)
            _check(got, ref, nbr, what)
            assert torch.equal(st.conv(tiles, wv, dev(sc), dev(sh), relu=relu), got), f"{what}: two runs differ"
            _assert_poison_outside(bx, PAD, PAD + x.size, what + " features")


# ================================================================================================ rulebook paths
@pytest.mark.parametrize("mode", ["hash", "rank", "tables_only"])
@pytest.mark.parametrize("geom", GEOMS)
def test_rulebook_paths_exact(geom, mode, monkeypatch):
    """Every table path gives the oracle's rulebook and the reference's bits: HEAL_SP_RULEBOOK=hash (sort + hash grid), the
    default rank structures (the voxel set's root structure, then the strided structure of a layer's output sites for the
    submanifold layer behind it) and HEAL_SP_TILES=0 (no pair tiles anywhere)."""
    from heal_amd import ops
    _env(monkeypatch, HEAL_SP_RULEBOOK="hash" if mode == "hash" else None, HEAL_SP_TILES="0" if mode == "tables_only" else None)
    cin, cout = (32, 64) if mode == "rank" else (16, 16)      # rank: a pair the tiles do not take, so the table is built
    for g in _geoms(geom):
        for layer in ("subm", "s2", "s2p011"):
            what = f"{mode} rulebook {g.name} {layer} {cin}->{cout}"
            ks = F.LAYERS[layer][0]
            out_idx, out_shape, nbr, x, w, sc, sh = _values(g, layer, cin, cout, _seed(g.name, layer, mode))
            st = _sparse_input(g, x)
            assert (st._rank is None) == (mode == "hash")
            oi, oshape, stride, pad, rank = _out_sites(st, g, layer)
            table = st.rulebook(oi, oshape, ks, stride, pad, cin, cout)
            assert isinstance(table, torch.Tensor), what
            assert torch.equal(table.cpu(), torch.from_numpy(nbr.astype(np.int32))), f"{what}: neighbour table"
            got = st.conv(table, dev(w), dev(sc), dev(sh), relu=True)
            _check(got, _ref(x, nbr, w, sc, sh, True), nbr, what)
            if layer == "subm":
                continue
            # the submanifold layer on the new site set, through the structure out_sites_ex left (rank) or the hash grid
            assert (rank is None) == (mode == "hash")
            h = F.Geometry(f"{g.name}/{layer}", out_idx, out_shape, g.batch)
            _, _, nbr2, y, w2, sc2, sh2 = _values(h, "subm", cout, cout, _seed(h.name, mode))
            ys = ops.SparseTensor(dev(y), oi, oshape, g.batch)
            ys._rank = rank
            t2 = ys.rulebook(oi, oshape, (3, 3, 3), (1, 1, 1), (1, 1, 1), cout, cout)
            if isinstance(t2, ops.PairTiles):
                t2 = t2.to_neighbors()
            assert torch.equal(t2.cpu(), torch.from_numpy(nbr2.astype(np.int32))), f"{what}: strided structure's table"
            got2 = ys.conv(t2, dev(w2), dev(sc2), dev(sh2), relu=False)
            _check(got2, _ref(y, nbr2, w2, sc2, sh2, False), nbr2, what + " -> subm")


# ================================================================================================ backward
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64), (64, 128)], ids=["32to16", "64to32", "128to64"])
@pytest.mark.parametrize("geom", GEOMS)
def test_backward_transposed_rulebook_and_adjoint_exact(geom, cin, cout):
    """heal_sp_transpose_neighbors = the numpy transpose of the rulebook; sp_conv_raw on it with W[t]^T (the transposed
    instantiations 32 -> 16, 64 -> 32, 128 -> 64) = the exact adjoint gx[i] = sum_t W[t] g[o] of the forward layer."""
    from heal_amd import ops
    for g in _geoms(geom):
        for layer in ("subm", "s2"):
            what = f"backward {g.name} {layer} {cout}->{cin}"
            _, _, nbr = g.rules(layer)
            rng = np.random.default_rng(_seed(g.name, layer, cin, "bwd"))
            K = nbr.shape[1]
            want_t = np.full((g.n, K), -1, np.int64)
            o, t = np.nonzero(nbr >= 0)
            want_t[nbr[o, t], t] = o
            nbr_t = ops.sp_transpose_neighbors(dev(nbr.astype(np.int32)), g.n)
            assert torch.equal(nbr_t.cpu(), torch.from_numpy(want_t.astype(np.int32))), f"{what}: transposed rulebook"
            gout = F.features(rng, len(nbr), cout)
            wt = np.ascontiguousarray(F.weights(rng, K, cin, cout).transpose(0, 2, 1))
            ref = _ref(gout, want_t, wt)
            bg, gv = _poisoned(torch.from_numpy(gout))
            bw, wv = _poisoned(torch.from_numpy(wt))
            got = ops.sp_conv_raw(gv, nbr_t, wv)
            _check(got, ref, want_t, what)
            _assert_poison_outside(bg, PAD, PAD + gout.size, what + " grad_out")


def test_sp_conv_uninstantiated_pair_raises():
    """A channel pair with no kernel is an error, never an unwritten result."""
    from heal_amd import _capi, ops
    g = F.counts(65)
    _, _, nbr = g.rules("subm")
    with pytest.raises(_capi.HealAmdError, match="not instantiated"):
        ops.sp_conv_raw(torch.ones((g.n, 16), device="cuda"), dev(nbr.astype(np.int32)), torch.ones((27, 16, 48), device="cuda"))
    with pytest.raises(_capi.HealAmdError, match="not instantiated"):
        ops.sp_conv_raw(torch.ones((g.n, 12), device="cuda"), dev(nbr.astype(np.int32)), torch.ones((27, 12, 16), device="cuda"))


# ================================================================================================ k_sp_wgrad
WGRAD = [(1, 16), (3, 32), (4, 48), (5, 64), (16, 16), (48, 32), (64, 64), (64, 48), (3, 16), (16, 64), (5, 48), (1, 64)]


@pytest.mark.parametrize("n_out", [2047, 2048, 2049, 4097])
@pytest.mark.parametrize("K", [27, 3])
@pytest.mark.parametrize("cin,cout", WGRAD, ids=[f"{a}x{b}" for a, b in WGRAD])
def test_wgrad_chunks_exact(cin, cout, K, n_out):
    """heal_sp_wgrad: every 2048-row chunk's partial [K, Cin, Cout] against its own fp64 reference (a failure names the chunk),
    then the summed gradient of ops.sp_wgrad.  Chunk 0 has taps with 31, 32 and 33 pairs (the 32-pair MFMA stage seams), the last
    output row every tap live; Cin not a multiple of 4 takes the scalar gather."""
    from heal_amd import _capi, ops
    rng = np.random.default_rng(_seed(cin, cout, K, n_out))
    n_in = 1500
    nbr = F.wgrad_table(rng, n_out, n_in, K)
    x, g = F.features(rng, n_in, cin), F.features(rng, n_out, cout)
    part, bound = F.wgrad_ref(x, g, nbr)
    _exact_bound(torch.from_numpy(bound))
    chunks = _capi.query("heal_sp_wgrad_chunks", n_out)
    assert chunks == part.shape[0] == (n_out + 2047) // 2048
    bx, xv = _poisoned(torch.from_numpy(x))
    bg, gv = _poisoned(torch.from_numpy(g))
    bp, pv = _poison_fill(chunks * K * cin, cout)
    nb = dev(nbr.astype(np.int32))
    _capi.call("heal_sp_wgrad", ops._ptr(xv), ops._ptr(gv), ops._ptr(nb), n_out, K, cin, cout, None, ops._ptr(pv), ops._stream())
    pv = pv.view(chunks, K, cin, cout)
    for c in range(chunks):
        _assert_equal(pv[c], torch.from_numpy(part[c]), f"k_sp_wgrad chunk {c} of {chunks} (rows {2048 * c}..) [tap, ci, co]")
    _assert_poison_outside(bp, PAD, PAD + pv.numel(), "k_sp_wgrad partials")
    _assert_poison_outside(bx, PAD, PAD + x.size, "k_sp_wgrad x")
    _assert_poison_outside(bg, PAD, PAD + g.size, "k_sp_wgrad grad_out")
    total = ops.sp_wgrad(xv, gv, nb)
    _assert_equal(total, torch.from_numpy(part.sum(0)), "sp_wgrad sum over the chunks [tap, ci, co]")
    assert torch.equal(ops.sp_wgrad(xv, gv, nb), total)


# ================================================================================================ heal_sp_to_bev
def test_to_bev_scatter_exact_and_no_stale_cells():
    """SparseTensor.dense() = the numpy scatter with channel c * D + z, empty cells exactly 0; a second site set on the same
    workspace keeps nothing of the first (the cell map is rebuilt per call).  20 channels: a tail of the 16-channel blocks."""
    from heal_amd import ops
    shape, batch, C = (5, 8, 12), 2, 20
    rng = np.random.default_rng(3)
    cells = batch * shape[0] * shape[1] * shape[2]
    for occ in (0.4, 0.15):
        flat = np.nonzero(rng.random(cells) < occ)[0]
        idx = np.stack(np.unravel_index(flat, (batch,) + shape), 1).astype(np.int32)
        x = F.features(rng, len(idx), C)
        bx, xv = _poisoned(torch.from_numpy(x))
        got = ops.SparseTensor(xv, dev(idx), shape, batch).dense()
        ref = np.zeros((batch, C) + shape, np.float32)
        ref[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = x
        _assert_equal(got, torch.from_numpy(ref.reshape(batch, C * shape[0], shape[1], shape[2])), f"sp_to_bev occupancy {occ}")
        _assert_poison_outside(bx, PAD, PAD + x.size, "sp_to_bev features")


# ================================================================================================ device-count mode
def _capacity_operands(x, cap_in, nbr, cap_out):
    """Features with cap_in rows (rows behind the live count NaN) and a neighbour table with cap_out rows whose rows behind the live
    count point at live input rows: a kernel that ran them would write finite values where the output must stay NaN."""
    n_in, cin = x.shape
    bx, xv = _poison_fill(cap_in, cin)
    xv[:n_in] = torch.from_numpy(x).cuda()
    nbc = np.zeros((cap_out, nbr.shape[1]), np.int32)
    nbc[:len(nbr)] = nbr
    return bx, xv, dev(nbc)


@pytest.mark.parametrize("kernel", ["v2", "v1"])
@pytest.mark.parametrize("cin,cout", [(4, 16), (16, 32), (64, 64), (64, 128)], ids=["4to16", "16to32", "64to64", "64to128"])
@pytest.mark.parametrize("geom", ["dense", "counts", "seam"])
def test_conv_device_count_guards(geom, cin, cout, kernel, monkeypatch):
    """heal_sp_conv with capacity-sized operands and a device row count: live rows exact, every row at or behind the live count
    still NaN (nothing written there), NaN input rows behind the live input count never reach a live output."""
    from heal_amd import _capi, ops
    _env(monkeypatch, HEAL_SP_CONV="v1" if kernel == "v1" else None)
    for g in _geoms(geom):
        for layer in ("subm", "s2"):
            what = f"sp_conv[{kernel}] device count {g.name} {layer} {cin}->{cout}"
            _, _, nbr, x, w, sc, sh = _values(g, layer, cin, cout, _seed(g.name, layer, cin, cout, "cap"))
            ref = _ref(x, nbr, w, sc, sh, True)
            n_out = len(nbr)
            cap_in, cap_out = g.n + 37, n_out + 53
            bx, xv, nbc = _capacity_operands(x, cap_in, nbr, cap_out)
            bo, ov = _poison_fill(cap_out, cout)
            wd, scd, shd = dev(w), dev(sc), dev(sh)         # held: the kernel reads them after _capi.call returns
            n_dev = torch.tensor([n_out], dtype=torch.int32, device="cuda")
            _capi.call("heal_sp_conv", ops._ptr(xv), ops._ptr(nbc), cap_out, nbr.shape[1], cin, cout, ops._ptr(wd),
                       ops._optr(ops.sp_weight_fragments(wd)), ops._ptr(scd), ops._ptr(shd), 1, ops._ptr(ov), ops._ptr(n_dev),
                       ops._stream())
            _check(ov[:n_out], ref, nbr, what)
            assert bool((ov[n_out:].view(torch.int32) == POISON).all()), f"{what}: a row behind the live count was written"
            _assert_poison_outside(bo, PAD, PAD + ov.numel(), what + " out")
            _assert_poison_outside(bx, PAD, PAD + g.n * cin, what + " features")


@pytest.mark.parametrize("cin,cout", TILE_PAIRS, ids=[f"{a}to{b}" for a, b in TILE_PAIRS])
@pytest.mark.parametrize("geom", ["dense", "counts", "seam"])
def test_pair_tiles_device_count_guards(geom, cin, cout, monkeypatch):
    """The pair-tile path as the graph-captured encoder runs it: capacity-sized site buffers with the live counts on the device
    (heal_sp_neighbor_tiles, heal_sp_conv_tiles), NaN input rows behind the live count, a NaN-prefilled capacity-sized output."""
    from heal_amd import _capi, ops
    _env(monkeypatch)
    for g in _geoms(geom):
        for layer in ("subm", "s2"):
            what = f"sp_conv_tiles device count {g.name} {layer} {cin}->{cout}"
            out_idx, _, nbr, x, w, sc, sh = _values(g, layer, cin, cout, _seed(g.name, layer, cin, cout, "tcap"))
            ref = _ref(x, nbr, w, sc, sh, True)
            n, pad_rows = g.n, 77
            ipad = np.concatenate([g.idx, np.full((pad_rows, 4), 3, np.int32)])
            ipad[n:, 0] = 0
            fpad = np.concatenate([x, np.full((pad_rows, cin), 7.0, np.float32)])
            st = ops.SparseTensor.from_unsorted(dev(fpad), dev(ipad), g.shape, g.batch,
                                                n_dev=torch.tensor([n], dtype=torch.int32, device="cuda"))
            assert torch.equal(st.indices[:n].cpu(), torch.from_numpy(g.idx))
            ks, stride, pad, subm = F.LAYERS[layer]
            if subm:
                oi, oshape, n_out_dev, stride, pad = st.indices, list(g.shape), st.n_dev, (1, 1, 1), (1, 1, 1)
            else:
                oi, oshape, n_out_dev, _ = st.out_sites_ex(ks, stride, pad)
            n_out = int(n_out_dev.item())
            assert n_out == len(nbr) and torch.equal(oi[:n_out].cpu(), torch.from_numpy(out_idx)), f"{what}: output sites"
            tiles = st.rulebook(oi, oshape, ks, stride, pad, cin, cout, n_out_dev=n_out_dev)
            assert isinstance(tiles, ops.PairTiles)
            bx, xv = _poison_fill(n + pad_rows, cin)
            xv[:n] = torch.from_numpy(x).cuda()
            cap_out = int(oi.shape[0])
            bo, ov = _poison_fill(cap_out, cout)
            wd, scd, shd = dev(w), dev(sc), dev(sh)         # held: the kernel reads them after _capi.call returns
            _capi.call("heal_sp_conv_tiles", ops._ptr(xv), ops._ptr(tiles.buf), cap_out, tiles.slot_sites, cin, cout,
                       ops._ptr(ops.sp_weight_fragments(wd)), ops._ptr(scd), ops._ptr(shd), 1, ops._ptr(ov),
                       ops._ptr(n_out_dev), ops._stream())
            _check(ov[:n_out], ref, nbr, what)
            assert bool((ov[n_out:].view(torch.int32) == POISON).all()), f"{what}: a row behind the live count was written"
            _assert_poison_outside(bo, PAD, PAD + ov.numel(), what + " out")


# ================================================================================================ wrapper operand checks
def _operands(cin=16, cout=32, K=27):
    from heal_amd import ops
    g = F.counts(65)
    _, _, nbr = g.rules("subm")
    rng = np.random.default_rng(4)
    x = dev(F.features(rng, g.n, cin))
    st = ops.SparseTensor(x, dev(g.idx), g.shape, 1)
    w = dev(F.weights(rng, K, cin, cout))
    sc, sh = (dev(v) for v in F.batchnorm(rng, cout))
    return st, x, dev(nbr.astype(np.int32)), w, sc, sh


def test_operand_conv_rejects_int64_nbr():
    from heal_amd._capi import HealAmdError
    st, _, nb, w, sc, sh = _operands()
    with pytest.raises(HealAmdError, match="nbr"):
        st.conv(nb.long(), w, sc, sh)


def test_operand_conv_rejects_cpu_nbr():
    from heal_amd._capi import HealAmdError
    st, _, nb, w, sc, sh = _operands()
    with pytest.raises(HealAmdError, match="nbr"):
        st.conv(nb.cpu(), w, sc, sh)


def test_operand_conv_rejects_nbr_of_another_tap_count():
    from heal_amd._capi import HealAmdError
    st, _, nb, _, sc, sh = _operands()
    w3 = torch.ones((3, 16, 32), device="cuda")          # a 3-tap weight on a 27-tap table
    with pytest.raises(HealAmdError, match="nbr"):
        st.conv(nb, w3, sc, sh)


def test_operand_conv_rejects_features_of_another_width():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    st, _, nb, w, sc, sh = _operands()
    wide = ops.SparseTensor(torch.ones((st.n, 32), device="cuda"), st.indices, st.spatial_shape, 1)
    with pytest.raises(HealAmdError, match="features"):
        wide.conv(nb, w, sc, sh)


def test_operand_conv_rejects_bn_scale_length():
    from heal_amd._capi import HealAmdError
    st, _, nb, w, sc, sh = _operands()
    with pytest.raises(HealAmdError, match="bn_scale"):
        st.conv(nb, w, torch.cat([sc, sc]), sh)


def test_operand_conv_rejects_bn_shift_length():
    from heal_amd._capi import HealAmdError
    st, _, nb, w, sc, sh = _operands()
    with pytest.raises(HealAmdError, match="bn_shift"):
        st.conv(nb, w, sc, torch.cat([sh, sh]))


def test_operand_conv_pair_tiles_exempt_from_nbr_dtype():
    """PairTiles is a word buffer, not an int32 table: it passes the operand checks and gives the table's bits."""
    from heal_amd import ops
    g = F.counts(65)
    rng = np.random.default_rng(5)
    x = F.features(rng, g.n, 16)
    st = _sparse_input(g, x)
    tiles = st.rulebook(st.indices, g.shape, (3, 3, 3), (1, 1, 1), (1, 1, 1), 16, 32)
    assert isinstance(tiles, ops.PairTiles)
    w = dev(F.weights(rng, 27, 16, 32))
    sc, sh = (dev(v) for v in F.batchnorm(rng, 32))
    _, _, nbr = g.rules("subm")
    _check(st.conv(tiles, w, sc, sh), _ref(x, nbr, w.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy(), True), nbr, "tiles")


def test_operand_raw_rejects_int64_nbr():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    _, x, nb, w, _, _ = _operands()
    with pytest.raises(HealAmdError, match="nbr"):
        ops.sp_conv_raw(x, nb.long(), w)


def test_operand_raw_rejects_cpu_nbr():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    _, x, nb, w, _, _ = _operands()
    with pytest.raises(HealAmdError, match="nbr"):
        ops.sp_conv_raw(x, nb.cpu(), w)


def test_operand_raw_rejects_nbr_of_another_tap_count():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    _, x, nb, _, _, _ = _operands()
    with pytest.raises(HealAmdError, match="nbr"):
        ops.sp_conv_raw(x, nb, torch.ones((3, 16, 32), device="cuda"))


def test_operand_raw_rejects_features_of_another_width():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    _, x, nb, w, _, _ = _operands()
    with pytest.raises(HealAmdError, match="features"):
        ops.sp_conv_raw(torch.cat([x, x], 1), nb, w)


def test_operand_wgrad_rejects_grad_out_rows():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    _, x, nb, _, _, _ = _operands()
    g = torch.ones((nb.shape[0] + 5, 32), device="cuda")
    with pytest.raises(HealAmdError, match="grad_out"):
        ops.sp_wgrad(x, g, nb)
