"""The device-wide exclusive scan and the stable radix sort of csrc/prims.hip, alone, against numpy, exactly.

The two primitives decide which row every sparse site and every frustum point lands in, but the model path reaches them only
through their clients (sparse_conv.hip, bev_pool.hip), whose tests compare feature maps three kernels later and at sizes the clients
choose.  Here they run through their own entry points (include/heal_amd_ext.h: heal_scan_exclusive, heal_radix_sort_pairs) at the
sizes where a tiled scan or sort goes wrong.  Integer kernels: every comparison is np.array_equal / torch.equal, no tolerance.

  scan   reference np.cumsum in int64, shifted by one.  A scan tile is SCAN_TILE = 4096 elements (1024 threads x 4), a wave 64 threads
         = 256 elements; k_scan_final adds up the sums of the earlier tiles with a loop of stride 1024 that takes its second step
         at the 1025th tile, n = 1024 * 4096 + 1.
  sort   reference order = np.argsort(keys & mask, kind="stable"), mask = the low min(32, 9 * ceil(key_bits / 9)) bits (the contract
         stated in csrc/prims.h).  The values are the input indices, so sorted values == order IS stability; the sorted keys are
         keys[order] with all 32 bits.  A sort tile is SORT_TILE = 2048 pairs; the histogram of 512 * tiles words is scanned in place
         by the scan above and spans two scan tiles from 9 tiles = 16 385 pairs on.

Every operand, result and the workspace lies in the middle of a poisoned buffer with PAD guard words on each side (inside one
allocation, so an overrun lands in the guard, not in somebody else's memory); the workspace handed over is exactly what the size
query returned, so a scratch overrun by one word is seen."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0x7FBADBAD            # guard words, untouched outputs and the workspace's initial contents
PAD = 4096                     # poisoned words on each side of a region: 16 KiB
SCAN_TILE = 4096               # csrc/prims.h: SCAN_THREADS * SCAN_ITEMS
SORT_TILE = 2048               # csrc/prims.h: SORT_THREADS * SORT_ITEMS
RADIX_BITS = 9                 # csrc/prims.h: SORT_RADIX_BITS


def _capi():
    from heal_amd import _capi
    return _capi


def _guarded(n, values=None):
    """(backing buffer, view): an int32 region of n words in the middle of a poison-filled buffer, PAD poisoned words on each side.
    `values` (numpy, int32 or uint32, n elements) are copied in; without them the region itself is poison too."""
    buf = torch.full((PAD + n + PAD,), POISON, dtype=torch.int32, device="cuda")
    view = buf[PAD:PAD + n]
    if values is not None and n:
        assert values.shape == (n,) and values.dtype in (np.int32, np.uint32)
        view.copy_(torch.from_numpy(np.ascontiguousarray(values).view(np.int32)))
    return buf, view


def _p(buf):
    """Address of the region of a _guarded buffer (also where the region is empty)."""
    return ctypes.c_void_p(buf.data_ptr() + 4 * PAD)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _assert_guards(buf, n, what):
    """Every word of buf outside its region [PAD, PAD + n) still holds the poison pattern."""
    for part, name in ((buf[:PAD], "in front of"), (buf[PAD + n:], "behind")):
        bad = int((part != POISON).sum())
        assert bad == 0, f"{what}: {bad} guard words {name} the region were written"


def _assert_all_poison(view, what):
    bad = int((view != POISON).sum())
    assert bad == 0, f"{what}: {bad} of {view.numel()} words were written"


def _assert_same(got, want, what):
    """torch.equal of two device int32 vectors, with the first difference in the message."""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; first at {i} (tile {i // SCAN_TILE} + {i % SCAN_TILE}): "
                         f"got {int(got[i])} want {int(want[i])}")


# ================================================================================================ scan
SCAN_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257,         # a wave's 64 threads and its 256 elements
              4095, 4096, 4097,                            # one scan tile, and one element into a second
              8192, 3 * 4096 + 1,
              65 * 4096 + 7,                               # more earlier tiles than one wave of the tile-offset loop holds
              1024 * 4096 + 1]                             # 1025 tiles: the tile-offset loop's second step
SCAN_VALUES = ["rand0_7", "zeros", "ones", "signed"]


def _scan_values(kind, n):
    rng = np.random.default_rng(1000 + n % 9973 + 17 * SCAN_VALUES.index(kind))
    if kind == "rand0_7":
        return rng.integers(0, 8, n, dtype=np.int32)
    if kind == "zeros":
        return np.zeros(n, np.int32)
    if kind == "ones":
        return np.ones(n, np.int32)          # out[i] == i: a misplaced tile or wave is visible by its index
    return rng.integers(-3, 4, n, dtype=np.int32)


def _scan_reference(x):
    """(exclusive prefix sums, total) of x in int64, asserted to fit int32 at every prefix."""
    c = np.cumsum(x.astype(np.int64))
    total = int(c[-1]) if len(x) else 0
    assert -2 ** 31 <= total < 2 ** 31, total
    if len(x):
        assert -2 ** 31 <= int(c.min()) and int(c.max()) < 2 ** 31
    ref = np.concatenate([np.zeros(1, np.int64), c[:-1]]) if len(x) else np.zeros(0, np.int64)
    return ref.astype(np.int32), total


def _scan_once(x, in_place, with_total, what):
    """One guarded heal_scan_exclusive -> (out view, total or None).  Guards, the untouched input and an untouched `total` are checked."""
    capi = _capi()
    n = len(x)
    b_in, v_in = _guarded(n, x)
    b_out, v_out = (b_in, v_in) if in_place else _guarded(n)
    b_tot, v_tot = _guarded(1)
    need = capi.query("heal_scan_exclusive_workspace", n)
    assert need % 4 == 0 and need >= 4 * (math.ceil(n / SCAN_TILE))
    b_ws, _ = _guarded(need // 4)
    capi.call("heal_scan_exclusive", _p(b_in), _p(b_out), n, _p(b_tot) if with_total else None, _p(b_ws), need, _stream())
    torch.cuda.synchronize()
    for buf, words, name in ((b_in, n, "in"), (b_out, n, "out"), (b_tot, 1, "total"), (b_ws, need // 4, "workspace")):
        _assert_guards(buf, words, f"{what}: {name}")
    if not in_place and n:
        assert torch.equal(v_in, torch.from_numpy(x).cuda()), f"{what}: the input was changed"
    if not with_total:
        _assert_all_poison(v_tot, f"{what}: total (not passed)")
    return v_out, (int(v_tot[0]) if with_total else None)


def _check_scan(x, what):
    ref, total = _scan_reference(x)
    ref_dev = torch.from_numpy(ref).cuda()
    for in_place in (False, True):
        for with_total in (True, False):
            w = f"{what} {'in place' if in_place else 'out of place'}{', total' if with_total else ''}"
            out1, tot1 = _scan_once(x, in_place, with_total, w)
            _assert_same(out1, ref_dev, w)
            if with_total:
                assert tot1 == total, f"{w}: total {tot1}, want {total}"
            out2, tot2 = _scan_once(x, in_place, with_total, w + " (second launch)")
            assert torch.equal(out1, out2) and tot1 == tot2, f"{w}: two launches differ"


@pytest.mark.parametrize("kind", SCAN_VALUES)
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_exclusive_equals_cumsum(n, kind):
    _check_scan(_scan_values(kind, n), f"scan n={n} {kind}")


def test_scan_exclusive_total_just_under_2_pow_31():
    """4096 x 524 287: every prefix fits int32 and the total, 2 147 479 552, lies 4096 below 2^31 -- no intermediate sum (thread, wave,
    tile) may overflow on the way."""
    x = np.full(4096, 524287, np.int32)
    assert int(x.astype(np.int64).sum()) == 2147479552 < 2 ** 31
    _check_scan(x, "scan 4096 x 524287")


def test_scan_exclusive_of_nothing_writes_only_total():
    """n = 0: *total becomes 0 from a poisoned word, nothing else is written (the out buffer has no region: it stays poison whole)."""
    capi = _capi()
    need = capi.query("heal_scan_exclusive_workspace", 0)
    for with_total in (True, False):
        b_in, _ = _guarded(0)
        b_out, _ = _guarded(0)
        b_tot, v_tot = _guarded(1)
        b_ws, v_ws = _guarded(need // 4)
        capi.call("heal_scan_exclusive", _p(b_in), _p(b_out), 0, _p(b_tot) if with_total else None, _p(b_ws), need, _stream())
        torch.cuda.synchronize()
        assert int(v_tot[0]) == (0 if with_total else POISON)
        _assert_guards(b_tot, 1, "scan n=0: total")
        for buf, name in ((b_in, "in"), (b_out, "out")):
            _assert_all_poison(buf, f"scan n=0: {name}")
        _assert_guards(b_ws, need // 4, "scan n=0: workspace")
        _assert_all_poison(v_ws, "scan n=0: workspace")


def test_ops_scan_exclusive_agrees():
    from heal_amd import ops
    for n in (0, 1, 3 * 4096 + 1):
        x = _scan_values("signed", n)
        ref, total = _scan_reference(x)
        x_dev = torch.from_numpy(x).cuda()
        out, tot = ops.scan_exclusive(x_dev)
        assert np.array_equal(out.cpu().numpy(), ref) and int(tot[0]) == total and tot.dtype == torch.int32
        assert np.array_equal(x_dev.cpu().numpy(), x)
        only = ops.scan_exclusive(x_dev, want_total=False)
        assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), ref)
        same, tot = ops.scan_exclusive(x_dev, out=x_dev)                      # in place
        assert same is x_dev and np.array_equal(x_dev.cpu().numpy(), ref) and int(tot[0]) == total


# ================================================================================================ sort
SORT_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257,          # n <= 1 launches nothing; a wave's 64 lanes; one pass of a tile's 256 threads
              2047, 2048, 2049,                             # one sort tile, and one pair into a second
              4097,
              16385,                                        # 9 tiles: the histogram (4608 words) spans two scan tiles
              100003]
SORT_KEY_BITS = [1, 8, 9, 10, 18, 19, 27, 28, 32]
SORT_PASSES = {1: 1, 8: 1, 9: 1, 10: 2, 18: 2, 19: 3, 27: 3, 28: 4, 32: 4}


def _passes(key_bits):
    return -(-key_bits // RADIX_BITS)


def _compared_bits(key_bits):
    return min(32, RADIX_BITS * _passes(key_bits))


def _mask(bits):
    return np.uint32((1 << bits) - 1)


def _uniform(rng, n, bits):
    """n keys uniform below 2^bits (bits may be 0: all zero)."""
    return rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)


def _sort_once(keys, key_bits, what):
    """One guarded heal_radix_sort_pairs with vals = the input indices -> (sorted keys, sorted vals) as numpy uint32.  Checks the guard
    words of the four buffers and of the workspace, the returned buffer index and, for n <= 1, that nothing was written at all."""
    capi = _capi()
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    bk0, vk0 = _guarded(n, keys)
    bv0, vv0 = _guarded(n, vals)
    bk1, vk1 = _guarded(n)
    bv1, vv1 = _guarded(n)
    need = capi.query("heal_radix_sort_pairs_workspace", n)
    tiles = max(1, math.ceil(n / SORT_TILE))
    assert need % 4 == 0 and need >= 4 * (512 * tiles + math.ceil(512 * tiles / SCAN_TILE))
    b_ws, v_ws = _guarded(need // 4)
    which = ctypes.c_int(-1)
    capi.call("heal_radix_sort_pairs", _p(bk0), _p(bk1), _p(bv0), _p(bv1), n, key_bits, ctypes.byref(which), _p(b_ws), need, _stream())
    torch.cuda.synchronize()
    for buf, words, name in ((bk0, n, "keys0"), (bk1, n, "keys1"), (bv0, n, "vals0"), (bv1, n, "vals1"), (b_ws, need // 4, "workspace")):
        _assert_guards(buf, words, f"{what}: {name}")
    want = _passes(key_bits) % 2 if n > 1 else 0
    assert which.value == want, f"{what}: result in buffer {which.value}, want {want} ({_passes(key_bits)} passes)"
    if n <= 1:                                        # nothing is launched: buffer 0 is the result as it came, the rest untouched
        _assert_all_poison(vk1, f"{what}: keys1")
        _assert_all_poison(vv1, f"{what}: vals1")
        _assert_all_poison(v_ws, f"{what}: workspace")
    k, v = ((vk0, vv0), (vk1, vv1))[which.value]
    return k.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)


def _check_sort(keys, key_bits, what, order_keys=None):
    """The sort of `keys` equals the stable argsort of (order_keys or keys) under the compared-bits mask; two launches are bit-equal."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    assert _passes(key_bits) == SORT_PASSES[key_bits]
    by = (keys if order_keys is None else order_keys) & _mask(_compared_bits(key_bits))
    order = np.argsort(by, kind="stable")
    got_k, got_v = _sort_once(keys, key_bits, what)
    if not np.array_equal(got_v, order.astype(np.uint32)):
        i = int(np.flatnonzero(got_v != order)[0])
        raise AssertionError(f"{what}: values (input indices) differ from the stable order at {int((got_v != order).sum())} of {len(keys)} "
                             f"places; first at {i}: got {int(got_v[i])} want {int(order[i])}")
    assert np.array_equal(got_k, keys[order]), f"{what}: the keys did not travel with all 32 bits"
    again_k, again_v = _sort_once(keys, key_bits, what + " (second launch)")
    assert np.array_equal(again_k, got_k) and np.array_equal(again_v, got_v), f"{what}: two launches differ"
    return got_k, got_v


def _rng(*seed):
    return np.random.default_rng([2024, *seed])


@pytest.mark.parametrize("key_bits", [10, 28])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_radix_sort_pairs_every_size(n, key_bits):
    _check_sort(_uniform(_rng(n, key_bits), n, key_bits), key_bits, f"sort n={n} key_bits={key_bits}")


@pytest.mark.parametrize("n", [2049, 16385])
@pytest.mark.parametrize("key_bits", SORT_KEY_BITS)
def test_radix_sort_pairs_every_pass_count(key_bits, n):
    _check_sort(_uniform(_rng(n, key_bits), n, key_bits), key_bits, f"sort n={n} key_bits={key_bits}")


N_PAT = 4097                  # two full sort tiles and one pair: the key patterns


@pytest.mark.parametrize("key_bits", [10, 19, 32])
def test_radix_sort_pairs_all_keys_equal(key_bits):
    """One bin of every digit holds everything: the values come out as 0 .. n-1."""
    key = 0xA5A5A5A5 & int(_mask(key_bits))
    _, v = _check_sort(np.full(N_PAT, key, np.uint32), key_bits, f"sort all-equal key_bits={key_bits}")
    assert np.array_equal(v, np.arange(N_PAT, dtype=np.uint32))


@pytest.mark.parametrize("key_bits", [1, 10, 28])
def test_radix_sort_pairs_two_distinct_keys(key_bits):
    hi = int(_mask(key_bits))
    lo = hi >> 1 if key_bits > 1 else 0
    pick = _rng(key_bits).integers(0, 2, N_PAT).astype(bool)
    _, v = _check_sort(np.where(pick, hi, lo).astype(np.uint32), key_bits, f"sort two keys key_bits={key_bits}")
    assert np.array_equal(v, np.concatenate([np.flatnonzero(~pick), np.flatnonzero(pick)]).astype(np.uint32))


@pytest.mark.parametrize("key_bits", [18, 32])
def test_radix_sort_pairs_strictly_descending(key_bits):
    """Every pair moves: the result is the reversal."""
    i = np.arange(N_PAT, dtype=np.int64)
    keys = (N_PAT - 1 - i) if key_bits == 18 else (0xFFFFFFFF - i * 1048573)
    assert int(keys.min()) >= 0
    keys = keys.astype(np.uint32)
    assert int(keys.max()) <= int(_mask(key_bits)) and bool((np.diff(keys.astype(np.int64)) < 0).all())
    k, v = _check_sort(keys, key_bits, f"sort descending key_bits={key_bits}")
    assert np.array_equal(v, np.arange(N_PAT - 1, -1, -1, dtype=np.uint32)) and np.array_equal(k, keys[::-1])


@pytest.mark.parametrize("key_bits", [9, 27, 32])
def test_radix_sort_pairs_digits_0_and_511(key_bits):
    """Every 9-bit digit is 0 or 511 (the top digit of a 32-bit key: 0 or 31): only the first and the last bin of a pass are used."""
    rng = _rng(511, key_bits)
    keys = np.zeros(N_PAT, np.uint64)
    for p in range(_passes(key_bits)):
        keys |= (rng.integers(0, 2, N_PAT).astype(np.uint64) * np.uint64(511)) << np.uint64(RADIX_BITS * p)
    keys = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert int(keys.max()) <= int(_mask(key_bits))
    _check_sort(keys, key_bits, f"sort digits 0/511 key_bits={key_bits}")


def test_radix_sort_pairs_padding_stays_behind_real_keys():
    """The sparse convolution's case (sparse_conv.hip: 0xFFFFFFFF padding behind the real keys of a capacity-sized buffer, sorted
    with key_bits = 18): under the 18-bit mask the padding EQUALS a real key 2^18 - 1, and only stability keeps it behind."""
    key_bits, real = 18, 3001
    keys = _uniform(_rng(18), N_PAT, key_bits)
    keys[_rng(19).integers(0, real, 40)] = (1 << key_bits) - 1
    keys[real:] = 0xFFFFFFFF
    assert int((keys[:real] == (1 << key_bits) - 1).sum()) >= 20
    k, v = _check_sort(keys, key_bits, "sort with 0xFFFFFFFF padding")
    assert bool((k[:real] != 0xFFFFFFFF).all()) and bool((k[real:] == 0xFFFFFFFF).all())
    assert np.array_equal(v[real:], np.arange(real, N_PAT, dtype=np.uint32))
    assert bool((np.diff(k[:real].astype(np.int64)) >= 0).all())


@pytest.mark.parametrize("key_bits", [1, 8, 9, 10, 18, 19, 27])
def test_radix_sort_pairs_ignores_bits_above_the_last_digit(key_bits):
    """Random bits above 9 * ceil(key_bits / 9) do not influence the order (it is the order of the keys without them) and come out
    unchanged."""
    top = _compared_bits(key_bits)
    assert top < 32
    base = _uniform(_rng(1, key_bits), N_PAT, key_bits)
    noise = _uniform(_rng(2, key_bits), N_PAT, 32 - top) << np.uint32(top)
    assert int(noise.max()) > int(_mask(top))
    _check_sort(base | noise, key_bits, f"sort noise above bit {top} key_bits={key_bits}", order_keys=base)


@pytest.mark.parametrize("key_bits", [1, 8, 10, 19, 28])
def test_radix_sort_pairs_orders_by_the_whole_last_digit(key_bits):
    """Random bits between key_bits and 9 * ceil(key_bits / 9) DO take part: the last digit is a full digit (csrc/prims.h states it;
    this pins it).  The order is that of the keys with those bits, and differs from the order without them."""
    top = _compared_bits(key_bits)
    assert top > key_bits
    base = _uniform(_rng(3, key_bits), N_PAT, key_bits)
    keys = base | (_uniform(_rng(4, key_bits), N_PAT, top - key_bits) << np.uint32(key_bits))
    assert not np.array_equal(np.argsort(keys, kind="stable"), np.argsort(base, kind="stable"))
    _check_sort(keys, key_bits, f"sort bits {key_bits}..{top} key_bits={key_bits}")


def test_ops_radix_sort_pairs_agrees():
    from heal_amd import ops
    for n, key_bits in ((0, 10), (1, 10), (4097, 19), (4097, 28)):
        keys = _uniform(_rng(7, n, key_bits), n, key_bits)
        vals = _uniform(_rng(8, n), n, 32)
        order = np.argsort(keys & _mask(_compared_bits(key_bits)), kind="stable")
        k_dev, v_dev = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
        k, v = ops.radix_sort_pairs(k_dev, v_dev, key_bits)
        assert k.dtype == torch.int32 and tuple(k.shape) == (n,) and tuple(v.shape) == (n,)
        assert np.array_equal(k.cpu().numpy().view(np.uint32), keys[order])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), vals[order])
        assert np.array_equal(k_dev.cpu().numpy().view(np.uint32), keys) and np.array_equal(v_dev.cpu().numpy().view(np.uint32), vals)


# ================================================================================================ capture and replay
def test_sort_and_scan_replay_from_a_captured_graph():
    """The clients run inside captured graphs: one sort (n = 16 385, key_bits = 19: three passes, a histogram over two scan tiles) and
    one scan with its total, captured on a side stream after a warm-up call (the workspace exists), replayed on two inputs each."""
    from heal_amd import ops
    n, key_bits = 16385, 19
    key_sets = [_uniform(_rng(31, i), n, key_bits) for i in range(3)]                      # [0]: warm-up and capture
    scan_sets = [_rng(32, i).integers(-3, 4, 3 * 4096 + 1, dtype=np.int32) for i in range(3)]
    as_dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        keys = as_dev(key_sets[0])
        x = as_dev(scan_sets[0])
        ops.radix_sort_pairs(keys, vals, key_bits)
        ops.scan_exclusive(x)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            k, v = ops.radix_sort_pairs(keys, vals, key_bits)
            out, total = ops.scan_exclusive(x)
        for ks, xs in zip(key_sets[1:], scan_sets[1:]):
            keys.copy_(as_dev(ks))
            x.copy_(as_dev(xs))
            graph.replay()
            st.synchronize()
            order = np.argsort(ks & _mask(_compared_bits(key_bits)), kind="stable")
            assert np.array_equal(v.cpu().numpy().view(np.uint32), order.astype(np.uint32))
            assert np.array_equal(k.cpu().numpy().view(np.uint32), ks[order])
            ref, tot = _scan_reference(xs)
            assert np.array_equal(out.cpu().numpy(), ref) and int(total[0]) == tot
            ek, ev = ops.radix_sort_pairs(keys, vals, key_bits)                            # eager, same stream and workspace
            eo, et = ops.scan_exclusive(x)
            assert torch.equal(ek, k) and torch.equal(ev, v) and torch.equal(eo, out) and torch.equal(et, total)
            assert np.array_equal(keys.cpu().numpy().view(np.uint32), ks)                  # the replay left its inputs alone
    torch.cuda.current_stream().wait_stream(st)


# ================================================================================================ refusals
def test_scan_exclusive_refuses_before_any_launch():
    capi = _capi()
    n = 5000
    need = capi.query("heal_scan_exclusive_workspace", n)
    b_in, _ = _guarded(n, np.ones(n, np.int32))
    b_out, _ = _guarded(n)
    b_tot, _ = _guarded(1)
    b_ws, _ = _guarded(need // 4)
    good = dict(inp=_p(b_in), out=_p(b_out), n=n, ws=_p(b_ws), bytes=need)
    cases = {"negative n": dict(n=-1), "null in": dict(inp=None), "null out": dict(out=None), "null workspace": dict(ws=None),
             "small workspace": dict(bytes=need - 4), "no workspace bytes": dict(bytes=0)}
    for name, change in cases.items():
        a = dict(good, **change)
        with pytest.raises(capi.HealAmdError, match="heal_scan_exclusive"):
            capi.call("heal_scan_exclusive", a["inp"], a["out"], a["n"], _p(b_tot), a["ws"], a["bytes"], _stream())
        torch.cuda.synchronize()
        for buf, what in ((b_out, "out"), (b_tot, "total"), (b_ws, "workspace")):
            _assert_all_poison(buf, f"scan refusal ({name}): {what}")


def test_radix_sort_pairs_refuses_before_any_launch():
    capi = _capi()
    n = 5000
    need = capi.query("heal_radix_sort_pairs_workspace", n)
    keys = _uniform(_rng(41), n, 18)
    bk0, vk0 = _guarded(n, keys)
    bv0, vv0 = _guarded(n, np.arange(n, dtype=np.uint32))
    bk1, _ = _guarded(n)
    bv1, _ = _guarded(n)
    b_ws, _ = _guarded(need // 4)
    which = ctypes.c_int(-1)
    good = dict(k0=_p(bk0), k1=_p(bk1), v0=_p(bv0), v1=_p(bv1), n=n, bits=18, res=ctypes.byref(which), ws=_p(b_ws), bytes=need)
    cases = {"key_bits 0": dict(bits=0), "key_bits 33": dict(bits=33), "key_bits -1": dict(bits=-1), "negative n": dict(n=-1),
             "null keys0": dict(k0=None), "null keys1": dict(k1=None), "null vals0": dict(v0=None), "null vals1": dict(v1=None),
             "null result_buf": dict(res=None), "null workspace": dict(ws=None), "small workspace": dict(bytes=need - 4)}
    for name, change in cases.items():
        a = dict(good, **change)
        with pytest.raises(capi.HealAmdError, match="heal_radix_sort_pairs"):
            capi.call("heal_radix_sort_pairs", a["k0"], a["k1"], a["v0"], a["v1"], a["n"], a["bits"], a["res"], a["ws"], a["bytes"],
                      _stream())
        torch.cuda.synchronize()
        assert which.value == -1, name
        for buf, what in ((bk1, "keys1"), (bv1, "vals1"), (b_ws, "workspace")):
            _assert_all_poison(buf, f"sort refusal ({name}): {what}")
        assert np.array_equal(vk0.cpu().numpy().view(np.uint32), keys) and np.array_equal(vv0.cpu().numpy(), np.arange(n)), name
        for buf, what in ((bk0, "keys0"), (bv0, "vals0")):
            _assert_guards(buf, n, f"sort refusal ({name}): {what}")
