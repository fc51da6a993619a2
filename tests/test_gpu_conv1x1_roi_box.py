"""The box rule of the pointwise convolution's region-of-interest launch (heal_conv1x1_box_roi, include/heal_amd_roi.h): the 64-pixel
tiles enumerate each image's ALIGNED box (its rows, its columns rounded outward to multiples of 4) instead of the image.  The output is
prefilled with NaN; afterwards it equals heal_conv1x1 on the same inputs bit for bit inside the aligned box and is still all NaN
outside it.  The aligned box is worked out here from the header's text (x0 // 4 * 4, ceil(x1 / 4) * 4); the host mirror of the tiles
(ops.conv1x1_box_tiles, what scripts/roi_tile_count.py counts) is checked against brute force on the CPU and against the same masks.

Shapes are the smallest at which the mapping can go wrong: a tile that is a row (8 x 64), half a row (4 x 128), tiles that span rows
with bw * bh no multiple of 64 (12 x 16, 6 x 20), and a width that is no multiple of 4, which keeps the tile rule.  For that last one
the 5 x 6 map cannot be launched at all -- stride 1 needs H * W % 4 == 0, stride 2 an output width % 4 == 0, for heal_conv1x1 as
well; the test below pins that -- so the fallback is exercised on 6 x 6.  An aligned box holds a multiple of 4 pixels: "exactly 64" is
one full tile, and a box of 65 pixels (1 x 65 on 4 x 128, 5 x 13 on 12 x 16) aligns to 68 / 80, one tile and the start of the next."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NAN = float("nan")


def _aligned(box, W):
    """(y0, y1, xa, xb) of the header's rule, or None for an empty box."""
    y0, y1, x0, x1 = box
    if y0 >= y1 or x0 >= x1:
        return None
    return y0, y1, x0 // 4 * 4, min(-(-x1 // 4) * 4, W)


def _mask(box, H, W):
    m = np.zeros((H, W), dtype=bool)
    a = _aligned(box, W)
    if a is not None:
        m[a[0]:a[1], a[2]:a[3]] = True
    return m


# --------------------------------------------------------------------------------------------------------- host mirror, no GPU
def test_box_tiles_cover_the_aligned_box_exactly_once():
    """Every box of an 8 x 16 map, the empty ones included: the tiles' pixels are those of the aligned box, each once, none outside;
    ceil(bw * bh / 64) tiles; every group of four lies in one row at a 16-byte boundary."""
    from heal_amd import ops
    H, W = 8, 16
    for y0, y1, x0, x1 in itertools.product(range(H + 1), range(H + 1), range(W + 1), range(W + 1)):
        tiles = ops.conv1x1_box_tiles((y0, y1, x0, x1), H, W)
        brute = sorted(y * W + x for y in range(y0, y1) for x in range(x0 // 4 * 4, -(-x1 // 4) * 4) if x0 < x1)
        px = tiles[tiles >= 0]
        assert px.tolist() == brute, (y0, y1, x0, x1)                     # row by row: the enumeration IS the sorted order
        assert tiles.shape == (-(-len(brute) // 64), 64)
        g = tiles.reshape(-1, 4)
        g = g[g[:, 0] >= 0]
        assert (g[:, 0] % 4 == 0).all() and (g[:, 1:] == g[:, :1] + np.arange(1, 4)).all() and (g[:, 3] // W == g[:, 0] // W).all()
    assert (ops.conv1x1_box_tiles((0, H, 0, W), H, W).reshape(-1) == np.arange(H * W)).all()      # the full box: the identity
    with pytest.raises(ValueError):
        ops.conv1x1_box_tiles((0, 5, 0, 6), 5, 6)


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _launch(name, x, frag, bias, res, n, cin, cout, Hin, Win, stride, act, y, table=None):
    from heal_amd import _capi, ops
    head = (ops._ptr(x), ops._ptr(frag), ops._ptr(bias), ops._ptr(res) if res is not None else None, None, n, cin, cout, Hin, Win,
            stride, act)
    if table is None:
        _capi.call(name, *head, 0, ops._ptr(y), ops._stream())
    else:
        _capi.call(name, *head, ctypes.c_void_p(table.ctypes.data), ops._ptr(y), ops._stream())


def _boxes(H, W):
    """Boxes on an H x W output map, H >= 4, W >= 6."""
    out = [(0, H, 0, W),                                                   # full: the plain launch
           (2, 2, 0, W), (0, H, 5, 3),                                     # empty, two ways
           (1, 2, 4, 8) if W >= 8 else (1, 2, 0, 4),                       # one 4-pixel group
           (1, 3, 3, 5), (0, H, W - 5, W - 3),                             # x0 % 4 == 3 and x1 % 4 == 1 (W % 4 == 0)
           (1, H - 1, 2, W - 2),                                           # one pixel inside every border
           (0, 2, 0, 3), (H - 2, H, W - 3, W), (0, H, 0, 1), (0, H, W - 1, W), (0, 1, 0, W), (H - 1, H, 0, W)]   # each border
    out += {(8, 64): [(3, 4, 0, 64), (3, 5, 1, 31)],                       # 64 aligned pixels: one row = one tile | 2 x 32
            (4, 128): [(1, 2, 64, 128), (1, 2, 1, 66), (0, 4, 60, 70)],    # 64 | 65 pixels -> 68 aligned | across the half-row seam
            (12, 16): [(4, 8, 0, 16), (2, 7, 1, 14), (0, 12, 5, 11)],      # 64 | 65 pixels -> 80 aligned | 12 x 8 = 96
            (6, 20): [(0, 4, 2, 15), (1, 6, 9, 19)]}.get((H, W), [])       # 4 x 16 = 64 | 5 x 12 = 60
    for b in out:
        assert 0 <= b[0] <= H and 0 <= b[1] <= H and 0 <= b[2] <= W and 0 <= b[3] <= W, b
    return out


def _run_case(H, W, stride, launches, cins=(32, 40, 96), couts=(64, 80), expect=_mask):
    """launches: lists of n boxes (one per image).  Every (Cin, Cout), with / without residual, ReLU on / off."""
    from heal_amd import ops
    n = len(launches[0])
    Hin, Win = (H, W) if stride == 1 else (2 * H - 1, 2 * W)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + stride)
    masks = {b: torch.from_numpy(expect(b, H, W)).cuda() for boxes in launches for b in boxes}
    for cin, cout in itertools.product(cins, couts):
        x = torch.randn((n, cin, Hin, Win), generator=g).cuda()
        w = (torch.randn((cout, cin, 1, 1), generator=g) * 0.2).cuda()
        bias = torch.randn((cout,), generator=g).cuda()
        resid = torch.randn((n, cout, H, W), generator=g).cuda()
        frag = ops.conv1x1_fragments(w)
        for res, act in itertools.product((None, resid), (0, 1)):
            want = torch.full((n, cout, H, W), NAN, device="cuda")
            _launch("heal_conv1x1", x, frag, bias, res, n, cin, cout, Hin, Win, stride, act, want)
            assert bool(torch.isfinite(want).all())
            for boxes in launches:
                got = torch.full((n, cout, H, W), NAN, device="cuda")
                table = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(n, 4))
                _launch("heal_conv1x1_box_roi", x, frag, bias, res, n, cin, cout, Hin, Win, stride, act, got, table)
                for i, b in enumerate(boxes):
                    m = masks[b]
                    assert torch.equal(got[i][:, m], want[i][:, m]), (b, i, cin, cout, res is not None, act)
                    assert bool(torch.isnan(got[i][:, ~m]).all()), (b, i, cin, cout, res is not None, act)
    torch.cuda.synchronize()


def _groups_of_3(boxes):
    """Every box in some launch of three different boxes; the windows overlap, so most boxes run at two image indices."""
    return [boxes[j:j + 3] for j in range(0, len(boxes) - 2, 2)] + [boxes[-3:]]


@gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(8, 64), (4, 128), (12, 16), (6, 20)])
def test_conv1x1_box_roi_writes_the_aligned_box_and_nothing_else(H, W, stride):
    from heal_amd import ops
    boxes = _boxes(H, W)
    for b in boxes:                                                        # the host mirror says what the masks say
        t = ops.conv1x1_box_tiles(b, H, W)
        m = np.zeros(H * W, dtype=bool)
        m[t[t >= 0]] = True
        assert (m.reshape(H, W) == _mask(b, H, W)).all() and int((t >= 0).sum()) == int(m.sum())
    launches = _groups_of_3(boxes)
    assert {b for l in launches for b in l} == set(boxes)
    _run_case(H, W, stride, launches)


@gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_conv1x1_box_roi_flagship_boxes(stride):
    """The last pyramid level of the flagship scene: three LiDAR agents with the full box, two camera agents with the first block's need
    box and with K5's read box, on 64 x 64."""
    full = (0, 64, 0, 64)
    _run_case(64, 64, stride, [[full, full, full, (10, 54, 9, 55), (17, 47, 16, 48)]], cins=(96,), couts=(80,))


def _tile_rule_mask(box, H, W):
    """An output width that is no multiple of 4 keeps heal_conv1x1_roi's tile rule (header): 64 consecutive pixels of the flattened
    image, kept when a row the tile touches lies in the box's rows (one row: its columns are tested too)."""
    y0, y1, x0, x1 = box
    kept = np.zeros(H * W, dtype=bool)
    for p0 in range(0, H * W, 64):
        pl = min(p0 + 64, H * W) - 1
        r0, r1 = p0 // W, pl // W
        k = y0 < y1 and x0 < x1 and r0 < y1 and r1 >= y0
        if k and r0 == r1:
            k = p0 - r0 * W < x1 and pl - r0 * W >= x0
        kept[p0:pl + 1] = k
    return kept.reshape(H, W)


@gpu
def test_conv1x1_box_roi_falls_back_to_the_tile_rule_when_the_width_is_no_multiple_of_4():
    from heal_amd import _capi, ops
    boxes = [(0, 6, 0, 6), (2, 2, 0, 6), (1, 2, 4, 6), (1, 3, 3, 5), (0, 2, 0, 3), (4, 6, 3, 6)]
    big = [(0, 12, 0, 14), (0, 0, 0, 0), (0, 5, 3, 9), (5, 6, 0, 1), (11, 12, 9, 14), (6, 10, 13, 14)]   # on 12 x 14: three tiles that span rows
    _run_case(6, 6, 1, [boxes[:3], boxes[3:]], cins=(40,), couts=(80,), expect=_tile_rule_mask)
    _run_case(12, 14, 1, [big[:3], big[3:]], cins=(40,), couts=(80,), expect=_tile_rule_mask)
    # 5 x 6 cannot be launched by any entry point of the pointwise convolution
    x, w = torch.randn((1, 32, 5, 6)).cuda(), torch.randn((64, 32, 1, 1)).cuda()
    y, frag, bias = torch.empty((1, 64, 5, 6), device="cuda"), ops.conv1x1_fragments(w), torch.zeros(64).cuda()
    table = np.asarray([[0, 5, 0, 6]], dtype=np.int32)
    for name, t in (("heal_conv1x1", None), ("heal_conv1x1_box_roi", table)):
        with pytest.raises(_capi.HealAmdError, match="multiple of 4"):
            _launch(name, x, frag, bias, None, 1, 32, 64, 5, 6, 1, 0, y, t)
    for name, t in (("heal_conv1x1", None), ("heal_conv1x1_box_roi", table)):
        with pytest.raises(_capi.HealAmdError, match="multiple of 4"):
            _launch(name, torch.randn((1, 32, 9, 11)).cuda(), frag, bias, None, 1, 32, 64, 9, 11, 2, 0, y, t)   # stride 2 -> 5 x 6
    torch.cuda.synchronize()
