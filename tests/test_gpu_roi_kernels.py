"""Per-image region-of-interest launches of the pointwise and the small-group 3x3 convolution (include/heal_amd_roi.h): a workgroup
whose output tile holds no pixel of its image's box writes nothing, every other tile is the plain launch's, bit for bit.  The output
is prefilled with NaN, so a skipped tile is still all NaN afterwards and a kept tile equals ops.conv1x1 / ops.grouped_conv3x3 on the
same inputs everywhere (also outside the box).  The tile rule is mirrored here from the header's text, not from the kernels."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _boxes(H, W, tx):
    """Boxes on an H x W output (H >= 4) whose conv1x1 tiles are tx pixels of a row: aligned to tile edges, off by one pixel on each
    side, one pixel, empty (two ways), the full image."""
    y0, y1 = 1, 3
    x0, x1 = (tx, min(W, 2 * tx)) if W >= 2 * tx else (0, W)
    aligned = (y0, y1, x0, x1)
    out = [aligned,
           (max(0, y0 - 1), min(H, y1 + 1), max(0, x0 - 1), min(W, x1 + 1)),          # one pixel more on each side
           (y0, y1 - 1, x0 + 1, x1 - 1),                                              # one pixel less
           (H // 2, H // 2 + 1, W // 3, W // 3 + 1),                                  # one pixel
           (2, 2, 0, W), (0, H, 5, 3),                                                # empty: the whole image is skipped
           (0, H, 0, W)]                                                              # full: the plain launch everywhere
    for b in out:
        assert 0 <= b[0] <= H and 0 <= b[1] <= H and 0 <= b[2] <= W and 0 <= b[3] <= W, b
    return out


def _in_box(H, W, box, device):
    m = torch.zeros((H, W), dtype=torch.bool, device=device)
    if box[1] > box[0] and box[3] > box[2]:
        m[box[0]:box[1], box[2]:box[3]] = True
    return m


def _c1_kept(H, W, box):
    """[H * W] bool: pixel lies in a KEPT 64-pixel tile of the flattened image (heal_amd_roi.h: a tile in one row is tested on rows and
    columns, a tile that spans rows on the rows it touches alone)."""
    y0, y1, x0, x1 = box
    kept = np.zeros(H * W, dtype=bool)
    for p0 in range(0, H * W, 64):
        pl = min(p0 + 64, H * W) - 1
        r0, r1 = p0 // W, pl // W
        k = y0 < y1 and x0 < x1 and r0 < y1 and r1 >= y0
        if k and r0 == r1:
            k = p0 - r0 * W < x1 and pl - r0 * W >= x0
        kept[p0:pl + 1] = k
    return kept


def _check(got, want, kept, inside):
    """got / want [C, H, W]; kept, inside [H, W] bool (device)."""
    assert torch.equal(got[:, inside], want[:, inside])                         # inside the ROI: the plain launch
    assert torch.equal(got[:, kept], want[:, kept])                             # kept tiles: the plain launch everywhere
    assert bool(torch.isnan(got[:, ~kept]).all())                               # skipped tiles: untouched
    assert bool((kept | ~inside).all())                                         # never skipped a tile that holds a box pixel


# ------------------------------------------------------------------------------------------------------------------ conv1x1
C1_SHAPES = [(8, 64, 1), (4, 128, 1), (6, 24, 1), (8, 128, 2)]                  # (H, W, stride): row tiles | half rows | spanning | stride 2


@pytest.mark.parametrize("epilogue", ["plain", "residual_relu", "gelu"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (40, 80)])
@pytest.mark.parametrize("H,W,stride", C1_SHAPES)
def test_conv1x1_roi(H, W, stride, cin, cout, epilogue):
    from heal_amd import ops
    g = torch.Generator().manual_seed(H * 1000 + W + cin)
    x = torch.randn((2, cin, H, W), generator=g).cuda()
    w = (torch.randn((cout, cin, 1, 1), generator=g) * 0.2).cuda()
    b = torch.randn((cout,), generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn((2, cout, Ho, Wo), generator=g).cuda() if epilogue == "residual_relu" else None
    act = {"plain": 0, "residual_relu": 1, "gelu": 3}[epilogue]
    want = ops.conv1x1(x, w, b, res, act, stride=stride)
    assert bool(torch.isfinite(want).all())
    full = (0, Ho, 0, Wo)
    for box in _boxes(Ho, Wo, 64 if Wo >= 64 else 8):
        for n in (2, 1):
            rois = [full, box][2 - n:]                                          # n = 2: image 0 the full box, image 1 the box
            out = torch.full((n, cout, Ho, Wo), NAN, device="cuda")
            got = ops.conv1x1(x[2 - n:], w, b, None if res is None else res[2 - n:], act, stride=stride, out=out, roi=rois)
            assert got.data_ptr() == out.data_ptr()
            for i, r in enumerate(rois):
                kept = torch.from_numpy(_c1_kept(Ho, Wo, r).reshape(Ho, Wo)).cuda()
                inside = _in_box(Ho, Wo, r, "cuda")
                _check(got[i], want[2 - n + i], kept, inside)
                if Wo % 64 == 0:                                                # row-segment tiles: the skip test is exact
                    tiles_in = inside.reshape(-1, 64).any(1)
                    assert torch.equal(tiles_in, kept.reshape(-1, 64).all(1))
            if box == full:
                assert torch.equal(got, want[2 - n:])


def test_conv1x1_roi_rejects_what_it_cannot_do():
    from heal_amd import _capi, ops
    x = torch.randn((1, 32, 8, 64)).cuda()
    w = torch.randn((64, 32, 1, 1)).cuda()
    y = torch.empty((1, 64, 8, 64), device="cuda")
    frag = ops.conv1x1_fragments(w)
    box = np.asarray([[0, 8, 0, 64]], dtype=np.int32)

    def call(pm, table, n=1):
        _capi.call("heal_conv1x1_roi", ops._ptr(x), ops._ptr(frag), None, None, None, n, 32, 64, 8, 64, 1, 0, pm,
                   ctypes.c_void_p(table.ctypes.data) if table is not None else None, ops._ptr(y), ops._stream())
    call(0, box)
    with pytest.raises(_capi.HealAmdError, match="NCHW output only"):
        call(1, box)                                                            # pixel-major
    with pytest.raises(_capi.HealAmdError, match="null ROI"):
        call(0, None)
    with pytest.raises(_capi.HealAmdError, match="outside the output map"):
        call(0, np.asarray([[0, 9, 0, 64]], dtype=np.int32))
    with pytest.raises(_capi.HealAmdError, match="`out` and `roi` are for the NCHW result"):
        ops.conv1x1(x, w, None, None, 0, pixel_major=True, roi=[(0, 8, 0, 64)])
    with pytest.raises(_capi.HealAmdError, match="one .* box for each"):
        ops.conv1x1(x, w, None, None, 0, roi=[(0, 8, 0, 64)] * 2)
    x9 = torch.randn((9, 32, 8, 64)).cuda()
    with pytest.raises(_capi.HealAmdError, match="at most 8"):
        ops.conv1x1(x9, w, None, None, 0, roi=[(0, 8, 0, 64)] * 9)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- grouped 3x3, small groups
@pytest.fixture
def nan_outputs(monkeypatch):
    """ops allocates the grouped convolution's result itself: hand out NaN-filled tensors instead of torch.empty ones."""
    from heal_amd import ops
    real = ops._out_or_empty
    monkeypatch.setattr(ops, "_out_or_empty", lambda out, shape, device, who: (
        real(out, shape, device, who) if out is not None else torch.full(tuple(shape), NAN, dtype=torch.float32, device=device)))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("H,W", [(32, 32), (16, 48)])
def test_grouped_small_conv3x3_roi(H, W, C, stride, nan_outputs):
    from heal_amd import ops
    cg = C // 32
    g = torch.Generator().manual_seed(C + H + stride)
    x = torch.randn((2, C, H, W), generator=g).cuda()
    w = (torch.randn((C, cg, 3, 3), generator=g) * 0.2).cuda()
    b = torch.randn((C,), generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    th, tw = (16 if cg == 4 and stride == 1 else 8), (32 if stride == 1 else 16)   # heal_amd_roi.h: the kernel's tiles
    want = ops.grouped_conv3x3(x, w, b, 32, stride, True)
    assert bool(torch.isfinite(want).all())
    full = (0, Ho, 0, Wo)
    a0, a1 = (8 if Ho > 8 else 0), min(Ho, 16)
    boxes = [(a0, a1, 0, 16), (a0, a1, min(16, Wo - 8), min(Wo, 32)),                                  # aligned to 16 / 8
             (max(0, a0 - 1), min(Ho, a1 + 1), 15, min(Wo, 33)), (a0 + 1, a1 - 1, min(17, Wo - 3), min(Wo, 31)),   # one pixel more / less
             (Ho // 2, Ho // 2 + 1, Wo - 1, Wo), (3, 3, 0, Wo), full]
    for box in boxes:
        assert 0 <= box[0] <= box[1] <= Ho and 0 <= box[2] <= box[3] <= Wo, box
        got = ops.grouped_conv3x3(x, w, b, 32, stride, True, roi=[full, box])
        for i, r in enumerate((full, box)):
            inside = _in_box(Ho, Wo, r, "cuda")
            tiles = inside.new_zeros((-(-Ho // th) * th, -(-Wo // tw) * tw))
            tiles[:Ho, :Wo] = inside
            kept = tiles.reshape(-(-Ho // th), th, -(-Wo // tw), tw).any(3).any(1)       # exact: a tile is kept iff it holds a box pixel
            kept = kept.repeat_interleave(th, 0).repeat_interleave(tw, 1)[:Ho, :Wo]
            _check(got[i], want[i], kept, inside)
        if box == full:
            assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------------------- captured graph
def test_roi_box_is_a_constant_of_a_captured_graph():
    """Captured once with a fixed box, replayed on two inputs: both equal the eager ROI launch -- the table lives in the kernel's
    arguments, nothing about it is read from memory that a later call could have changed."""
    from heal_amd import ops
    g = torch.Generator().manual_seed(3)
    w = (torch.randn((64, 32, 1, 1), generator=g) * 0.2).cuda()
    inputs = [torch.randn((2, 32, 8, 64), generator=g).cuda() for _ in range(2)]
    rois = [(0, 8, 0, 64), (2, 5, 10, 40)]
    eager = []
    for x in inputs:
        out = torch.full((2, 64, 8, 64), NAN, device="cuda")
        eager.append(ops.conv1x1(x, w, None, None, 1, out=out, roi=rois).clone())
    side = torch.cuda.Stream()
    xs, ys = torch.zeros_like(inputs[0]), torch.full((2, 64, 8, 64), NAN, device="cuda")
    with torch.cuda.stream(side):
        ops.conv1x1(xs, w, None, None, 1, out=ys, roi=rois)                     # warm-up outside the capture (weight fragments)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ops.conv1x1(xs, w, None, None, 1, out=ys, roi=rois)
        ops.conv1x1(xs, w, None, None, 0, out=torch.empty_like(ys), roi=[(0, 0, 0, 0)] * 2)   # another table in between
        for x, want in zip(inputs, eager):
            xs.copy_(x)
            ys.fill_(NAN)
            graph.replay()
            side.synchronize()
            assert torch.equal(torch.nan_to_num(ys, nan=-7.0), torch.nan_to_num(want, nan=-7.0))
            assert bool(torch.isnan(ys[1, :, 0:2]).all()) and bool(torch.isfinite(ys[1, :, 2:5]).all())
    torch.cuda.synchronize()
