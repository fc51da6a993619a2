"""heal_deconv3x3_s2 and heal_ssfa_blend on the device against the fp64 references of tests/ssfa_refs.py, their refusals,
repeatability and capture, SSFA against the reference's recording (tests/golden/gen_golden_ssfa.py) both ways of HEAL_SSFA_FUSED, and
SecondSSFA / SecondSSFAUncertainty end to end through their post-processors.

Measured on an MI355X (max abs error against the fp64 reference; the bound of a kernel is twice the fp32 torch composition's own
error on the same inputs, same GPU) -- DESIGN.md section 27 carries the same figures:
  deconvolution, randn, (2, 256, 256, 6, 33), largest magnitude 125.8:   kernel 3.227e-05, F.conv_transpose2d + bias + ReLU 6.740e-05
  blend, randn (kernel / torch):   (1,64,1,4)      out 2.031e-07 / 1.797e-07   pa 4.405e-08 / 4.405e-08
                                   (2,128,3,4)     out 2.913e-07 / 5.851e-07   pa 5.470e-08 / 1.658e-07
                                   (1,128,5,12)    out 3.576e-07 / 6.100e-07   pa 7.531e-08 / 1.303e-07
                                   (2,128,100,352) out 8.854e-07 / 2.031e-06   pa 1.707e-07 / 4.343e-07

pa == 0 exactly cannot hold at ba = -40: 1 / (1 + exp(40)) is 4.25e-18 in fp32 (exp(40) is finite), in the kernel's formula and in
torch's softmax alike.  What holds exactly there is 1 - pa == 1 and out == b, and that is asserted; pa == 0 exactly is asserted at
ba = -200, where exp overflows to +inf.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, configs, ops
from heal_amd.opencood.models.sub_modules.cia_ssd_utils import SSFA
from tests import ssfa_refs
from tests.golden.detfill import fill_module

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-3                 # the project's bound for fp32 features, of the largest magnitude
DECONV_SHAPES = [(1, 64, 64, 1, 1), (1, 64, 64, 1, 7), (2, 64, 128, 3, 5), (1, 128, 64, 17, 9), (2, 256, 256, 6, 33),
                 (1, 256, 256, 50, 176)]
BLEND_SHAPES = [(1, 64, 1, 4), (2, 128, 3, 4), (1, 128, 5, 12), (2, 128, 100, 352)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ssfa_small.npz"))


def rel(got, want):
    return float(np.abs(got.detach().cpu().numpy() - want).max()) / float(np.abs(want).max())


# ---------------------------------------------------------------------------------------------------- deconvolution, integer data
@functools.lru_cache(maxsize=None)
def _int_case(shape):
    """Integer operands (every partial sum far below 2^24: the fp32 result is exact) and the fp64 scatter reference's linear part,
    computed once per shape and shared by the variants."""
    n, cin, cout, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-3, 4, (n, cin, H, W), generator=g).float()
    w = torch.randint(-2, 3, (cin, cout, 3, 3), generator=g).float()
    bias = torch.randint(-4, 5, (cout,), generator=g).float()
    res = torch.randint(-8, 9, (n, cout, 2 * H, 2 * W), generator=g).float()
    linear = ssfa_refs.deconv3x3_s2_linear(x.numpy(), w.numpy())
    linear.setflags(write=False)
    return x.cuda(), w.cuda(), bias.cuda(), res.cuda(), linear


@pytest.mark.parametrize("shape", DECONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [False, True])
def test_deconv_is_exact_on_integer_data(shape, relu):
    x, w, bias, res, linear = _int_case(shape)
    cout = shape[2]
    xn, wn, bn, rn = (t.cpu().numpy() for t in (x, w, bias, res))
    plain = ops.deconv3x3_s2(x, w, bias, relu=relu)
    for name, r in (("none", None), ("all", res), ("half", res[:, :cout // 2].contiguous())):
        got = plain if r is None else ops.deconv3x3_s2(x, w, bias, relu=relu, residual=r)
        want = ssfa_refs.deconv3x3_s2(xn, wn, bn, relu, None if r is None else r.cpu().numpy(), linear=linear)
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        assert np.array_equal(got[:, :, -1, :], want[:, :, -1, :]), (name, "last output row")
        assert np.array_equal(got[:, :, :, -1], want[:, :, :, -1]), (name, "last output column")
        assert np.array_equal(got, want), name
        if name == "half":      # the channels the residual does not cover are the plain result, bit for bit
            assert np.array_equal(got[:, cout // 2:], plain[:, cout // 2:].cpu().numpy().astype(np.float64))
            assert not np.array_equal(got[:, :cout // 2], plain[:, :cout // 2].cpu().numpy().astype(np.float64))


def test_deconv_fragments_and_weight_give_the_same_result():
    x, w, bias, res, _ = _int_case(DECONV_SHAPES[2])
    assert torch.equal(ops.deconv3x3_s2(x, ops.deconv3x3_s2_fragments(w), bias), ops.deconv3x3_s2(x, w, bias))
    assert torch.equal(ops.deconv3x3_s2(x, w, None, relu=False), ops.deconv3x3_s2(x, w, torch.zeros_like(bias), relu=False))


# ------------------------------------------------------------------------------------------------------ deconvolution, float data
def test_deconv_float_error_against_the_library():
    n, cin, cout, H, W = 2, 256, 256, 6, 33
    g = torch.Generator().manual_seed(7)
    x, w, bias = (torch.randn(s, generator=g) for s in ((n, cin, H, W), (cin, cout, 3, 3), (cout,)))
    want = ssfa_refs.deconv3x3_s2(x.numpy(), w.numpy(), bias.numpy(), True)
    got = ops.deconv3x3_s2(x.cuda(), w.cuda(), bias.cuda(), relu=True).cpu().numpy()
    lib = F.relu(F.conv_transpose2d(x.cuda(), w.cuda(), bias.cuda(), stride=2, padding=1, output_padding=1)).cpu().numpy()
    err, err_lib = float(np.abs(got - want).max()), float(np.abs(lib - want).max())
    print(f"deconv3x3_s2 randn {n}x{cin}x{cout}x{H}x{W}: kernel {err:.3e}, F.conv_transpose2d + bias + ReLU {err_lib:.3e} "
          f"(max abs error against fp64, largest magnitude {float(np.abs(want).max()):.1f})")
    assert err <= 2 * err_lib


# ------------------------------------------------------------------------------------------------------------------------- blend
def _blend_inputs(shape, seed=0):
    n, C, H, W = shape
    g = torch.Generator().manual_seed(100 + seed + n * C * H * W)
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    wa, wb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return a, b, wa, wb


@pytest.mark.parametrize("shape", BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_saturated_and_balanced(shape):
    a, b, wa, _ = _blend_inputs(shape)
    # randn draws an exact 0.0 now and then (twice among the 9 M values of the largest shape).  Where pa is tiny but not 0 the blend
    # of such an element is a pa, not b: out == b bit for bit needs |a| pa below half an ulp of b, which |b| >= 2^-20 guarantees
    b = torch.where(b.abs() < 2.0 ** -20, torch.ones_like(b), b)
    a, b, wa = a.cuda(), b.cuda(), wa.cuda()
    zero = torch.zeros_like(wa)
    out, pa = ops.ssfa_blend(a, b, zero, 40.0, zero, 0.0, want_weights=True)
    assert tuple(pa.shape) == (shape[0], 1, shape[2], shape[3])
    assert bool((pa == 1.0).all()) and torch.equal(out, a)
    out, pa = ops.ssfa_blend(a, b, zero, -40.0, zero, 0.0, want_weights=True)       # exp(40) is finite: pa = 4.25e-18, 1 - pa == 1
    assert bool((pa < 2.0 ** -56).all()) and bool(((1.0 - pa) == 1.0).all()) and torch.equal(out, b)
    out, pa = ops.ssfa_blend(a, b, zero, -200.0, zero, 0.0, want_weights=True)      # exp(200) = +inf: pa is 0
    assert bool((pa == 0.0).all()) and torch.equal(out, b)
    out, pa = ops.ssfa_blend(a, b, zero, 200.0, zero, 0.0, want_weights=True)
    assert bool((pa == 1.0).all()) and torch.equal(out, a)
    out, pa = ops.ssfa_blend(a, a.clone(), wa, 0.25, wa.clone(), 0.25, want_weights=True)
    assert bool((pa == 0.5).all()) and torch.equal(out, a)
    assert torch.equal(ops.ssfa_blend(a, b, wa, torch.tensor([0.5]).cuda(), zero, torch.tensor([-0.5]).cuda()),
                       ops.ssfa_blend(a, b, wa, 0.5, zero, -0.5))


@pytest.mark.parametrize("shape", BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_error_against_the_torch_composition(shape):
    a, b, wa, wb = _blend_inputs(shape, seed=1)
    C = shape[1]
    wa, wb = wa / C ** 0.5, wb / C ** 0.5                    # logits of unit scale: the softmax is not saturated
    ba, bb = 0.375, -0.25
    want, want_pa = ssfa_refs.ssfa_blend(a.numpy(), b.numpy(), wa.numpy(), ba, wb.numpy(), bb)
    a, b, wa, wb = a.cuda(), b.cuda(), wa.cuda(), wb.cuda()
    out, pa = ops.ssfa_blend(a, b, wa, ba, wb, bb, want_weights=True)
    s = torch.softmax(torch.cat([F.conv2d(a, wa.view(1, C, 1, 1)) + ba, F.conv2d(b, wb.view(1, C, 1, 1)) + bb], dim=1), dim=1)
    lib = a * s[:, 0:1] + b * s[:, 1:]
    e_out, e_pa = float(np.abs(out.cpu().numpy() - want).max()), float(np.abs(pa.cpu().numpy() - want_pa).max())
    l_out, l_pa = float(np.abs(lib.cpu().numpy() - want).max()), float(np.abs(s[:, 0:1].cpu().numpy() - want_pa).max())
    print(f"ssfa_blend randn {shape}: out kernel {e_out:.3e} torch {l_out:.3e}; pa kernel {e_pa:.3e} torch {l_pa:.3e} "
          "(max abs error against fp64)")
    assert e_out <= 2 * l_out and e_pa <= 2 * l_pa


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_from_host_validation_and_launch_nothing():
    calls = dict(ops.SSFA_CALLS)
    x, w = torch.zeros(1, 64, 3, 5).cuda(), torch.zeros(64, 64, 3, 3).cuda()
    with pytest.raises(_capi.HealAmdError, match="unsupported"):
        ops.deconv3x3_s2(torch.zeros(1, 48, 3, 5).cuda(), torch.zeros(48, 64, 3, 3).cuda())
    with pytest.raises(_capi.HealAmdError, match="unsupported"):
        ops.deconv3x3_s2(x, torch.zeros(64, 48, 3, 3).cuda())
    with pytest.raises(_capi.HealAmdError, match="does not fit"):
        ops.deconv3x3_s2(x, torch.zeros(128, 64, 3, 3).cuda())
    for bad in ((1, 64, 6, 9), (1, 96, 6, 10), (2, 64, 6, 10), (1, 64, 3, 5)):
        with pytest.raises(_capi.HealAmdError, match="residual"):
            ops.deconv3x3_s2(x, w, residual=torch.zeros(bad).cuda())
    off = torch.zeros(64 * 15 + 1).cuda()[1:].view(1, 64, 3, 5)               # contiguous, 4 bytes past a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(_capi.HealAmdError, match="16-byte aligned"):
        ops.deconv3x3_s2(off, w)
    with pytest.raises(_capi.HealAmdError, match="unsupported"):               # the C entry point refuses too, before any launch
        _capi.call("heal_deconv3x3_s2", ops._ptr(x), ops._ptr(w), None, None, 0, 1, 48, 64, 3, 5, 1, ops._ptr(x), ops._stream())
    a = torch.zeros(1, 128, 3, 4).cuda()
    wa = torch.zeros(128).cuda()
    with pytest.raises(_capi.HealAmdError, match="unsupported"):
        ops.ssfa_blend(torch.zeros(1, 32, 3, 4).cuda(), torch.zeros(1, 32, 3, 4).cuda(), wa[:32], 0.0, wa[:32], 0.0)
    with pytest.raises(_capi.HealAmdError, match="unsupported"):
        ops.ssfa_blend(a[:, :, :, :3], a[:, :, :, :3], wa, 0.0, wa, 0.0)       # 9 pixels: rows are not 16-byte pieces
    with pytest.raises(_capi.HealAmdError, match="one shape"):
        ops.ssfa_blend(a, torch.zeros(1, 128, 4, 3).cuda(), wa, 0.0, wa, 0.0)
    with pytest.raises(_capi.HealAmdError, match="must hold 128"):
        ops.ssfa_blend(a, a, wa[:64], 0.0, wa, 0.0)
    off = torch.zeros(128 * 12 + 1).cuda()[1:].view(1, 128, 3, 4)
    with pytest.raises(_capi.HealAmdError, match="16-byte aligned"):
        ops.ssfa_blend(off, a, wa, 0.0, wa, 0.0)
    torch.cuda.synchronize()
    assert ops.SSFA_CALLS == calls


# ------------------------------------------------------------------------------------------------------ repeatability and capture
def test_kernels_are_bit_equal_across_launches():
    g = torch.Generator().manual_seed(9)
    x, w, bias = (torch.randn(s, generator=g).cuda() for s in ((2, 256, 6, 33), (256, 256, 3, 3), (256,)))
    res = torch.randn((2, 128, 12, 66), generator=g).cuda()
    assert torch.equal(ops.deconv3x3_s2(x, w, bias, residual=res), ops.deconv3x3_s2(x, w, bias, residual=res))
    a, b, wa, wb = (t.cuda() for t in _blend_inputs((2, 128, 100, 352), seed=2))
    first, second = ops.ssfa_blend(a, b, wa, 0.1, wb, 0.2, want_weights=True), ops.ssfa_blend(a, b, wa, 0.1, wb, 0.2, want_weights=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def _ssfa(gold):
    head = "ssfa/sd/"
    model = SSFA({"feature_num": 128}).eval()
    model.load_state_dict({k[len(head):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(head)}, strict=True)
    return model.cuda()


def test_ssfa_graph_replay_equals_eager(gold, monkeypatch):
    """One capture on one stream, replayed twice on fresh inputs; 16 x 16 so that every layer runs on this library's kernels."""
    monkeypatch.delenv("HEAL_SSFA_FUSED", raising=False)
    model = _ssfa(gold)
    gen = torch.Generator().manual_seed(5)
    inputs = [torch.randn((1, 128, 16, 16), generator=gen).cuda() for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static_x = inputs[0].clone()
        for _ in range(2):
            model(static_x)              # weight-derived tensors and workspaces exist before the capture
        side.synchronize()
        calls = dict(ops.SSFA_CALLS)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_y = model(static_x)
        assert ops.SSFA_CALLS == {"deconv": calls["deconv"] + 1, "blend": calls["blend"] + 1}
        for xi in inputs:
            static_x.copy_(xi)
            graph.replay()
            side.synchronize()
            assert torch.equal(static_y, model(xi))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("fused", [True, False])
def test_ssfa_reproduces_the_reference_recording(gold, monkeypatch, fused):
    if fused:
        monkeypatch.delenv("HEAL_SSFA_FUSED", raising=False)
    else:
        monkeypatch.setenv("HEAL_SSFA_FUSED", "0")
    model = _ssfa(gold)
    calls = dict(ops.SSFA_CALLS)
    got = model(torch.from_numpy(gold["input"]).cuda())
    err = rel(got, gold["output"])
    print(f"SSFA {'fused' if fused else 'HEAL_SSFA_FUSED=0'}: {err:.3e} of the largest magnitude")
    assert got.shape == gold["output"].shape and err <= RTOL
    step = 1 if fused else 0                                  # the kernel path was the one taken (or not)
    assert ops.SSFA_CALLS == {"deconv": calls["deconv"] + step, "blend": calls["blend"] + step}


@functools.lru_cache(maxsize=None)
def _cloud():
    from heal_amd import synth
    rng_range = [-6.4, -6.4, -3, 6.4, 6.4, 1]
    p = torch.from_numpy(synth.lidar_frame(90)).cuda()
    p = p[(p[:, 0].abs() < 6.4) & (p[:, 1].abs() < 6.4)].contiguous()
    v, c, n = ops.voxelize(p, rng_range, [0.1, 0.1, 0.1], 5, 70000, batch_idx=0)
    return rng_range, {"voxel_features": v, "voxel_coords": c, "voxel_num_points": n}


@pytest.mark.parametrize("dim", [None, 3], ids=["second_ssfa", "second_ssfa_uncertainty"])
def test_models_end_to_end_both_ways_of_the_switch(dim, monkeypatch):
    from heal_amd.opencood.data_utils.post_processor.uncertainty_voxel_postprocessor import UncertaintyVoxelPostprocessor
    from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    from heal_amd.opencood.tools.train_utils import create_model
    rng_range, lidar = _cloud()
    hypes = configs.second_ssfa(rng_range, dim)
    # the largest logits of a 16 x 16 map sit on its border (zero padding), where a box sticks out of the 12.8 m square: the range
    # filter at the end of post_process gets room, so that it keeps them (x and y only; the z interval is the config's)
    hypes["postprocess"]["gt_range"] = [-12.8, -12.8, -3, 12.8, 12.8, 1]
    # Anchors at the same distance from the map's border score alike to the last digit (measured: three boxes at 0.200211), and the
    # greedy NMS keeps whichever of two overlapping ones it meets first: the kept set then follows the paths' rounding -- the
    # composition's changes from one run to the next.  The NMS runs with a threshold no IoU exceeds, so every candidate is kept.
    hypes["postprocess"]["nms_thresh"] = 1.0
    model = fill_module(create_model(hypes)).cuda().eval()
    # Keep a few dozen candidates: with all 512 anchors above the score threshold the greedy NMS takes thousands of decisions on
    # scores that lie 1e-6 apart, and the rounding of the two paths (1e-6 too) reorders them.  The class bias is moved so that the
    # threshold falls into the widest gap between the 8th and the 32nd largest logit of the map.
    monkeypatch.setenv("HEAL_SSFA_FUSED", "1")
    # The filled (untrained) sparse trunk hands SSFA a map of magnitude 0.02, on which the class map is flat: its largest logits lie
    # 6e-8 apart and the paths' rounding decides their order.  SSFA's first convolution is scaled so that its input counts as O(1).
    seen = {}
    hook = model.ssfa.register_forward_hook(lambda mod, inp, res: seen.update(x=float(inp[0].abs().max())))
    model({"processed_lidar": dict(lidar)})
    hook.remove()
    model.ssfa.bottom_up_block_0[1].weight.data *= 1.0 / seen["x"]
    v = torch.sort(model({"processed_lidar": dict(lidar)})["cls_preds"].flatten(), descending=True)[0]
    k = 8 + int(torch.argmax(v[7:31] - v[8:32]))
    assert float(v[k - 1] - v[k]) > 1e-3
    cls_bias = (model.head.conv_cls if dim is None else model.cls_head).bias
    cls_bias.data += float(np.log(0.2 / 0.8)) - float(v[k - 1] + v[k]) / 2
    # and the regression head is turned down: with O(1) deltas of a filled (untrained) head the decoded boxes are e^delta times the
    # anchor's size and the size / height filters remove every one of them
    reg_head = model.head.conv_box if dim is None else model.reg_head
    reg_head.weight.data *= 0.05
    reg_head.bias.data *= 0.05
    # and the direction head prefers bin 0 clearly: the two bin logits of a filled head are nearly equal in places, where the paths'
    # rounding picks the bin and turns a box by pi (same footprint, corners in another order)
    dir_head = model.head.conv_dir if dim is None else model.dir_head
    dir_head.bias.data[0::2] += 5.0
    post = (VoxelPostprocessor if dim is None else UncertaintyVoxelPostprocessor)(hypes["postprocess"], train=False)
    batch = {"ego": {"transformation_matrix": torch.eye(4), "anchor_box": torch.from_numpy(post.generate_anchor_box())}}
    results = []
    for value in ("1", "0"):
        monkeypatch.setenv("HEAL_SSFA_FUSED", value)
        calls = dict(ops.SSFA_CALLS)
        out = model({"processed_lidar": dict(lidar)})
        assert (ops.SSFA_CALLS["deconv"] - calls["deconv"], ops.SSFA_CALLS["blend"] - calls["blend"]) == ((1, 1) if value == "1" else (0, 0))
        assert tuple(out["cls_preds"].shape) == (1, 2, 16, 16) and tuple(out["reg_preds"].shape) == (1, 14, 16, 16)
        assert int((torch.sigmoid(out["cls_preds"]) > 0.2).sum()) == k          # the candidates the bias shift selected
        if dim is None:
            assert tuple(out["iou_preds"].shape) == (1, 2, 16, 16) and tuple(out["dir_preds"].shape) == (1, 4, 16, 16)
            boxes, scores = post.post_process(batch, {"ego": out})
            plain = post.post_process(batch, {"ego": {key: t for key, t in out.items() if key != "iou_preds"}})[1]
            assert float(scores.max()) < float(plain.max())          # the IoU factor ((iou + 1) / 2) ** 4 is below 1
        else:
            assert tuple(out["unc_preds"].shape) == (1, 2 * dim, 16, 16)
            boxes, scores, unc = post.post_process(batch, {"ego": out}, return_uncertainty=True)
            assert tuple(unc.shape) == (boxes.shape[0], dim)
        assert boxes is not None and boxes.shape[0] > 0 and tuple(boxes.shape[1:]) == (8, 3)
        results.append((boxes.cpu().numpy(), scores.cpu().numpy()))
    (b1, s1), (b0, s0) = results
    for name, b, sc in (("fused", b1, s1), ("composition", b0, s0)):
        print(f"{'second_ssfa' if dim is None else 'second_ssfa_uncertainty'} {name}: scores {np.round(sc, 6).tolist()} centres "
              f"{np.round(b.mean(axis=1)[:, :2], 3).tolist()}")
    # The same boxes are kept.  Their ORDER is the order of their scores, which tied scores leave open: each box of one result is
    # compared with the box of the other that lies on it.
    assert 1 <= b1.shape[0] <= k and b1.shape == b0.shape
    match = np.abs(b1[:, None] - b0[None]).sum(axis=(2, 3)).argmin(axis=1)          # the composition's box nearest to each fused one
    assert sorted(match.tolist()) == list(range(len(b0)))                          # one to one
    b0, s0 = b0[match], s0[match]
    np.testing.assert_allclose(b1, b0, rtol=0, atol=1e-3)
    np.testing.assert_allclose(s1, s0, rtol=0, atol=1e-4)
