"""The SECOND + SSFA detectors on the CPU: the reference's state-dict keys in its order, its recorded outputs
(tests/golden/gen_golden_ssfa.py; the same composition in the same precision), the fp64 references of tests/ssfa_refs.py against
torch, construction from configs.second_ssfa, the gradient path, `iou_preds` rescoring in VoxelPostprocessor.post_process, and the
plumbing of the new entry points (header, ctypes table, switch, README row)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, configs, switches
from heal_amd.opencood.models.sub_modules.cia_ssd_utils import SSFA, Head
from heal_amd.opencood.tools.train_utils import create_model
from tests import ssfa_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SMALL_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
HEAD = {"num_input": 128, "num_pred": 14, "num_cls": 2, "num_iou": 2, "use_dir": True, "num_dir": 4}
SYMBOLS = ("heal_ssfa_fused_enabled", "heal_deconv3x3_s2_supported", "heal_deconv3x3_s2", "heal_ssfa_blend_supported",
           "heal_ssfa_blend")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ssfa_small.npz"))


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLD, "ssfa_state_dict_keys.json")) as f:
        return json.load(f)


def golden_state(gold, name):
    head = name + "/sd/"
    return {k[len(head):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(head)}


def rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / float(np.abs(np.asarray(want)).max())


# ------------------------------------------------------------------------------------------------------------------ the mirror
def test_mirror_has_the_reference_keys_in_order(ref_keys):
    assert list(SSFA({"feature_num": 128}).state_dict()) == ref_keys["ssfa"]
    assert list(Head(**HEAD).state_dict()) == ref_keys["head"]
    assert list(Head(**dict(HEAD, use_dir=False)).state_dict()) == ref_keys["head_no_dir"]


def test_ssfa_reproduces_the_reference_recording(gold):
    model = SSFA({"feature_num": 128}).eval()
    model.load_state_dict(golden_state(gold, "ssfa"), strict=True)
    hooks = {}
    model.conv_0.register_forward_hook(lambda mod, inp, res: hooks.update(x_middle_0=inp[0].detach(), x_output_0=res.detach()))
    model.w_0.register_forward_hook(lambda mod, inp, res: hooks.update(w0=res.detach()))
    model.w_1.register_forward_hook(lambda mod, inp, res: hooks.update(w1=res.detach()))
    with torch.no_grad():
        got = model(torch.from_numpy(gold["input"]))
    hooks["x_weight"] = torch.softmax(torch.cat([hooks.pop("w0"), hooks.pop("w1")], dim=1), dim=1)
    assert got.shape == gold["output"].shape and got.is_contiguous()
    for name, value in [("output", got)] + sorted(hooks.items()):
        err = rel(value.numpy(), gold[name])
        print(f"{name}: {err:.3e} of the largest magnitude")
        assert err <= 1e-5, name


@pytest.mark.grad          # the heads have no CPU inference path: on the CPU they run as the modules (the gradient path)
def test_head_reproduces_the_reference_recording(gold):
    head = Head(**HEAD).eval()
    head.load_state_dict(golden_state(gold, "head"), strict=True)
    out = head(torch.from_numpy(gold["output"]))
    assert list(out) == ["reg_preds", "cls_preds", "dir_preds", "iou_preds"]
    for k, v in out.items():
        assert rel(v.detach().numpy(), gold["head/" + k]) <= 1e-5, k


@pytest.mark.grad
def test_head_without_direction_returns_the_zero_tensor():
    out = Head(**dict(HEAD, use_dir=False))(torch.randn(3, 128, 4, 4))
    assert tuple(out["dir_preds"].shape) == (3, 1, 2) and not bool(out["dir_preds"].any())
    assert tuple(out["iou_preds"].shape) == (3, 2, 4, 4) and tuple(out["reg_preds"].shape) == (3, 14, 4, 4)


# -------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", [(1, 4, 3, 1, 1), (2, 5, 6, 3, 4), (1, 8, 8, 5, 2)])
@pytest.mark.parametrize("relu", [False, True])
def test_deconv_reference_agrees_with_conv_transpose2d(shape, relu):
    n, cin, cout, H, W = shape
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn((n, cin, H, W), generator=g, dtype=torch.float64), torch.randn((cin, cout, 3, 3), generator=g, dtype=torch.float64)
    b, r = torch.randn(cout, generator=g, dtype=torch.float64), torch.randn((n, cout // 2, 2 * H, 2 * W), generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    want = F.relu(want) if relu else want
    want[:, :cout // 2] += r
    got = ssfa_refs.deconv3x3_s2(x.numpy(), w.numpy(), b.numpy(), relu, r.numpy())
    assert got.shape == (n, cout, 2 * H, 2 * W) and rel(got, want.numpy()) <= 1e-13
    plain = ssfa_refs.deconv3x3_s2(x.numpy(), w.numpy(), None, False, None)
    assert rel(plain, F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1).numpy()) <= 1e-13


def test_blend_reference_agrees_with_the_torch_composition():
    g = torch.Generator().manual_seed(4)
    a, b = (torch.randn((2, 16, 3, 4), generator=g, dtype=torch.float64) for _ in range(2))
    wa, wb = (torch.randn(16, generator=g, dtype=torch.float64) for _ in range(2))
    ba, bb = 0.3, -0.7
    s = torch.cat([F.conv2d(a, wa.view(1, -1, 1, 1)) + ba, F.conv2d(b, wb.view(1, -1, 1, 1)) + bb], dim=1).softmax(dim=1)
    want = a * s[:, 0:1] + b * s[:, 1:]
    out, pa = ssfa_refs.ssfa_blend(a.numpy(), b.numpy(), wa.numpy(), ba, wb.numpy(), bb)
    assert rel(out, want.numpy()) <= 1e-13 and rel(pa, s[:, 0:1].numpy()) <= 1e-13
    far, pfar = ssfa_refs.ssfa_blend(a.numpy(), b.numpy(), 0 * wa.numpy(), 800.0, 0 * wb.numpy(), 0.0)    # no overflow on the way
    assert np.array_equal(far, a.numpy()) and bool((pfar == 1.0).all())


# ------------------------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("dim", [None, 3])
def test_models_build_from_configs_with_the_reference_names(dim, ref_keys):
    hypes = configs.second_ssfa(SMALL_RANGE, dim)
    hypes["model"]["args"]["shrink_header"] = {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [128], "input_dim": 128}
    name = "second_ssfa" if dim is None else "second_ssfa_uncertainty"
    assert hypes["model"]["core_method"] == name and hypes["model"]["args"]["ssfa"] == {"feature_num": 128}
    assert {"mean_vfe", "spconv", "map2bev", "ssfa"} <= set(hypes["model"]["args"])
    assert hypes["postprocess"]["anchor_args"]["feature_stride"] == 8 and hypes["postprocess"]["anchor_args"]["W"] == 256
    model = create_model(hypes)
    assert type(model).__name__ == ("SecondSSFA" if dim is None else "SecondSSFAUncertainty")
    heads = ["head"] if dim is None else ["cls_head", "reg_head", "unc_head", "dir_head"]
    assert [n for n, _ in model.named_children()] == ["vfe", "spconv_block", "map_to_bev", "ssfa", "shrink_conv"] + heads
    mine = [k for k in model.state_dict() if not k.startswith("spconv_block.")]
    assert mine == ref_keys[name]
    if dim is not None:
        assert model.unc_head.out_channels == 2 * dim and "uncertainty_dim" in hypes["model"]["args"]
        assert hypes["postprocess"]["core_method"] == "UncertaintyVoxelPostprocessor"
    else:
        assert set(hypes["model"]["args"]["head"]) == set(HEAD)
    plain = create_model(configs.second_ssfa(SMALL_RANGE, dim))              # no shrink header: the attribute is absent
    assert not hasattr(plain, "shrink_conv") and plain.out_channel == 128


@pytest.mark.grad
def test_gradient_path_back_propagates_through_ssfa(gold):
    model = SSFA({"feature_num": 128}).train()
    model.load_state_dict(golden_state(gold, "ssfa"), strict=True)
    x = torch.from_numpy(gold["input"]).clone().requires_grad_(True)
    model(x).square().mean().backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------------------------- iou rescoring
def _post_case(monkeypatch, n_cavs):
    """Hand-built maps: zero regression (the boxes are the anchors), a few confident anchors far apart in each cav, an IoU logit
    per anchor.  The rotated NMS (a device kernel) is replaced by its result on boxes that do not overlap: all of them, by score."""
    from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    from heal_amd.opencood.utils import box_utils
    monkeypatch.setattr(box_utils, "nms_rotated",
                        lambda boxes, scores, thr: torch.argsort(scores, descending=True).numpy().astype(np.int32))
    post = VoxelPostprocessor(configs.second_ssfa(SMALL_RANGE)["postprocess"], train=False)
    anchors = torch.from_numpy(post.generate_anchor_box())
    H, W, A = anchors.shape[:3]
    g = torch.Generator().manual_seed(11 + n_cavs)
    data, out, want = {}, {}, []
    for c in range(n_cavs):
        cls = torch.full((1, A, H, W), -6.0)
        iou = torch.randn((1, A, H, W), generator=g) * 2
        for k, (y, x, a) in enumerate([(4 + 8 * c, 5, 0), (6 + 8 * c, 20, 1), (10 + 8 * c, 12, 0)]):
            cls[0, a, y, x] = 0.5 + k + 0.25 * c
            want.append((float(torch.sigmoid(cls[0, a, y, x])), float(torch.sigmoid(iou[0, a, y, x]))))
        data[f"cav{c}"] = {"transformation_matrix": torch.eye(4), "anchor_box": anchors}
        out[f"cav{c}"] = {"cls_preds": cls, "reg_preds": torch.zeros(1, 7 * A, H, W), "dir_preds": torch.zeros(1, 2 * A, H, W),
                          "iou_preds": iou}
    return post, data, out, want


@pytest.mark.parametrize("n_cavs", [1, 2])
def test_post_process_rescoring_with_iou_preds(monkeypatch, n_cavs):
    post, data, out, want = _post_case(monkeypatch, n_cavs)
    boxes, scores = post.post_process(data, out)                      # raised NotImplementedError before
    assert boxes.shape == (3 * n_cavs, 8, 3) and scores.shape == (3 * n_cavs,)
    expect = sorted((p * ((s + 1) / 2) ** 4 for p, s in want), reverse=True)
    np.testing.assert_allclose(scores.numpy(), np.array(expect, dtype=np.float32), rtol=2e-6)
    assert bool((scores[:-1] >= scores[1:]).all())
    # without the IoU head: the same boxes with the plain probabilities (one cav: that is the decode kernel's path, a device
    # operator, so the comparison goes through the tensor path both times)
    plain = {k: {n: t for n, t in v.items() if n != "iou_preds"} for k, v in out.items()}
    boxes0, scores0 = post._post_process_multi(data, plain)
    np.testing.assert_allclose(np.sort(scores0.numpy())[::-1], np.array(sorted((p for p, _ in want), reverse=True), np.float32),
                               rtol=2e-6)
    key = lambda b: sorted(map(tuple, b.reshape(len(b), -1).numpy().round(4).tolist()))     # noqa: E731
    assert key(boxes) == key(boxes0)


def test_post_process_without_iou_preds_is_unchanged_by_a_neutral_head(monkeypatch):
    """An IoU logit of +inf-like size gives iou = 1 and the factor ((1 + 1) / 2) ** 4 = 1: the result equals the no-IoU result."""
    post, data, out, _ = _post_case(monkeypatch, 2)
    for v in out.values():
        v["iou_preds"] = torch.full_like(v["iou_preds"], 40.0)
    plain = {k: {n: t for n, t in v.items() if n != "iou_preds"} for k, v in out.items()}
    (b1, s1), (b0, s0) = post.post_process(data, out), post.post_process(data, plain)
    assert torch.equal(b1, b0) and torch.equal(s1, s0)


def test_post_process_takes_the_zero_direction_tensor_as_no_direction_map(monkeypatch):
    post, data, out, _ = _post_case(monkeypatch, 1)
    plain = {k: {n: t for n, t in v.items() if n != "dir_preds"} for k, v in out.items()}
    for v in out.values():
        v["dir_preds"] = torch.zeros(1, 1, 2)
    (b1, s1), (b0, s0) = post.post_process(data, out), post.post_process(data, plain)
    assert torch.equal(b1, b0) and torch.equal(s1, s0)


# -------------------------------------------------------------------------------------------------------------------- plumbing
def test_ssfa_header_is_bound():
    sig = _capi.signatures_ssfa()
    assert sorted(sig) == sorted(SYMBOLS)
    with open(_capi.HEADER_SSFA) as f:
        text = f.read()
    assert sorted(set(re.findall(r"\b(heal_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))) == sorted(SYMBOLS)
    res, args = sig["heal_deconv3x3_s2"]
    assert res is ctypes.c_int and len(args) == 13 and args[:4] == [ctypes.c_void_p] * 4 and args[4:11] == [ctypes.c_int] * 7
    res, args = sig["heal_ssfa_blend"]
    assert res is ctypes.c_int and len(args) == 12 and args[:6] == [ctypes.c_void_p] * 6 and args[6:9] == [ctypes.c_int] * 3
    lib = _capi.lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)


def test_support_rules():
    from heal_amd import ops
    for c in (64, 128, 256):
        for d in (64, 128, 256):
            for hw in ((1, 1), (1, 7), (17, 9), (50, 176), (3, 1000)):
                assert ops.deconv3x3_s2_supported(c, d, *hw), (c, d, hw)
    for bad in ((48, 64, 4, 4), (64, 48, 4, 4), (16, 64, 4, 4), (64, 64, 0, 4), (64, 64, 4, 0), (4096, 64, 4, 4)):
        assert not ops.deconv3x3_s2_supported(*bad), bad
    for c in (64, 128):
        for hw in (4, 12, 60, 35200):
            assert ops.ssfa_blend_supported(c, hw), (c, hw)
    for bad in ((32, 64), (256, 64), (128, 6), (128, 0), (64, 1 << 24)):
        assert not ops.ssfa_blend_supported(*bad), bad


def test_fragment_order():
    from heal_amd import ops
    w = torch.arange(32 * 48 * 9, dtype=torch.float32).reshape(32, 48, 3, 3)
    f = ops._deconv3x3_s2_pack(w)
    assert tuple(f.shape) == (3, 4, 9, 64, 2)
    for mt, kc, t, lane, j in ((0, 0, 0, 0, 0), (2, 3, 8, 63, 1), (1, 2, 5, 37, 1), (2, 0, 4, 16, 0)):
        assert float(f[mt, kc, t, lane, j]) == float(w[8 * kc + 4 * j + (lane >> 4), 16 * mt + (lane & 15), t // 3, t % 3])


def test_switch_is_declared_documented_and_read_by_the_library(monkeypatch):
    """HEAL_SSFA_FUSED is one of the library's own variables (heal_ssfa_fused_enabled reads it when called)."""
    from heal_amd import ops
    assert switches.SWITCHES["HEAL_SSFA_FUSED"].where == "library"
    monkeypatch.delenv("HEAL_SSFA_FUSED", raising=False)
    assert ops.ssfa_fused_enabled() is True
    for text, want in (("0", False), ("1", True), ("", True)):
        monkeypatch.setenv("HEAL_SSFA_FUSED", text)
        assert ops.ssfa_fused_enabled() is want
    monkeypatch.setenv("HEAL_SSFA_FUSED", "yes")
    with pytest.raises(_capi.HealAmdError, match="HEAL_SSFA_FUSED"):
        ops.ssfa_fused_enabled()
    with open(os.path.join(ROOT, "README.md")) as f:
        assert any(line.startswith("| `HEAL_SSFA_FUSED=0`") for line in f.read().splitlines())
