"""The fused criterion terms (heal_det_loss, heal_occ_loss, heal_depth_focal_loss) without a GPU: the C ABI is declared, bound
and exported, the workspace queries are the host arithmetic the header states, the *_supported predicates route everything the
kernels do not cover to the torch compositions, and with CPU tensors the loss classes still take those."""
import contextlib
import ctypes
import os

import pytest
import torch

from heal_amd import _capi, configs, ops

SYMBOLS = ["heal_det_loss", "heal_det_loss_workspace", "heal_occ_loss", "heal_occ_loss_workspace", "heal_depth_focal_loss",
           "heal_depth_focal_loss_workspace"]


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def up(x):
    return (x + 255) // 256 * 256


def tiles(n, hw):
    return n * ((hw + 63) // 64)


def occ_ws(n, H, W, ks):
    arr = (ctypes.c_int * len(ks))(*ks)
    return _capi.query("heal_occ_loss_workspace", n, H, W, len(ks), ctypes.cast(arr, ctypes.c_void_p))


def test_symbols_are_declared_bound_and_exported():
    declared = _capi.declared_symbols()
    lib = _capi.lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _capi.signatures(), name
        assert hasattr(lib, name), name
    assert _capi.abi_version_of_header() == 13
    assert int(lib.heal_abi_version()) == 13


def test_workspace_queries_are_the_header_arithmetic():
    q = _capi.query
    assert q("heal_det_loss_workspace", 2, 2, 16, 24) == 256 * 2 + up(12 * tiles(2, 16 * 24)) == 768
    assert q("heal_det_loss_workspace", 4, 2, 256, 256) == 256 * 4 + up(12 * 4096) == 50176
    assert occ_ws(2, 16, 24, [1, 2, 4]) == 256 * 3 * 2 + up(4 * (tiles(2, 384) + tiles(2, 96) + tiles(2, 24))) == 1792
    assert occ_ws(4, 256, 256, [1, 2, 4]) == 256 * 3 * 4 + up(4 * 4 * (1024 + 256 + 64)) == 24576
    assert q("heal_depth_focal_loss_workspace", 8, 12, 6, 8) == up(4 * tiles(8, 48)) == 256
    assert q("heal_depth_focal_loss_workspace", 16, 48, 48, 64) == up(4 * tiles(16, 3072)) == 3072
    # N = 0 or an empty map
    for args in ((0, 2, 16, 24), (2, 0, 16, 24), (2, 2, 0, 24), (2, 2, 16, 0), (2, 5, 16, 24)):
        assert q("heal_det_loss_workspace", *args) == 0, args
    for args in ((0, 12, 6, 8), (8, 0, 6, 8), (8, 12, 0, 8), (8, 12, 6, 0)):
        assert q("heal_depth_focal_loss_workspace", *args) == 0, args
    assert occ_ws(0, 16, 24, [1, 2, 4]) == 0 and occ_ws(2, 0, 24, [1]) == 0 and occ_ws(2, 16, 0, [1]) == 0
    assert occ_ws(2, 16, 24, [1, 2, 32]) == 0            # a level whose pooled map is empty
    assert occ_ws(2, 16, 24, [1, 1, 1, 1, 1][:4]) > 0 and occ_ws(2, 16, 24, []) == 0


def _inputs(n=2, H=16, W=24):
    from tests.test_reference_live import _loss_inputs
    return _loss_inputs(0, n=n, H=H, W=W)


def test_supported_is_false_for_cpu_tensors_and_the_switch():
    out, tgt = _inputs()
    labels = (tgt["pos_equal_one"], tgt["neg_equal_one"], tgt["targets"])
    assert not ops.det_loss_supported(out["cls_preds"], out["reg_preds"], out["dir_preds"], *labels)
    assert not ops.det_loss_supported(out["cls_preds"], out["reg_preds"], None, *labels)
    assert not ops.occ_loss_supported(out["occ_single_list"], labels[0], labels[1], [1, 2, 4])
    logit, idx, mask = out["depth_items_m2"]
    assert not ops.depth_focal_loss_supported(logit, idx, mask) and not ops.depth_focal_loss_supported(logit, idx)
    with env("HEAL_LOSS_FUSED", "0"):
        assert not ops.loss_fused_enabled()
    with env("HEAL_LOSS_FUSED", "1"):
        assert ops.loss_fused_enabled()


def test_supported_checks_every_condition_of_the_kernel_path(monkeypatch):
    """With the device test out of the way (tensors that claim to be CUDA), every other condition decides on its own."""
    monkeypatch.setattr(ops, "_loss_map_ok", lambda t: bool(isinstance(t, torch.Tensor) and t.dtype == torch.float32
                                                             and t.dim() == 4 and t.numel() > 0))
    out, tgt = _inputs()
    cls, reg, dirp, occ = out["cls_preds"], out["reg_preds"], out["dir_preds"], out["occ_single_list"]
    pos, neg, targets = tgt["pos_equal_one"], tgt["neg_equal_one"], tgt["targets"]
    logit, idx, mask = out["depth_items_m2"]
    with env("HEAL_LOSS_FUSED", "1"):
        assert ops.det_loss_supported(cls, reg, dirp, pos, neg, targets)
        assert ops.det_loss_supported(cls, reg, None, pos.double(), neg.double(), targets.double(), batch_size=2)
        assert not ops.det_loss_supported(cls, reg, dirp, pos, neg, targets, gamma=1.5)
        assert not ops.det_loss_supported(cls, reg, dirp, pos, neg, targets, num_bins=4)
        assert not ops.det_loss_supported(cls, reg, dirp, pos, neg, targets, iou={"sigma": 3.0, "weight": 1.0})
        assert not ops.det_loss_supported(cls, reg, dirp, pos, neg, targets, batch_size=3)
        assert not ops.det_loss_supported(cls, reg, dirp, pos.double(), neg, targets)            # mixed label types
        assert not ops.det_loss_supported(cls, reg, dirp, pos.half(), neg.half(), targets.half())
        assert not ops.det_loss_supported(cls.double(), reg, dirp, pos, neg, targets)
        assert not ops.det_loss_supported(cls, reg[:, :7], dirp, pos, neg, targets)
        assert not ops.det_loss_supported(cls, reg, dirp, pos[:1], neg, targets)
        wide = torch.zeros((2, 5, 16, 24))
        assert not ops.det_loss_supported(wide, torch.zeros((2, 35, 16, 24)), None, torch.zeros((2, 16, 24, 5)),
                                          torch.zeros((2, 16, 24, 5)), torch.zeros((2, 16, 24, 35)))      # A > 4
        assert ops.occ_loss_supported(occ, pos, neg, [1, 2, 4])
        assert ops.occ_loss_supported(occ, pos.double(), neg.double(), [1, 2, 4])
        assert not ops.occ_loss_supported(occ, pos, neg, [1, 2, 4], gamma=3.0)
        assert not ops.occ_loss_supported(occ, pos, neg, [1, 2, 2])                              # not the pooled label's shape
        assert not ops.occ_loss_supported(occ + occ, pos, neg, [1, 2, 4] * 2)                    # more than four levels
        assert not ops.occ_loss_supported([], pos, neg, [1, 2, 4])
        assert ops.depth_focal_loss_supported(logit, idx, mask) and ops.depth_focal_loss_supported(logit, idx)
        assert not ops.depth_focal_loss_supported(logit, idx, mask, smooth_target=True)
        assert not ops.depth_focal_loss_supported(logit, idx, mask, gamma=1.0)
        assert not ops.depth_focal_loss_supported(logit, idx.int(), mask)
        assert not ops.depth_focal_loss_supported(logit, idx, mask > 0)
        assert not ops.depth_focal_loss_supported(logit, idx[:, :3], None)
    with env("HEAL_LOSS_FUSED", "0"):
        assert not ops.det_loss_supported(cls, reg, dirp, pos, neg, targets)
        assert not ops.occ_loss_supported(occ, pos, neg, [1, 2, 4])
        assert not ops.depth_focal_loss_supported(logit, idx, mask)


def test_wrappers_refuse_cpu_tensors():
    out, tgt = _inputs()
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.det_loss(out["cls_preds"], out["reg_preds"], out["dir_preds"], tgt["pos_equal_one"], tgt["neg_equal_one"],
                     tgt["targets"], 2.0, 0.25, 3.0, (1.0, 2.0, 0.2), anchor_yaw=[0.0, 1.0])
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.occ_loss(out["occ_single_list"], tgt["pos_equal_one"], tgt["neg_equal_one"], [1, 2, 4], [0.4, 0.2, 0.1], 2.0, 0.25)
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.depth_focal_loss(*out["depth_items_m2"])


@pytest.mark.grad
def test_loss_classes_take_the_composition_on_cpu(monkeypatch):
    """CPU tensors never reach the C ABI: the three classes give what they gave before, loss_dict of Python floats included."""
    from heal_amd.opencood.tools.train_utils import create_loss
    monkeypatch.setattr(_capi, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("C ABI called on CPU tensors")))
    hy = configs.lidar_pyramid()
    hy["loss"]["args"]["depth"]["use_fg_mask"] = True
    crit = create_loss(hy)
    out, tgt = _inputs()
    out["pyramid"] = "single"
    for t in [out["cls_preds"], out["reg_preds"], out["dir_preds"], out["depth_items_m2"][0]] + out["occ_single_list"]:
        t.requires_grad_(True)
    with env("HEAL_LOSS_FUSED", "1"):
        total = crit(out, tgt)
    total.backward()
    assert all(isinstance(crit.loss_dict[k], float) for k in ("total_loss", "reg_loss", "cls_loss", "dir_loss", "pyramid_loss"))
    assert isinstance(crit.loss_dict["depth_loss"], torch.Tensor)
    assert out["cls_preds"].grad is not None and out["occ_single_list"][2].grad is not None
