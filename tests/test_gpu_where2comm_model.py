"""Where2comm and CenterPointWhere2comm on the device against the reference's recordings (tests/golden/w2c_comm_small.npz) at the
project's feature tolerance (1e-3 relative, README); the fused path (heal_comm_mask + heal_warp_att_fuse_levels_masked) against the
torch composition under HEAL_COMM_FUSED=0; post_process on the model's output; one training step."""
import os

import numpy as np
import pytest
import torch

from heal_amd import configs, ops
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
from heal_amd.opencood.tools import train_utils
from tests.golden import w2c_comm_margins as WM
from tests.test_where2comm_model_cpu import M_RANGE, kept, make_module, model_hypes, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "w2c_comm_small.npz"))


@pytest.fixture(scope="module")
def center():
    return np.load(os.path.join(GOLD, "center_small.npz"))


def timed(fn):
    """-> (result, sorted names of the operators that ran)."""
    calls = {}
    ops.TIMING = calls
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    return out, sorted(calls)


def data_of(center):
    return {"processed_lidar": {"voxel_features": torch.from_numpy(center["m3_voxel_features"]).to(DEV),
                                "voxel_coords": torch.from_numpy(center["m3_voxel_coords"]).to(torch.int32).to(DEV),
                                "voxel_num_points": torch.from_numpy(center["m3_voxel_num_points"]).to(torch.int32).to(DEV)},
            "record_len": torch.tensor([3]), "pairwise_t_matrix": torch.from_numpy(center["m3_pairwise"].copy()).to(DEV)}


def model_of(g, **kw):
    hypes = model_hypes(g)
    hypes["model"]["args"].update(kw)
    return WM.model_fill(train_utils.create_model(hypes)).to(DEV).eval(), hypes


# ---- Where2comm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", sorted(WM.MODULE_CASES))
def test_where2comm_module_matches_reference_on_the_kernels(g, prefix, monkeypatch):
    monkeypatch.delenv("HEAL_COMM_FUSED", raising=False)
    module, backbone, inputs = make_module(g, prefix, DEV)
    (y, rate, extra), calls = timed(lambda: module(*inputs, backbone))
    assert "comm_mask" in calls and "warp_att_fuse_levels_masked" in calls and "warp_att_fuse_levels" not in calls
    assert extra == {} and np.float32(rate.item()) == g["mod_rate"]
    e = rel_err(kept(y.cpu().numpy(), prefix), g[prefix + "out"])
    print(prefix, "fused", e)
    assert e <= TOL
    # the composition on the device: the same output to the same tolerance, the same masks exactly
    fused_masks, _ = module.naive_communication.level_masks(inputs[1], WM.RECORD_LEN, 3)
    monkeypatch.setenv("HEAL_COMM_FUSED", "0")
    (y0, rate0, _), calls0 = timed(lambda: module(*inputs, backbone))
    assert "comm_mask" not in calls0 and "warp_att_fuse_levels_masked" not in calls0
    masks0, _ = module.naive_communication.level_masks(inputs[1], WM.RECORD_LEN, 3)
    assert all(torch.equal(a, b) for a, b in zip(fused_masks, masks0)) and np.float32(rate0.item()) == g["mod_rate"]
    e0 = rel_err(kept(y0.cpu().numpy(), prefix), g[prefix + "out"])
    print(prefix, "composition", e0, "fused against composition", rel_err(y.cpu().numpy(), y0.cpu().numpy().astype(np.float64)))
    assert e0 <= TOL and rel_err(y.cpu().numpy(), y0.cpu().numpy().astype(np.float64)) <= TOL


def test_where2comm_without_communication_takes_the_unmasked_entry(g):
    from heal_amd.opencood.models.fuse_modules.where2comm_attn import Where2comm
    from tests.test_where2comm_model_cpu import module_args
    args = module_args("ATTEN", False, 0.0)
    del args["communication"]
    module = Where2comm(args).to(DEV).eval()
    _, _, inputs = make_module(g, "att_ss_", DEV)
    (y, rate, _), calls = timed(lambda: module(*inputs))
    assert "warp_att_fuse_levels" in calls and "comm_mask" not in calls
    assert rate.dtype == torch.int64 and int(rate) == 0 and rate.is_cuda and tuple(y.shape) == (2, 64, 32, 32)


# ---- CenterPointWhere2comm -------------------------------------------------------------------------------------------------------------
def test_model_matches_reference_and_post_process_runs(g, center, monkeypatch):
    monkeypatch.delenv("HEAL_COMM_FUSED", raising=False)
    model, hypes = model_of(g)
    data = data_of(center)
    out, calls = timed(lambda: model(data))
    assert sorted(out) == sorted(WM.MODEL_KEYS)
    assert "comm_mask" in calls and "warp_att_fuse_levels_masked" in calls and "center_boxes" in calls
    masks, _ = model.fusion_net.naive_communication.level_masks(out["cls_preds_single"], [3], 3)
    assert np.array_equal(masks[0].cpu().numpy()[:, 0].astype(np.uint8), g["m_mask0"])
    assert np.float32(out["comm_rate"].item()) == g["m_comm_rate"]
    for key in WM.MODEL_KEYS[:-1]:
        want = g["m_" + key]
        assert tuple(out[key].shape) == want.shape, key
        e = rel_err(out[key].cpu().numpy(), want)
        print(key, e)
        assert e <= TOL, (key, e)
    monkeypatch.setenv("HEAL_COMM_FUSED", "0")
    out0, calls0 = timed(lambda: model(data))
    assert "comm_mask" not in calls0 and "warp_att_fuse_levels_masked" not in calls0
    assert np.float32(out0["comm_rate"].item()) == g["m_comm_rate"]
    for key in ("cls_preds", "bbox_preds", "reg_preds"):
        assert rel_err(out0[key].cpu().numpy(), g["m_" + key]) <= TOL, key
        assert rel_err(out[key].cpu().numpy(), out0[key].cpu().numpy().astype(np.float64)) <= TOL, key
    monkeypatch.delenv("HEAL_COMM_FUSED")
    post = VoxelPostprocessor(hypes["postprocess"], train=False)
    boxes, scores = post.post_process({"ego": {"transformation_matrix": torch.eye(4), "anchor_box": None}}, {"ego": out})
    assert (boxes is None) == (scores is None)
    if boxes is not None:
        assert boxes.shape[1:] == (8, 3) and boxes.shape[0] == scores.shape[0] and bool(torch.isfinite(boxes).all())


def _labels(n, suffix=""):
    rng = np.random.default_rng(11)
    boxes = np.zeros((n, 20, 7), np.float32)
    boxes[:, :6] = np.concatenate([rng.uniform(-12, 12, (n, 6, 2)), rng.uniform(-1.5, -0.5, (n, 6, 1)),
                                   rng.uniform(1.4, 4.0, (n, 6, 3)), rng.uniform(-3, 3, (n, 6, 1))], axis=2)
    mask = np.zeros((n, 20), np.float32)
    mask[:, :6] = 1
    return {"object_bbx_center" + suffix: torch.from_numpy(boxes).to(DEV), "object_bbx_mask" + suffix: torch.from_numpy(mask).to(DEV)}


@pytest.mark.grad
def test_one_training_step_gives_finite_gradients(g, center, monkeypatch):
    """CenterPointLoss on both suffixes.  The communication filter's parameters receive no gradient, as in the reference: the mask is a
    comparison.  The mask itself still comes from the kernel."""
    monkeypatch.delenv("HEAL_COMM_FUSED", raising=False)
    model, hypes = model_of(g)
    model.train()
    hypes["loss"]["args"]["target_assigner_config"]["max_objs"] = 16
    crit = train_utils.create_loss(hypes)
    model.zero_grad()

    def step():
        out = model(data_of(center))
        total = crit(out, _labels(1)) + crit(out, _labels(3, "_single"), suffix="_single")
        total.backward()
        return out, total
    (out, total), calls = timed(step)
    assert "comm_mask" in calls and "warp_att_fuse_levels_masked" not in calls and bool(torch.isfinite(total))
    assert out["bbox_preds"].requires_grad and out["bbox_preds_single"].requires_grad and not out["reg_preds"].requires_grad
    without = sorted(n for n, p in model.named_parameters() if p.grad is None)
    assert without == ["fusion_net.naive_communication.gaussian_filter.bias", "fusion_net.naive_communication.gaussian_filter.weight"]
    for name, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), name
    assert float(model.reg_head.weight.grad.abs().max()) > 0 and float(model.backbone.resnet.layer0[0].conv1.weight.grad.abs().max()) > 0


@pytest.mark.grad
def test_backbone_fix_leaves_only_the_filter_trainable_and_it_gets_no_gradient(g, center):
    model, hypes = model_of(g, backbone_fix=True)
    model.train()
    hypes["loss"]["args"]["target_assigner_config"]["max_objs"] = 16
    crit = train_utils.create_loss(hypes)
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    assert trainable == ["fusion_net.naive_communication.gaussian_filter.bias", "fusion_net.naive_communication.gaussian_filter.weight"]
    out = model(data_of(center))
    total = crit(out, _labels(1))
    torch.cuda.synchronize()
    # nothing trainable lies on a differentiable path (the reference's own state: the mask is torch.where on a comparison)
    assert bool(torch.isfinite(total)) and not total.requires_grad
    assert all(p.grad is None for p in model.parameters())
