"""The anchor-free centre head on the MI355X: heal_center_loss (through ops and through CenterPointLoss) against the reference's
recordings of tests/golden/center_small.npz, its debug outputs, exact zeros, bit-equal repeats, NULL outputs, the paths that take
the composition, max_objs = 500; heal_center_boxes; heal_center_decode_nms through post_process (single cav and the late form);
the two models against the reference's head maps and one training step."""
import contextlib
import os

import numpy as np
import pytest
import torch

from heal_amd import configs, ops
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
from heal_amd.opencood.loss.center_point_loss import CenterPointLoss, gaussian_radius
from heal_amd.opencood.tools import train_utils
from tests.golden import center_margins as CM
from tests.golden.detfill import fill_module

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5            # loss terms relative; gradients and anno_boxes against the largest magnitude of the expected tensor
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "center_small.npz"))


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


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _case(c):
    """(the four device tensors, the kernel's keyword arguments) of a case dict of center_margins.loss_case."""
    t = [torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("cls", "bbox", "boxes", "mask")]
    return t, CenterPointLoss(CM.loss_args(c))._kernel_cfg()


def _check_terms_and_grads(tag, terms, grads, want_terms, want_grads):
    for name, got, want in zip(("cls", "reg"), terms, want_terms):
        err = abs(float(got) - float(want)) / abs(float(want))
        print(f"{tag} {name}_loss {float(got)!r} (expected {float(want)!r}) relative error {err:.3e}")
        assert err <= TOL
    for name, got, want in zip(("grad_cls", "grad_bbox"), grads, want_grads):
        err = _rel(got.cpu().numpy(), want)
        print(f"{tag} {name} error / largest magnitude {err:.3e}")
        assert err <= TOL


@pytest.mark.parametrize("prefix", CM.LOSS_CASES)
def test_kernel_matches_reference_terms_gradients_and_targets(g, prefix):
    c = CM.loss_case(g, prefix)
    t, cfg = _case(c)
    assert ops.center_loss_supported(*t, cfg["cav_lidar_range"], cfg["voxel_size"], cfg["out_size_factor"], cfg["max_objs"])
    terms, grads, dbg = ops.center_loss(*t, debug=True, **cfg)
    torch.cuda.synchronize()
    _check_terms_and_grads(prefix, terms.cpu(), grads, (g[prefix + "cls_loss"], g[prefix + "reg_loss"]),
                           (g[prefix + "grad_cls"], g[prefix + "grad_bbox"]))
    inds, masks = dbg["inds"].cpu().numpy(), dbg["masks"].cpu().numpy()
    assert np.array_equal(inds, g[prefix + "inds"]) and np.array_equal(masks, g[prefix + "masks"])
    heat, want = dbg["heatmap"].cpu().numpy(), g[prefix + "heatmap"]
    assert np.array_equal(heat == 1, want == 1) and np.array_equal(heat == 0, want == 0)
    ulps = int(np.abs(heat.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max())
    print(f"{prefix} heat map: largest difference {ulps} fp32 ulp")
    assert ulps <= 1
    err = _rel(dbg["anno_boxes"].cpu().numpy(), g[prefix + "anno_boxes"])
    print(f"{prefix} anno_boxes error / largest magnitude {err:.3e}")
    assert err <= TOL
    # grad_bbox is bitwise zero off the kept inds; both gradients are bitwise zero where the clamp is active
    gb = grads[1].cpu().numpy().view(np.uint32).reshape(inds.shape[0], 8, -1)
    off = np.ones((inds.shape[0], gb.shape[2]), bool)
    for b in range(inds.shape[0]):
        off[b, inds[b][masks[b] == 1]] = False
    assert not gb.transpose(0, 2, 1)[off].any()
    clamped = np.abs(c["cls"]) > CM.CLAMP_EDGE
    assert not grads[0].cpu().numpy().view(np.uint32)[clamped].any()
    assert prefix != "c_" or clamped.sum() >= 4                         # the four +-12 logits (and what the draw adds)


@pytest.mark.parametrize("prefix", CM.LOSS_CASES)
def test_loss_module_matches_reference_and_reports_the_kernel(g, prefix):
    c = CM.loss_case(g, prefix)
    (cls, bbox, boxes, mask), _ = _case(c)
    cls.requires_grad_(True)
    bbox.requires_grad_(True)
    crit = CenterPointLoss(CM.loss_args(c))
    calls = {}
    ops.TIMING = calls
    try:
        total = crit({"cls_preds": cls, "bbox_preds": bbox}, {"object_bbx_center": boxes, "object_bbx_mask": mask})
        total.backward()
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert sorted(calls) == ["center_loss"]
    d = crit.loss_dict
    _check_terms_and_grads(prefix + " module", (d["cls_loss"], d["reg_loss"]), (cls.grad, bbox.grad),
                           (g[prefix + "cls_loss"], g[prefix + "reg_loss"]), (g[prefix + "grad_cls"], g[prefix + "grad_bbox"]))
    err = abs(d["total_loss"] - float(g[prefix + "total_loss"])) / float(g[prefix + "total_loss"])
    print(f"{prefix} module total {d['total_loss']!r} relative error {err:.3e}")
    assert err <= TOL and abs(float(total.detach()) - d["total_loss"]) <= TOL * d["total_loss"]


def test_two_launches_are_bit_equal_whatever_the_workspace_holds(g):
    c = CM.loss_case(g, "c_")
    t, cfg = _case(c)
    nbytes = ops._capi.query("heal_center_loss_workspace", 3, 32, 32, 8)
    runs = []
    for fill in (None, 0xFF, 0x00):
        ws = None
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        terms, grads, dbg = ops.center_loss(*t, debug=True, workspace=ws, **cfg)
        runs.append([terms, *grads, *[dbg[k] for k in sorted(dbg)]])
    torch.cuda.synchronize()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b) and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_null_gradient_and_debug_pointers_are_accepted(g):
    c = CM.loss_case(g, "a_")
    t, cfg = _case(c)
    full, grads = ops.center_loss(*t, **cfg)
    none, no_grads = ops.center_loss(*t, need_grad=False, **cfg)
    only_cls, g_cls = ops.center_loss(*t, need_grad=(True, False), **cfg)
    only_box, g_box = ops.center_loss(*t, need_grad=(False, True), **cfg)
    torch.cuda.synchronize()
    assert no_grads is None and g_cls[1] is None and g_box[0] is None
    assert torch.equal(full, none) and torch.equal(full, only_cls) and torch.equal(full, only_box)
    assert torch.equal(grads[0], g_cls[0]) and torch.equal(grads[1], g_box[1])


def test_composition_runs_where_the_kernel_does_not_apply(g):
    c = CM.loss_case(g, "a_")
    (cls, bbox, boxes, mask), _ = _case(c)
    want = float(g["a_total_loss"])

    def run(args, maps, targets):
        calls = {}
        ops.TIMING = calls
        try:
            crit = CenterPointLoss(args)
            total = float(crit({"cls_preds": maps[0], "bbox_preds": maps[1]},
                               {"object_bbx_center": targets[0], "object_bbx_mask": targets[1]}))
            torch.cuda.synchronize()
        finally:
            ops.TIMING = None
        return total, sorted(calls)

    total, calls = run(CM.loss_args(c), (cls, bbox), (boxes, mask))
    assert calls == ["center_loss"] and abs(total - want) <= TOL * want
    with env("HEAL_LOSS_FUSED", "0"):
        total, calls = run(CM.loss_args(c), (cls, bbox), (boxes, mask))
    assert calls == [] and abs(total - want) <= TOL * want
    total, calls = run(CM.loss_args(c), (cls.cpu(), bbox.cpu()), (boxes.cpu(), mask.cpu()))
    assert calls == [] and abs(total - want) <= TOL * want
    # a map that is not the feature map of the target assigner's range: the reference would fail in its gather or draw a
    # heat map of another size; the kernel refuses, the module takes the composition (which fails like the reference)
    args = CM.loss_args(c)
    args["target_assigner_config"]["cav_lidar_range"] = [-4.4, -4.4, -3, 4.4, 4.4, 1]
    cfg = CenterPointLoss(args)._kernel_cfg()
    assert not ops.center_loss_supported(cls, bbox, boxes, mask, cfg["cav_lidar_range"], cfg["voxel_size"], 2, 8)
    with pytest.raises(ops._capi.HealAmdError):
        ops.center_loss(cls, bbox, boxes, mask, **cfg)
    with pytest.raises(RuntimeError):
        run(args, (cls, bbox), (boxes, mask))


def _crowd(seed):
    """2 x 64 x 64 with 120 objects per sample and CenterPoint's customary max_objs = 500, redrawn until the margins hold."""
    H = W = 64
    r = [-25.6, -25.6, -3, 25.6, 25.6, 1]
    for attempt in range(100):
        rng = np.random.default_rng(seed + attempt)
        boxes = np.zeros((2, 128, 7), np.float32)
        boxes[:, :120, 0] = rng.uniform(r[0] - 0.5, r[3] + 0.5, (2, 120))
        boxes[:, :120, 1] = rng.uniform(r[1] - 0.5, r[4] + 0.5, (2, 120))
        boxes[:, :120, 2] = rng.uniform(-1.5, -0.5, (2, 120))
        boxes[:, :120, 3:6] = rng.uniform((1.2, 1.4, 3.0), (3.5, 4.0, 8.0), (2, 120, 3))
        boxes[:, :120, 6] = rng.uniform(-3.1, 3.1, (2, 120))
        mask = np.zeros((2, 128), np.float32)
        mask[:, :120] = 1
        c = dict(cls=(rng.standard_normal((2, 1, H, W)) * 2 - 1).astype(np.float32),
                 bbox=(rng.standard_normal((2, 8, H, W)) * 0.7).astype(np.float32), boxes=boxes, mask=mask, range=np.array(r),
                 voxel=np.array([0.4, 0.4, 4]), factor=np.array(2), max_objs=np.array(500), min_radius=np.array(2),
                 overlap=np.array(0.1), code_weights=np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]),
                 cls_weight=np.array(1.0), loc_weight=np.array(0.25))
        cell, rad, logit, finite = CM.loss_margins(c, gaussian_radius)
        if cell >= 1e-3 and rad >= 1e-3 and logit >= CM.LOGIT_MARGIN and finite:
            return c
    raise AssertionError("the margins did not settle")


def test_max_objs_500_matches_the_cpu_composition():
    c = _crowd(500)
    crit = CenterPointLoss(CM.loss_args(c))
    cls = torch.from_numpy(c["cls"]).requires_grad_(True)
    bbox = torch.from_numpy(c["bbox"]).requires_grad_(True)
    boxes, mask = torch.from_numpy(c["boxes"]), torch.from_numpy(c["mask"])
    crit({"cls_preds": cls, "bbox_preds": bbox}, {"object_bbx_center": boxes, "object_bbx_mask": mask}).backward()
    want = crit.assign_targets(boxes, mask)
    assert 150 < int(want["masks"].sum()) <= 240                        # most of the 2 x 120 are inside the map
    t, cfg = _case(c)
    terms, grads, dbg = ops.center_loss(*t, debug=True, **cfg)
    torch.cuda.synchronize()
    _check_terms_and_grads("max_objs 500", terms.cpu(), grads, (crit.loss_dict["cls_loss"], crit.loss_dict["reg_loss"]),
                           (cls.grad.numpy(), bbox.grad.numpy()))
    assert torch.equal(dbg["inds"].cpu(), want["inds"]) and torch.equal(dbg["masks"].cpu(), want["masks"])
    heat = dbg["heatmap"].cpu()
    assert torch.equal(heat == 1, want["heatmaps"] == 1) and torch.equal(heat == 0, want["heatmaps"] == 0)
    assert _rel(heat.numpy(), want["heatmaps"].numpy()) <= TOL


def test_scaled_loss_gives_scaled_gradients(g):
    c = CM.loss_case(g, "a_")
    grads = []
    for scale in (1.0, 3.0):
        (cls, bbox, boxes, mask), _ = _case(c)
        cls.requires_grad_(True)
        bbox.requires_grad_(True)
        total = CenterPointLoss(CM.loss_args(c))({"cls_preds": cls, "bbox_preds": bbox},
                                                  {"object_bbx_center": boxes, "object_bbx_mask": mask})
        (scale * total).backward()
        grads.append((cls.grad, bbox.grad))
    for a, b in zip(*grads):
        assert torch.equal(3.0 * a, b) and bool(a.abs().max() > 0)


def test_center_boxes_matches_generate_predicted_boxes(g):
    calls = {}
    ops.TIMING = calls
    try:
        out = ops.center_boxes(torch.from_numpy(g["box_bbox"]).to(DEV), g["box_range"].tolist(), [0.4, 0.4, 4], 2)
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert sorted(calls) == ["center_boxes"] and tuple(out.shape) == (2, 35, 7) and not out.requires_grad
    got, want = out.cpu().numpy(), g["box_out"]
    for col in range(7):
        err = _rel(got[..., col], want[..., col])
        print(f"center_boxes column {col}: error / largest magnitude {err:.3e}")
        assert err <= TOL
    x = torch.from_numpy(g["box_bbox"]).to(DEV).requires_grad_(True)
    assert not ops.center_boxes(x * 1.0, g["box_range"].tolist(), [0.4, 0.4, 4], 2).requires_grad      # no gradient through it


def _post(g):
    p = configs.lidar_centerpoint("max", [-6.4, -6.4, -3, 6.4, 6.4, 1], dir_head=True)["postprocess"]
    p["gt_range"] = g["dec_gt_range"].tolist()
    assert p["target_args"]["score_threshold"] == float(g["dec_score_thr"]) and p["nms_thresh"] == float(g["dec_nms_thr"])
    return VoxelPostprocessor(p, train=False)


def _decode(g, tag, with_dir, post):
    cavs = CM.case_cavs(g, tag)
    data = {f"cav{k}": {"transformation_matrix": torch.from_numpy(c["tfm"]), "anchor_box": None} for k, c in enumerate(cavs)}
    out = {}
    for k, c in enumerate(cavs):
        out[f"cav{k}"] = {"cls_preds": torch.from_numpy(c["cls"]).to(DEV), "reg_preds": torch.from_numpy(c["boxes"]).to(DEV)}
        if with_dir:
            out[f"cav{k}"]["dir_preds"] = torch.from_numpy(c["dir"]).to(DEV)
    calls = {}
    ops.TIMING = calls
    try:
        with torch.no_grad():
            pred, score = post.post_process(data, out)
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    return pred.cpu().numpy(), score.cpu().numpy(), sorted(calls)


@pytest.mark.parametrize("tag,with_dir", [("d", True), ("n", False), ("m", True)])
def test_post_process_matches_reference(g, tag, with_dir):
    pred, score, calls = _decode(g, tag, with_dir, _post(g))
    want_pred, want_score = g[f"{tag}_pred"], g[f"{tag}_score"]
    assert ("center_decode_nms" in calls) == (tag != "m")              # one cav: the kernel; the late form: the tensor path
    assert pred.shape == want_pred.shape and score.shape == want_score.shape
    s_err = float(np.abs(score.astype(np.float64) - want_score).max() / want_score.max())
    c_err = float(np.abs(pred.astype(np.float64) - want_pred).max())
    print(f"decode {tag}: {pred.shape[0]} boxes, score error {s_err:.3e}, corner error {c_err:.3e}")
    assert np.all(np.abs(score.astype(np.float64) - want_score) <= 1e-6 * want_score)      # set and order: scores are distinct
    assert c_err <= 1e-4


def test_decode_without_survivors_returns_none(g):
    c = CM.case_cavs(g, "d")[0]
    cls = torch.full((1, 1, 16, 16), -8.0, device=DEV)
    post = _post(g)
    with torch.no_grad():
        pred, score = post.post_process({"ego": {"transformation_matrix": torch.from_numpy(c["tfm"]), "anchor_box": None}},
                                        {"ego": {"cls_preds": cls, "reg_preds": torch.from_numpy(c["boxes"]).to(DEV)}})
    assert pred is None and score is None


def _model(fusion):
    return fill_module(train_utils.create_model(configs.lidar_centerpoint(fusion, M_RANGE))).to(DEV).eval()


def _lidar(g):
    return {"voxel_features": torch.from_numpy(g["m3_voxel_features"]).to(DEV),
            "voxel_coords": torch.from_numpy(g["m3_voxel_coords"]).to(torch.int32).to(DEV),
            "voxel_num_points": torch.from_numpy(g["m3_voxel_num_points"]).to(torch.int32).to(DEV)}


@pytest.mark.parametrize("fusion,tag", [("max", "fused"), (None, "single")])
def test_models_match_the_reference_head_maps(g, fusion, tag):
    model = _model(fusion)
    data = {"processed_lidar": _lidar(g), "record_len": torch.tensor([3]),
            "pairwise_t_matrix": torch.from_numpy(g["m3_pairwise"]).to(DEV)}
    with torch.no_grad():
        out = model(data)
    assert sorted(out) == ["bbox_preds", "cls_preds", "reg_preds"]
    for key, name in (("cls_preds", "cls"), ("bbox_preds", "bbox"), ("reg_preds", "reg")):
        want = g[f"m3_{tag}_{name}"]
        assert tuple(out[key].shape) == want.shape
        err = _rel(out[key].cpu().numpy(), want)
        print(f"{tag} {key}: relative error {err:.3e}")
        assert err <= 1e-3


@pytest.mark.parametrize("fusion", ["max", None])
def test_one_training_step_gives_finite_gradients(g, fusion):
    hypes = configs.lidar_centerpoint(fusion, M_RANGE)
    hypes["loss"]["args"]["target_assigner_config"]["max_objs"] = 16
    model = _model(fusion).train()
    crit = train_utils.create_loss(hypes)
    n = 1 if fusion else 3
    rng = np.random.default_rng(11)
    boxes = np.zeros((n, 20, 7), np.float32)
    boxes[:, :6] = np.concatenate([rng.uniform(-12, 12, (n, 6, 2)), rng.uniform(-1.5, -0.5, (n, 6, 1)),
                                   rng.uniform(1.4, 4.0, (n, 6, 3)), rng.uniform(-3, 3, (n, 6, 1))], axis=2)
    mask = np.zeros((n, 20), np.float32)
    mask[:, :6] = 1
    data = {"processed_lidar": _lidar(g), "record_len": torch.tensor([3]),
            "pairwise_t_matrix": torch.from_numpy(g["m3_pairwise"]).to(DEV)}
    model.zero_grad()
    calls = {}
    ops.TIMING = calls
    try:
        out = model(data)
        total = crit(out, {"object_bbx_center": torch.from_numpy(boxes).to(DEV), "object_bbx_mask": torch.from_numpy(mask).to(DEV)})
        total.backward()
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert "center_loss" in calls and "center_boxes" in calls and bool(torch.isfinite(total))
    assert not out["reg_preds"].requires_grad and out["bbox_preds"].requires_grad
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(model.reg_head.weight.grad.abs().max()) > 0 and float(model.cls_head.weight.grad.abs().max()) > 0
