"""Generate tests/golden/unc_loss.npz and tests/golden/unc_post.npz by IMPORTING the reference (build container only).

    python -m tests.golden.gen_unc_golden

CoAlign's first stage: the criterion opencood/loss/point_pillar_uncertainty_loss.py, the post-processor
opencood/data_utils/post_processor/uncertainty_voxel_postprocessor.py and the state_dict names of
opencood/models/point_pillar_uncertainty.py.  Inputs and recorded outputs only.  The reference's d3d.mathh.i0e_cuda is not
installed: a stub module hands it torch.special.i0e, the same function.

unc_loss.npz -- the REFERENCE's PointPillarUncertaintyLoss.forward in float32 on the CPU for the five configurations of
tests/golden/unc_cases.py on 2 x 9 x 15 maps with two anchors: the inputs, loss_dict, and the autograd gradients of the total
with respect to the four (three) head maps.  s is drawn from [-4, 4] (asserted), so the reference's own exp(kappa) is finite.
`state_dict_keys`: the reference model's parameter and buffer names for configs.lidar_uncertainty's own arguments.

unc_post.npz -- post_process(..., return_uncertainty=True) on two cavs (a 16 x 16 and a 12 x 16 grid, their own poses and anchor
tables, dim 3) and on the first of them alone, and post_process_stage1 on a batch of two 16 x 16 samples.  Asserted on what is
written: no pairwise IoU among the NMS candidates within 1e-3 of nms_thresh, no score within 1e-4 of the score threshold (and,
for post_process, the geometric margins of tests/golden/late_margins.py)."""
import copy

import numpy as np
import torch

from heal_amd import configs, synth
from oracle import cref
from tests.golden import late_margins as M
from tests.golden import ref_import as R
from tests.golden import unc_cases as U
from tests.golden.gen_golden import save

GT_RANGE = [-8.0, -8.0, -3.0, 8.0, 8.0, 1.0]
SQ, RECT = [-6.4, -6.4, -3, 6.4, 6.4, 1], [-6.4, -4.8, -3, 6.4, 4.8, 1]
THR_MARGIN = 1e-4


def install():
    R.install()
    d3d = R._stub("d3d")
    d3d.mathh = R._stub("d3d.mathh", i0e_cuda=torch.special.i0e)


# ---- criterion ------------------------------------------------------------------------------------------------------------------
def gen_loss():
    L = R.ref("opencood.loss.point_pillar_uncertainty_loss")
    out = {}
    for tag, (dim, _, _, _, with_dir) in U.CONFIGS.items():
        maps, tgt = U.golden_inputs(tag)
        assert float(maps["unc_preds"].abs().max()) <= U.S_RANGE
        if not with_dir:
            del maps["dir_preds"]
        crit = L.PointPillarUncertaintyLoss(U.loss_args(tag))
        leafs = {k: v.clone().requires_grad_(True) for k, v in maps.items()}
        total = crit(dict(leafs), {k: v.clone() for k, v in tgt.items()})
        total.backward()
        assert bool(torch.isfinite(total)) and total.dtype == torch.float32
        for k, v in {**maps, **tgt}.items():
            out[f"{tag}_{k}"] = v.numpy()
        for k, v in crit.loss_dict.items():
            out[f"{tag}_{k}"] = np.float32(v)
        for k, v in leafs.items():
            out[f"{tag}_grad_{k}"] = v.grad.numpy()
        assert float(leafs["unc_preds"].grad.abs().max()) > 0
        print(tag, {k: round(v, 6) for k, v in crit.loss_dict.items()})
    model = R.ref("opencood.models.point_pillar_uncertainty")
    args = copy.deepcopy(configs.lidar_uncertainty()["model"]["args"])
    args["point_pillar_scatter"]["grid_size"] = np.round(
        (np.array(args["lidar_range"][3:]) - np.array(args["lidar_range"][:3])) / np.array(args["voxel_size"])).astype(np.int64)
    out["state_dict_keys"] = np.array(list(model.PointPillarUncertainty(args).state_dict().keys()))
    save("unc_loss", **out)


# ---- post-processor --------------------------------------------------------------------------------------------------------------
def _post(lidar_range, W, H):
    up = R.ref("opencood.data_utils.post_processor.uncertainty_voxel_postprocessor")
    p = copy.deepcopy(configs.lidar_uncertainty(lidar_range)["postprocess"])
    p["anchor_args"].update({"W": W, "H": H, "cav_lidar_range": list(lidar_range)})
    p["gt_range"] = list(GT_RANGE)
    return up.UncertaintyVoxelPostprocessor(p, train=False)


def _unc_map(rng, cav, dim):
    A, H, W = cav["cls"].shape[1:]
    cav["unc"] = rng.uniform(-U.S_RANGE, U.S_RANGE, (1, dim * A, H, W)).astype(np.float32)


def _iou_margin(corners, scores, nms_thr):
    """Indices (lower-scored box of the pair) of candidate pairs whose IoU lies within IOU_MARGIN of nms_thr."""
    order = np.argsort(scores, kind="stable")[::-1][:M.TOP]
    quads = np.ascontiguousarray(corners[order][:, :4, :2], np.float32)
    iou = cref.quad_iou(quads, quads) if len(order) else np.zeros((0, 0), np.float32)
    _, j = np.nonzero(np.triu(np.abs(iou.astype(np.float64) - nms_thr) < M.IOU_MARGIN, 1))
    return order[j]


def _assert_post_margins(cavs, params):
    bad, info = M.offenders(cavs, *params)
    thr = params[0]
    every = M.pooled_candidates(cavs, thr, params[1], params[2])[4]
    assert not bad and float(np.abs(every.astype(np.float64) - thr).min()) >= THR_MARGIN, (bad, info)
    return info


def _reference_post(cavs, post):
    data = {f"cav{k}": {"transformation_matrix": torch.from_numpy(c["tfm"]), "anchor_box": torch.from_numpy(c["anchors"])}
            for k, c in enumerate(cavs)}
    out = {f"cav{k}": {"cls_preds": torch.from_numpy(c["cls"]), "reg_preds": torch.from_numpy(c["reg"]),
                       "unc_preds": torch.from_numpy(c["unc"]), "dir_preds": torch.from_numpy(c["dir"])}
           for k, c in enumerate(cavs)}
    with torch.no_grad():
        pred, score, unc = post.post_process(data, out, return_uncertainty=True)
    return pred.numpy(), score.numpy(), unc.numpy()


def gen_post():
    rng = np.random.default_rng(2026)
    post = _post(SQ, 32, 32)
    anchors_sq = post.generate_anchor_box()
    anchors_rect = _post(RECT, 32, 24).generate_anchor_box()
    assert anchors_sq.shape == (16, 16, 2, 7) and anchors_rect.shape == (12, 16, 2, 7)
    thr, nms = post.params["target_args"]["score_threshold"], post.params["nms_thresh"]
    doff, bins = post.params["dir_args"]["dir_offset"], post.params["dir_args"]["num_bins"]
    params = (thr, doff, bins, nms, GT_RANGE)
    out = {"gt_range": np.array(GT_RANGE), "score_thr": np.array(thr), "nms_thr": np.array(nms), "dir_offset": np.array(doff),
           "num_bins": np.array(bins), "sq_range": np.array(SQ), "rect_range": np.array(RECT)}
    # two cavs, pooled
    cavs = [M.make_cav(rng, anchors_sq, synth.x_to_world([0.5, -0.3, 0.05, 0.0, 12.0, 0.0]), 9),
            M.make_cav(rng, anchors_rect, synth.x_to_world([-1.5, 1.0, -0.1, 0.2, -65.0, 0.1]), 7)]
    M.deal_ladder(rng, cavs)
    for c in cavs:
        _unc_map(rng, c, 3)
    for tag, group in (("p", cavs), ("s", cavs[:1])):
        group = [dict(c, cls=c["cls"].copy()) for c in group]
        M.settle(group, *params)
        info = _assert_post_margins(group, params)
        pred, score, unc = _reference_post(group, post)
        print(tag, info, "kept", pred.shape[0])
        assert 0 < pred.shape[0] < info["passing"] and unc.shape == (pred.shape[0], 3)
        out[f"{tag}_n"] = np.array(len(group))
        for k, c in enumerate(group):
            for name in ("cls", "reg", "dir", "unc", "anchors", "tfm"):
                out[f"{tag}{k}_{name}"] = c[name]
        out[f"{tag}_pred"], out[f"{tag}_score"], out[f"{tag}_unc"] = pred, score, unc
    # stage 1: a batch of two samples on one grid, each in its own frame, NMS per sample, no filters
    eye = np.eye(4)
    batch = [M.make_cav(rng, anchors_sq, eye, 8), M.make_cav(rng, anchors_sq, eye, 6)]
    M.deal_ladder(rng, batch)
    for c in batch:
        _unc_map(rng, c, 3)
    for _ in range(50):
        dirty = False
        for c in batch:
            corners, scores, pooled, _, every = M.pooled_candidates([c], thr, doff, bins)
            assert float(np.abs(every.astype(np.float64) - thr).min()) >= THR_MARGIN
            for p in pooled[_iou_margin(corners, scores, nms)]:
                A, H, W = c["cls"].shape[1:]
                c["cls"][0, p % A, (p // A) // W, (p // A) % W] = M.BACKGROUND
                dirty = True
        if not dirty:
            break
    else:
        raise AssertionError("the stage-1 margins did not settle")
    stage1 = {k: torch.from_numpy(np.concatenate([c[n] for c in batch])) for k, n in
              (("cls_preds", "cls"), ("reg_preds", "reg"), ("unc_preds", "unc"), ("dir_preds", "dir"))}
    with torch.no_grad():
        corners, boxes, uncs = post.post_process_stage1(stage1, torch.from_numpy(anchors_sq))
    for k, v in stage1.items():
        out[f"st_{k}"] = v.numpy()
    out["st_anchors"] = anchors_sq
    for b in range(2):
        print("stage1 sample", b, "kept", corners[b].shape[0])
        assert corners[b].shape[0] > 0
        out[f"st_corners{b}"], out[f"st_boxes{b}"], out[f"st_unc{b}"] = corners[b].numpy(), boxes[b].numpy(), uncs[b].numpy()
    save("unc_post", **out)


if __name__ == "__main__":
    install()
    gen_loss()
    gen_post()
