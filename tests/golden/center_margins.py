"""The margins the centre-head fixture (tests/golden/center_small.npz) must keep, and the numpy restatement of the anchor-free
candidates of VoxelPostprocessor.post_process (voxel_postprocessor.py:305-380 with 3-D reg_preds) that the decode margins need:
shared by the generator (tests/golden/gen_golden_center.py), which asserts them on what it writes, and by
tests/test_center_point_cpu.py, which re-checks the committed file.

Loss cases: the target assignment truncates fp32 quotients (the heat-map cell of a centre, the Gaussian radius) and compares a
sigmoid against the clamp of clip_sigmoid; a kernel and the reference may differ by an ulp there, so a fixture is only a fair
golden when no such decision sits on an edge:
  * every coor_x, coor_y of a row in use lies at least CELL_MARGIN from an integer;
  * every fp32 gaussian_radius of a sized row lies at least CELL_MARGIN from an integer;
  * no logit lies within LOGIT_MARGIN of +-CLAMP_EDGE = log((1 - 1e-4) / 1e-4), where the clamp starts;
  * no NaN anywhere.
Decode cases: the margins of tests/golden/late_margins.py (SCORE_MARGIN, GEOM_MARGIN, IOU_MARGIN), on the pooled candidates."""
import numpy as np
import torch

from oracle import cref
from oracle import oracle_np as O
from tests.golden.late_margins import GEOM_MARGIN, IOU_MARGIN, SCORE_MARGIN, TOP, filter_quantities, passes

CELL_MARGIN = 0.02
LOGIT_MARGIN = 0.01
CLAMP_EDGE = float(np.log((1 - 1e-4) / 1e-4))      # 9.2102
F32 = np.float32

LOSS_CASES = ("a_", "b_", "c_")


def loss_case(g, prefix):
    """The stored inputs and settings of one loss case."""
    keys = ("cls", "bbox", "boxes", "mask", "range", "voxel", "factor", "max_objs", "min_radius", "overlap", "code_weights",
            "cls_weight", "loc_weight")
    return {k: np.asarray(g[prefix + k]) for k in keys}


def loss_args(c):
    """The `args` of CenterPointLoss for a case of loss_case()."""
    return {"cls_weight": float(c["cls_weight"]), "loc_weight": float(c["loc_weight"]),
            "code_weights": [float(v) for v in c["code_weights"]],
            "target_assigner_config": {"max_objs": int(c["max_objs"]), "min_radius": int(c["min_radius"]),
                                       "gaussian_overlap": float(c["overlap"]), "out_size_factor": int(c["factor"]),
                                       "voxel_size": [float(v) for v in c["voxel"]],
                                       "cav_lidar_range": [float(v) for v in c["range"]]}}


def loss_margins(c, gaussian_radius):
    """(smallest distance of a coor_x / coor_y in use from an integer, the same of a gaussian_radius, smallest distance of a
    logit from the clamp edge, everything finite).  `gaussian_radius((h, w), min_overlap)` is the fp32 tensor function under
    test or the reference's; the fp32 chains are the ones of center_point_loss.py:419-431."""
    boxes, mask = torch.from_numpy(c["boxes"].astype(F32)), c["mask"]
    r, v, f = [float(x) for x in c["range"]], [float(x) for x in c["voxel"]], int(c["factor"])
    cell, rad = np.inf, np.inf
    for b in range(boxes.shape[0]):
        for k in range(min(int(mask[b].sum()), int(c["max_objs"]), boxes.shape[1])):
            t = boxes[b, k]
            h, w = t[3] / v[0] / f, t[4] / v[1] / f
            if not (h > 0 and w > 0):
                continue
            for coor in ((t[0] - r[0]) / v[0] / f, (t[1] - r[1]) / v[1] / f):
                cell = min(cell, abs(float(coor) - round(float(coor))))
            radius = float(gaussian_radius((h, w), min_overlap=float(c["overlap"])))
            rad = min(rad, abs(radius - round(radius)))
    logit = float(np.abs(np.abs(c["cls"].astype(np.float64)) - CLAMP_EDGE).min())
    finite = all(bool(np.isfinite(c[k]).all()) for k in ("cls", "bbox", "boxes"))
    return cell, rad, logit, finite


# ---- decode ---------------------------------------------------------------------------------------------------------------------
def case_cavs(g, tag):
    """The cavs of decode case `tag`: list of dicts cls [1,1,H,W], boxes [1,H*W,7], dir [1,2,H,W], tfm [4,4]."""
    n = int(g[f"{tag}_n"])
    return [{k: np.asarray(g[f"{tag}{i}_{k}"]) for k in ("cls", "boxes", "dir", "tfm")} for i in range(n)]


def pooled_candidates(cavs, score_thr, dir_offset, num_bins, with_dir):
    """Every above-threshold cell of every cav in pooled order, BEFORE the size / z filters:
    (corners [M,8,3] f32 in the ego frame, scores [M] f32, pooled index [M], all scores of all cells)."""
    corners, scores, pooled, every = [], [], [], []
    off = 0
    for c in cavs:
        cls = np.asarray(c["cls"], F32)
        prob = (F32(1) / (F32(1) + np.exp(-cls.transpose(0, 2, 3, 1)))).astype(F32).reshape(-1)
        every.append(prob)
        mask = prob > F32(score_thr)
        boxes = np.asarray(c["boxes"], F32).reshape(-1, 7)[mask].copy()
        if len(boxes):
            if with_dir:
                dm = np.asarray(c["dir"], F32).transpose(0, 2, 3, 1).reshape(-1, num_bins)[mask]
                period = 2 * np.pi / num_bins
                rot = O.limit_period(boxes[:, 6] - F32(dir_offset), 0, period)
                boxes[:, 6] = rot + F32(dir_offset) + F32(period) * np.argmax(dm, axis=-1).astype(F32)
                boxes[:, 6] = O.limit_period(boxes[:, 6], 0.5, 2 * np.pi)
            corners.append(O.project_box3d(O.boxes_to_corners_3d_hwl(boxes), c["tfm"]))
            scores.append(prob[mask])
            pooled.append(off + np.nonzero(mask)[0])
        off += prob.size
    if not corners:
        return np.zeros((0, 8, 3), F32), np.zeros(0, F32), np.zeros(0, np.int64), np.concatenate(every)
    return np.concatenate(corners), np.concatenate(scores), np.concatenate(pooled), np.concatenate(every)


def offenders(cavs, score_thr, dir_offset, num_bins, nms_thr, gt_range, with_dir):
    """Pooled indices of above-threshold cells that break a margin of late_margins.py (for a near-threshold IoU pair: the
    lower-scored box), plus a summary.  An empty list means the case keeps every margin."""
    corners, scores, pooled, every = pooled_candidates(cavs, score_thr, dir_offset, num_bins, with_dir)
    bad = set()
    near_thr = np.abs(every.astype(np.float64) - score_thr) < SCORE_MARGIN
    x_len, y_len, zmin, zmax = filter_quantities(corners.astype(np.float64))
    edge = ((np.abs(x_len - 6) < GEOM_MARGIN) | (np.abs(y_len - 6) < GEOM_MARGIN) | (np.abs(y_len) < GEOM_MARGIN)
            | (np.abs(zmin + 3) < GEOM_MARGIN) | (np.abs(zmax - 1) < GEOM_MARGIN))
    bad.update(pooled[edge].tolist())
    ok = passes(corners)
    pc, ps, pp = corners[ok], scores[ok], pooled[ok]
    order = np.argsort(ps, kind="stable")[::-1]
    d = -np.diff(ps[order].astype(np.float64))
    bad.update(pp[order[np.nonzero(d < SCORE_MARGIN)[0] + 1]].tolist())
    r = np.asarray(gt_range, np.float64)
    on_range = (np.abs(pc.astype(np.float64) - r[:3]) < GEOM_MARGIN) | (np.abs(pc.astype(np.float64) - r[3:]) < GEOM_MARGIN)
    bad.update(pp[on_range.any(axis=(1, 2))].tolist())
    top = order[:TOP]
    quads = np.ascontiguousarray(pc[top][:, :4, :2], F32)
    iou = cref.quad_iou(quads, quads) if len(top) else np.zeros((0, 0), F32)
    i, j = np.nonzero(np.triu(np.abs(iou.astype(np.float64) - nms_thr) < IOU_MARGIN, 1))
    bad.update(pp[top[j]].tolist())
    inside = ((pc >= r[:3]) & (pc <= r[3:])).all(axis=(1, 2))
    info = {"above_threshold": int(len(scores)), "passing": int(ok.sum()), "near_threshold": int(near_thr.sum()),
            "min_score_gap": float(d.min()) if len(d) else float("inf"),
            "pairs_above": int(np.triu(iou > nms_thr, 1).sum()), "pairs_overlapping_below": int(
                np.triu((iou > 0.01) & (iou < nms_thr), 1).sum()),
            "too_large": int(((x_len > 6) | (y_len > 6)).sum()), "bad_z": int(((zmin < -3) | (zmax > 1)).sum()),
            "out_of_range": int((~inside).sum())}
    return sorted(bad), info
