"""Numpy restatement of the pooled late-fusion candidates (voxel_postprocessor.py:277-380 with several cavs) and the margins
the late-fusion fixture must keep: shared by the generator (tests/golden/gen_golden_late.py), which asserts them on what it
writes, and by tests/test_late_decode_cpu.py, which re-checks the committed file.

The reference's tie order is implementation-defined (numpy's unstable argsort) and its torch arithmetic differs from the
kernel's by ulps, so a fixture is only a fair golden when no decision sits on an edge:
  * adjacent pooled passing scores differ by >= SCORE_MARGIN, no score lies within SCORE_MARGIN of the threshold;
  * no filter quantity (x_len, y_len, zmin, zmax, any corner vs gt_range) lies within GEOM_MARGIN of its limit;
  * no pair among the top-1000 has an IoU within IOU_MARGIN of nms_thresh.
These are 10x the comparison tolerances (scores 1e-6 relative, corners 1e-4; a 1e-4 corner shift moves the IoU of 2 x 4 m boxes
by a few 1e-4)."""
import numpy as np

from heal_amd.synth import BACKGROUND, deal_ladder, make_cav  # noqa: F401  (the case builders, used through this module)
from oracle import cref
from oracle import oracle_np as O

SCORE_MARGIN = 1e-5
GEOM_MARGIN = 1e-3
IOU_MARGIN = 1e-3
TOP = 1000
F32 = np.float32


def case_cavs(g, tag):
    """The cavs of case `tag` of the fixture: list of dicts cls [1,A,H,W], reg, dir, anchors [H,W,A,7], tfm [4,4]."""
    n = int(g[f"{tag}_n"])
    return [{k: np.asarray(g[f"{tag}{i}_{k}"]) for k in ("cls", "reg", "dir", "anchors", "tfm")} for i in range(n)]


def pooled_candidates(cavs, score_thr, dir_offset, num_bins):
    """Every above-threshold anchor of every cav, in pooled order (cav order, then anchor order), BEFORE the size / z filters:
    (corners [M,8,3] f32 in the ego frame, scores [M] f32, pooled index [M], agent [M], all scores of all anchors)."""
    corners, scores, pooled, agent, every = [], [], [], [], []
    off = 0
    for k, c in enumerate(cavs):
        cls = np.asarray(c["cls"], F32)
        prob = (F32(1) / (F32(1) + np.exp(-cls.transpose(0, 2, 3, 1)))).astype(F32).reshape(-1)
        every.append(prob)
        mask = prob > F32(score_thr)
        idx = np.nonzero(mask)[0]
        boxes = O.delta_to_boxes3d(c["reg"], c["anchors"])[mask]
        if len(boxes):
            dm = np.asarray(c["dir"], F32).transpose(0, 2, 3, 1).reshape(-1, num_bins)[mask]
            period = 2 * np.pi / num_bins
            rot = O.limit_period(boxes[:, 6] - F32(dir_offset), 0, period)
            boxes[:, 6] = rot + F32(dir_offset) + F32(period) * np.argmax(dm, axis=-1).astype(F32)
            boxes[:, 6] = O.limit_period(boxes[:, 6], 0.5, 2 * np.pi)
            corners.append(O.project_box3d(O.boxes_to_corners_3d_hwl(boxes), c["tfm"]))
            scores.append(prob[mask])
            pooled.append(off + idx)
            agent.append(np.full(len(idx), k))
        off += prob.size
    if not corners:
        return np.zeros((0, 8, 3), F32), np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.concatenate(every)
    return np.concatenate(corners), np.concatenate(scores), np.concatenate(pooled), np.concatenate(agent), np.concatenate(every)


def filter_quantities(corners):
    """x_len, y_len, zmin, zmax of box_utils.py:840-890 (remove_large_pred_bbx / remove_bbx_abnormal_z)."""
    x_len = corners[:, :, 0].max(1) - corners[:, :, 0].min(1)
    y_len = corners[:, :, 1].max(1) - corners[:, :, 1].min(1)
    return x_len, y_len, corners[:, :, 2].min(1), corners[:, :, 2].max(1)


def passes(corners):
    x_len, y_len, zmin, zmax = filter_quantities(corners)
    return (x_len <= 6) & (y_len <= 6) & (y_len != 0) & (zmin >= -3) & (zmax <= 1)


def offenders(cavs, score_thr, dir_offset, num_bins, nms_thr, gt_range):
    """Pooled indices of above-threshold candidates that break a margin (for a near-threshold IoU pair: the lower-scored box),
    plus a summary of the pool.  An empty list means the case keeps every margin."""
    corners, scores, pooled, agent, every = pooled_candidates(cavs, score_thr, dir_offset, num_bins)
    bad = set()
    near_thr = np.abs(every.astype(np.float64) - score_thr) < SCORE_MARGIN
    x_len, y_len, zmin, zmax = filter_quantities(corners.astype(np.float64))
    edge = ((np.abs(x_len - 6) < GEOM_MARGIN) | (np.abs(y_len - 6) < GEOM_MARGIN) | (np.abs(y_len) < GEOM_MARGIN)
            | (np.abs(zmin + 3) < GEOM_MARGIN) | (np.abs(zmax - 1) < GEOM_MARGIN))
    bad.update(pooled[edge].tolist())
    ok = passes(corners)
    pc, ps, pp, pa = corners[ok], scores[ok], pooled[ok], agent[ok]
    order = np.argsort(ps, kind="stable")[::-1]
    d = -np.diff(ps[order].astype(np.float64))
    close = np.nonzero(d < SCORE_MARGIN)[0]
    bad.update(pp[order[close + 1]].tolist())
    r = np.asarray(gt_range, np.float64)
    on_range = (np.abs(pc.astype(np.float64) - r[:3]) < GEOM_MARGIN) | (np.abs(pc.astype(np.float64) - r[3:]) < GEOM_MARGIN)
    bad.update(pp[on_range.any(axis=(1, 2))].tolist())
    top = order[:TOP]
    quads = np.ascontiguousarray(pc[top][:, :4, :2], F32)
    iou = cref.quad_iou(quads, quads) if len(top) else np.zeros((0, 0), F32)
    i, j = np.nonzero(np.triu(np.abs(iou.astype(np.float64) - nms_thr) < IOU_MARGIN, 1))
    bad.update(pp[top[j]].tolist())      # j > i: the lower-scored box of the pair
    info = {"above_threshold": int(len(scores)), "passing": int(ok.sum()), "near_threshold": int(near_thr.sum()),
            "per_agent_above": np.bincount(agent, minlength=len(cavs)).tolist(),
            "per_agent_passing": np.bincount(pa, minlength=len(cavs)).tolist(),
            "min_score_gap": float(d.min()) if len(d) else float("inf")}
    return sorted(bad), info


def expected_agents(cavs, pred_scores, score_thr, dir_offset, num_bins):
    """The source agent of every kept box, derived from the composition: scores are distinct, so a kept score names its cav."""
    corners, scores, pooled, agent, _ = pooled_candidates(cavs, score_thr, dir_offset, num_bins)
    ok = passes(corners)
    scores, agent = scores[ok], agent[ok]
    order = np.argsort(scores)
    pos = np.searchsorted(scores[order], pred_scores)
    pos = np.clip(pos, 0, len(order) - 1)
    left = np.clip(pos - 1, 0, len(order) - 1)
    nearer = np.where(np.abs(scores[order][left] - pred_scores) < np.abs(scores[order][pos] - pred_scores), left, pos)
    return agent[order][nearer]


# ---- a case that keeps the margins (the generator, and GPU tests that need a larger seeded case); make_cav and deal_ladder
# of heal_amd.synth build it, deal_ladder's default minimum step being 2 * SCORE_MARGIN ----------------------------------------
def settle(cavs, score_thr, dir_offset, num_bins, nms_thr, gt_range):
    """Demote margin offenders to background until none is left."""
    args = (score_thr, dir_offset, num_bins, nms_thr, gt_range)
    sizes = np.cumsum([0] + [c["cls"].size for c in cavs])
    for _ in range(50):
        bad, info = offenders(cavs, *args)
        if not bad:
            assert info["near_threshold"] == 0 and info["min_score_gap"] >= SCORE_MARGIN, info
            return info
        for p in bad:
            k = int(np.searchsorted(sizes, p, side="right") - 1)
            A, H, W = cavs[k]["cls"].shape[1:]
            j = p - sizes[k]                                           # anchor index: (h * W + w) * A + a
            cavs[k]["cls"][0, j % A, (j // A) // W, (j // A) % W] = BACKGROUND
    raise AssertionError("the margins did not settle")
