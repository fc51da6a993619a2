"""The margins and the coverage the AP-evaluation fixture (tests/golden/eval_match.npz) must keep: shared by the generator
(tests/golden/gen_golden_eval.py), which enforces and asserts them on what it writes, and by tests/test_eval_cpu.py, which
re-checks the committed file.

The reference's outcome (eval_utils.py:67-87) depends on `<` at a threshold, on np.argsort's order on ties and on np.argmax
between near-equal IoUs, and its shapely arithmetic differs from the fp64 clip by ulps, so a fixture is only a fair golden when
no decision sits on an edge:
  * scores are pairwise distinct by >= SCORE_MARGIN;
  * every pairwise IoU is >= IOU_MARGIN away from every threshold;
  * in every row, the two largest IoUs above the lowest threshold differ by >= IOU_MARGIN (the argmax is unambiguous).
Coverage (what makes the fixture tell the reference's matcher from its neighbours):
  * taken  -- detections that are FP at some threshold ONLY because every box they reach there was already matched;
  * popped -- detections that are TP on a box other than their overall best, because that one was taken (the VOC variant, which
              looks at the best box only, calls these FP);
  * the TP count differs between thresholds."""
import numpy as np

from oracle import cref

THRESHOLDS = (0.3, 0.5, 0.7)
SCORE_MARGIN = 1e-5
IOU_MARGIN = 1e-3
MIN_TAKEN, MIN_POPPED = 5, 3


def footprints(boxes):
    return np.ascontiguousarray(np.asarray(boxes, np.float32)[:, :4, :2])


def iou_matrix(det, gt):
    return cref.quad_iou(footprints(det), footprints(gt)).astype(np.float64)


def offenders(det, gt):
    """Detection rows that break an IoU margin."""
    iou = iou_matrix(det, gt)
    near = np.zeros(iou.shape[0], bool)
    for t in THRESHOLDS:
        near |= (np.abs(iou - t) < IOU_MARGIN).any(axis=1)
    top = -np.sort(-iou, axis=1)[:, :2]
    if top.shape[1] == 2:
        near |= (top[:, 1] > THRESHOLDS[0] - IOU_MARGIN) & (top[:, 0] - top[:, 1] < IOU_MARGIN)
    return np.nonzero(near)[0]


def min_score_gap(score):
    s = np.sort(np.asarray(score, np.float32).astype(np.float64))
    return float(np.diff(s).min()) if len(s) > 1 else float("inf")


def coverage(det, score, gt, match):
    """match: the matcher under test, (iou [n,m], thresholds, score) -> (order, tp [T,n], gt_index [T,n]).
    -> dict(taken, popped, tp_counts)."""
    iou = iou_matrix(det, gt).astype(np.float32)
    order, tp, gi = match(iou, THRESHOLDS, score)
    taken = popped = 0
    for t, thr in enumerate(THRESHOLDS):
        for r, i in enumerate(order):
            if tp[t, r] == 0 and iou[i].max() >= np.float32(thr):
                taken += 1
            if tp[t, r] == 1 and gi[t, r] != int(np.argmax(iou[i])):
                popped += 1
    return {"taken": taken, "popped": popped, "tp_counts": [int(v) for v in tp.sum(axis=1)]}


def check(det, score, gt, match):
    """Assert every margin and the coverage; -> the coverage dict."""
    assert min_score_gap(score) >= SCORE_MARGIN, min_score_gap(score)
    bad = offenders(det, gt)
    assert len(bad) == 0, f"detections {bad.tolist()} sit within {IOU_MARGIN} of a threshold or of a tie"
    cov = coverage(det, score, gt, match)
    assert cov["taken"] >= MIN_TAKEN and cov["popped"] >= MIN_POPPED and len(set(cov["tp_counts"])) > 1, cov
    return cov
