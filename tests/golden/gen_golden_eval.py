"""Generate tests/golden/eval_match.npz by running the REFERENCE's caluclate_tp_fp and calculate_ap
(opencood/utils/eval_utils.py:40-137; build container only, shapely replaced by ref_import's convex-quad stand-in) on two frames.

    python -m tests.golden.gen_golden_eval

Frame "a": about 130 detections x 40 ground-truth boxes.  Frame "b": about 300 x 70, so the ground-truth count crosses one wave.
Ground-truth boxes of car size; two jittered detections per box at mixed jitter scales; clutter detections; a few ADJACENT,
overlapping ground-truth pairs, each with a detection between them that scores below a detection sitting on its nearer box (so
the nearer box is taken first and the detection falls to the other one).

Detections that would put a decision on an edge are re-drawn until every margin of tests/golden/eval_margins.py holds; margins
and coverage are asserted on what is written.  The fixture stores the inputs and the reference's outputs, plus gt_index: the
matched box per TP from the restated loop (the reference does not report it), recorded only after that loop's tp / fp lists
have been checked equal to the reference's."""
import os

import numpy as np
import torch

from heal_amd.opencood.utils.eval_utils import _greedy_match
from tests.golden import eval_margins as M
from tests.golden import ref_import as R

OUT = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def corners(box):
    """(x, y, z, h, w, l, yaw) -> [8,3] f32: the footprint's four corners at the bottom (0..3), then at the top."""
    x, y, z, h, w, l, yaw = box
    c, s = np.cos(yaw), np.sin(yaw)
    fp = np.array([[l / 2, w / 2], [l / 2, -w / 2], [-l / 2, -w / 2], [-l / 2, w / 2]])
    xy = fp @ np.array([[c, s], [-s, c]]) + [x, y]
    return np.concatenate([np.c_[xy, np.full(4, z - h / 2)], np.c_[xy, np.full(4, z + h / 2)]]).astype(F32)


def jitter(rng, box, scale):
    b = np.array(box, np.float64)
    b[:2] += rng.normal(0, scale, 2)
    b[3:6] *= 1 + rng.normal(0, 0.1 * scale, 3)
    b[6] += rng.normal(0, 0.1 * scale)
    return b


def car(rng, x, y):
    return np.array([x, y, -1.0, 1.5 + 0.2 * rng.random(), 1.8 + 0.4 * rng.random(), 4.0 + 1.0 * rng.random(),
                     rng.uniform(-np.pi, np.pi)])


def make_frame(rng, n_single, n_pairs, n_clutter):
    """-> det [n,8,3], score [n], gt [m,8,3] (f32), every margin kept."""
    gt, draw = [], []                 # draw[i]() re-draws detection i
    half = 90.0
    cells = rng.permutation(18 * 18)[:n_single + n_pairs]          # one box (or pair) per 10 m cell: separate cars do not overlap
    centre = lambda c: (-half + 10 * (c % 18) + 5 + rng.uniform(-1, 1), -half + 10 * (c // 18) + 5 + rng.uniform(-1, 1))
    scales = (0.08, 0.25, 0.5, 0.9)
    for k in range(n_single):
        g = car(rng, *centre(cells[k]))
        gt.append(g)
        for _ in range(2):
            sc = scales[int(rng.integers(len(scales)))]
            draw.append(lambda g=g, sc=sc: jitter(rng, g, sc))
    before = []                        # (index of the detection on the nearer box, index of the detection in between)
    for k in range(n_pairs):
        a = car(rng, *centre(cells[n_single + k]))
        b = a.copy()
        side = rng.uniform(1.1, 1.4)                               # lateral offset: the two boxes overlap by a third or so
        b[0] += -np.sin(a[6]) * side
        b[1] += np.cos(a[6]) * side
        gt += [a, b]
        draw.append(lambda a=a: jitter(rng, a, 0.08))              # sits on a
        on_a = len(draw) - 1

        def between(a=a, b=b):
            f = rng.uniform(0.36, 0.46)                            # nearer a than b
            mid = a.copy()
            mid[:2] = a[:2] + f * (b[:2] - a[:2])
            return jitter(rng, mid, 0.03)
        draw.append(between)
        before.append((on_a, len(draw) - 1))
        if k % 2:                                                  # half of the pairs: a late detection on b, FP once b is taken
            draw.append(lambda b=b: jitter(rng, b, 0.08))
    for _ in range(n_clutter):
        draw.append(lambda: car(rng, rng.uniform(-half, half), rng.uniform(-half, half)))
    order = rng.permutation(len(gt))                               # the adjacent pairs are not neighbours in index order
    gt = np.stack([corners(gt[i]) for i in order])
    n = len(draw)
    det = np.stack([corners(d()) for d in draw])
    for _ in range(200):
        bad = M.offenders(det, gt)
        if len(bad) == 0:
            break
        for i in bad:
            det[i] = corners(draw[i]())
    else:
        raise AssertionError("the IoU margins did not settle")
    score = (0.05 + 0.9 * rng.permutation(n) / n).astype(F32)     # a ladder with steps of 0.9 / n >> SCORE_MARGIN
    for hi, lo in before:
        if score[hi] < score[lo]:
            score[hi], score[lo] = score[lo], score[hi]
    mix = rng.permutation(n)                                       # detection order is unrelated to how the frame was built
    return det[mix], score[mix], gt


def reference(eu, det, score, gt, stat):
    for thr in M.THRESHOLDS:
        eu.caluclate_tp_fp(torch.from_numpy(det), torch.from_numpy(score), torch.from_numpy(gt), stat, thr)


def record(out, tag, eu, stat):
    for k in ("tp", "fp", "score"):
        out[f"{tag}_{k}"] = np.array([stat[thr][k] for thr in M.THRESHOLDS])
    out[f"{tag}_gt"] = np.array([stat[thr]["gt"] for thr in M.THRESHOLDS])
    aps = [eu.calculate_ap(stat, thr) for thr in M.THRESHOLDS]
    out[f"{tag}_ap"] = np.array([a[0] for a in aps], np.float64)
    out[f"{tag}_mrec"] = np.array([a[1] for a in aps], np.float64)
    out[f"{tag}_mpre"] = np.array([a[2] for a in aps], np.float64)


def main():
    eu = R.ref("opencood.utils.eval_utils")
    rng = np.random.default_rng(2025)
    new_stat = lambda: {thr: {"tp": [], "fp": [], "gt": 0, "score": []} for thr in M.THRESHOLDS}
    out = {"thresholds": np.array(M.THRESHOLDS, np.float64)}
    run = new_stat()
    for tag, sizes in (("a", (30, 5, 55)), ("b", (54, 8, 170))):
        det, score, gt = make_frame(rng, *sizes)
        cov = M.check(det, score, gt, _greedy_match)
        stat = new_stat()
        reference(eu, det, score, gt, stat)
        reference(eu, det, score, gt, run)
        order, tp, gi = _greedy_match(M.iou_matrix(det, gt).astype(F32), M.THRESHOLDS, score)
        for t, thr in enumerate(M.THRESHOLDS):                     # the restated loop against the reference, before gt_index is kept
            assert stat[thr]["tp"] == tp[t].tolist() and stat[thr]["fp"] == (1 - tp[t].astype(int)).tolist()
            assert stat[thr]["score"] == score[order].tolist() and stat[thr]["gt"] == len(gt)
        out.update({f"{tag}_det": det, f"{tag}_det_score": score, f"{tag}_gt_boxes": gt, f"{tag}_order": order, f"{tag}_gt_index": gi})
        record(out, tag, eu, stat)
        print(tag, det.shape, gt.shape, cov, "ap", out[f"{tag}_ap"])
    record(out, "run", eu, run)                                    # both frames accumulated, as an inference run does
    print("run ap", out["run_ap"])
    path = os.path.join(OUT, "eval_match.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
