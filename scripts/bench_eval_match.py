"""AP evaluation per frame, three thresholds (0.3 / 0.5 / 0.7), three paths on the same GPU and the same seeded frames:
  (i)   fused: heal_eval_match, all thresholds in one launch pair
          fused_host_read   caluclate_tp_fp_multi: the launch pair + one host read (host wall time, ends in a synchronise)
          fused_add         DeviceResultStat.add: no host read (device events around a batch of appends)
          fused_kernels     the launch pair alone as a captured graph replays it (ops.graph_period_ms)
  (ii)  fallback: one heal_quad_iou launch + a host read + the numpy loop (HEAL_EVAL_FUSED=0; host wall time)
  (iii) per_detection: what install_as_opencood served before this module existed -- the reference loop
        (eval_utils.py:67-87) over common_utils.compute_iou, one heal_quad_iou launch with an upload and a synchronous
        read-back per detection and threshold; restated here (host wall time)
at 100 detections x 30 ground-truth boxes (a typical frame) and 1000 x 150 (the limits in use).  Every path is warmed up; the
paths alternate over ROUNDS rounds; medians with (min, max).  All paths must give the same TP / FP lists.

    python scripts/bench_eval_match.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import ops  # noqa: E402
from heal_amd.opencood.utils import common_utils, eval_utils as E  # noqa: E402

THR = (0.3, 0.5, 0.7)
SHAPES = [(100, 30), (1000, 150)]
ROUNDS = 5


def corners(boxes):
    x, y, z, h, w, l, yaw = (boxes[:, i] for i in range(7))
    c, s = np.cos(yaw), np.sin(yaw)
    sx, sy = np.array([1, 1, -1, -1]), np.array([1, -1, -1, 1])
    px = x[:, None] + 0.5 * (l[:, None] * sx * c[:, None] - w[:, None] * sy * s[:, None])
    py = y[:, None] + 0.5 * (l[:, None] * sx * s[:, None] + w[:, None] * sy * c[:, None])
    lo = np.stack([px, py, np.repeat((z - h / 2)[:, None], 4, 1)], -1)
    hi = np.stack([px, py, np.repeat((z + h / 2)[:, None], 4, 1)], -1)
    return np.concatenate([lo, hi], 1).astype(np.float32)


def frame(seed, n, m):
    """m cars spread over a 200 m square; two thirds of the detections jittered off a car, the rest clutter."""
    rng = np.random.default_rng(seed)
    cars = np.stack([rng.uniform(-100, 100, m), rng.uniform(-100, 100, m), np.full(m, -1.0), rng.uniform(1.4, 1.8, m),
                     rng.uniform(1.7, 2.2, m), rng.uniform(3.8, 5.0, m), rng.uniform(-np.pi, np.pi, m)], 1)
    det = cars[rng.integers(0, m, n)].copy()
    det[:, :2] += rng.normal(0, 1, (n, 1)) * rng.choice([0.1, 0.4, 30.0], (n, 1))
    return corners(det), rng.permutation(n).astype(np.float32) / n, corners(cars)


def per_detection(det, score, gt, stat):
    """The reference's caluclate_tp_fp body (eval_utils.py:57-91) over this package's host mirrors, once per threshold."""
    for thr in THR:
        fp, tp = [], []
        d, s, g = (common_utils.torch_tensor_to_numpy(t) for t in (det, score, gt))
        order = np.argsort(-s)
        s = s[order]
        det_polys, gt_polys = list(common_utils.convert_format(d)), list(common_utils.convert_format(g))
        for i in range(order.shape[0]):
            ious = common_utils.compute_iou(det_polys[order[i]], gt_polys)
            if len(gt_polys) == 0 or np.max(ious) < thr:
                fp.append(1)
                tp.append(0)
                continue
            fp.append(0)
            tp.append(1)
            gt_polys.pop(int(np.argmax(ious)))
        stat[thr]['score'] += s.tolist()
        stat[thr]['fp'] += fp
        stat[thr]['tp'] += tp
        stat[thr]['gt'] += g.shape[0]


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def main():
    out = {"device": torch.cuda.get_device_name(0), "thresholds": list(THR)}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    for n, m in SHAPES:
        det, score, gt = (torch.from_numpy(a).cuda() for a in frame(n + m, n, m))
        iters = 200 if n <= 100 else 50
        acc = E.DeviceResultStat(THR, capacity=n * iters)

        def fused_add():
            acc.buffers["cursor"].zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                acc.add(det, score, gt)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        def host_path(fused):
            def run():
                os.environ["HEAL_EVAL_FUSED"] = "1" if fused else "0"
                return wall_ms(lambda: E.caluclate_tp_fp_multi(det, score, gt, E.new_result_stat(THR), THR), iters)
            return run

        paths = {
            "fused_host_read": host_path(True),
            "fused_add": fused_add,
            "fused_kernels": lambda: ops.graph_period_ms(lambda: ops.eval_match(det, score, gt, THR, sync=False), reps=20, iters=10),
            "fallback_quad_iou_numpy": host_path(False),
            "per_detection_compute_iou": lambda: wall_ms(lambda: per_detection(det, score, gt, E.new_result_stat(THR)),
                                                         5 if n <= 100 else 2),
        }
        stats = {}
        for fused in ("1", "0"):                                     # the answers first: every path, the same lists
            os.environ["HEAL_EVAL_FUSED"] = fused
            stats[fused] = E.new_result_stat(THR)
            E.caluclate_tp_fp_multi(det, score, gt, stats[fused], THR)
        stats["ref"] = E.new_result_stat(THR)
        per_detection(det, score, gt, stats["ref"])
        acc.add(det, score, gt)
        same = stats["1"] == stats["0"] == stats["ref"] == acc.result_stat()
        times = {k: [] for k in paths}
        for k, fn in paths.items():                                  # warm-up of every path at this shape
            fn()
        for _ in range(ROUNDS):
            for k, fn in paths.items():
                times[k].append(fn())
        os.environ["HEAL_EVAL_FUSED"] = "1"
        row = {k: med(v) for k, v in times.items()}
        row["tp_per_threshold"] = [int(sum(stats["1"][t]["tp"])) for t in THR]
        row["all_paths_same_lists"] = bool(same)
        row["speedup_fused_over_fallback"] = round(row["fallback_quad_iou_numpy"]["median_us"] / row["fused_host_read"]["median_us"], 2)
        row["speedup_fused_over_per_detection"] = round(row["per_detection_compute_iou"]["median_us"]
                                                        / row["fused_host_read"]["median_us"], 1)
        out[f"{n}x{m}"] = row
        print(f"{n}x{m}", row, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0 if all(out[f"{n}x{m}"]["all_paths_same_lists"] for n, m in SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
