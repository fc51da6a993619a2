"""CoAlign's box alignment: the device call (ops.pose_graph_align -> heal_pose_graph_align, two kernels) against this repository's
float64 host path (box_align_v2.box_alignment_relative_np, numpy Levenberg-Marquardt) on the same inputs.

  one frame      5 agents, ~40 boxes each (50 objects, each seen by an agent with probability 0.8), box noise 0.1 m / 0.02 rad,
                 pose noise 0.2 m / 0.2 degrees, uncertainties given
  batch of 8     eight such samples (other seeds) in one launch; the host path runs them one after the other

What is timed, in ROUNDS alternating rounds (medians with (min, max)):
  device call    the whole ops call -- list concatenation, fp64 conversion, offsets upload, the two launches -- by a host clock
                 around ITERS calls that end in a device synchronise, with the inputs already on the device
  device kernels the two kernels alone, by device events around the C call (ops.TIMING)
  host path      box_alignment_relative_np on numpy inputs, host clock
The baseline is the host mirror of THIS repository, not the reference's g2o path: g2o is not installed, so neither its time nor
its iterates were measured.  The LM iteration counts of both sides are reported per sample.  There is no speed threshold.

    python scripts/pose_graph_bench.py [out.json]        # default: profiles/pose_graph_bench.json
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import ops  # noqa: E402
from heal_amd.opencood.models.sub_modules import box_align_v2 as BA  # noqa: E402
from tests import posegraph_refs as R  # noqa: E402

ROUNDS, ITERS, WARMUP, HOST_ITERS = 5, 50, 5, 3


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def frame(seed):
    return R.scene(seed, 5, 50, box_noise=(0.1, 0.02), pose_noise=(0.2, 0.2), seen=0.8)


def measure(scenes):
    dev = "cuda"
    corners = [torch.from_numpy(c).to(dev) for s in scenes for c in s["corners"]]
    unc = [torch.from_numpy(u).to(dev) for s in scenes for u in s["unc"]]
    pose_np = np.concatenate([s["pose"] for s in scenes])
    pose = torch.from_numpy(pose_np).to(dev)
    rec = [s["pose"].shape[0] for s in scenes]
    host_corners = [c for s in scenes for c in s["corners"]]
    host_unc = [u for s in scenes for u in s["unc"]]

    def device_call():
        return ops.pose_graph_align(corners, pose, unc, rec)

    def device_period_ms():
        for _ in range(WARMUP):
            device_call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            device_call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / ITERS

    def host_period_ms():
        t0 = time.perf_counter()
        for _ in range(HOST_ITERS):
            BA.box_alignment_relative_np(host_corners, host_unc, pose_np, rec)
        return (time.perf_counter() - t0) * 1e3 / HOST_ITERS

    times = {"device_call": [], "host_path": []}
    for _ in range(ROUNDS):
        times["device_call"].append(device_period_ms())
        times["host_path"].append(host_period_ms())
    row = {k: med(v) for k, v in times.items()}
    kernel = []
    for _ in range(ROUNDS):
        calls = {}
        ops.TIMING = calls
        for _ in range(ITERS):
            device_call()
        torch.cuda.synchronize()
        ops.TIMING = None
        (name, (n, mean_ms)), = [(k, v) for k, v in _summary(calls).items() if k.startswith("pose_graph_align")]
        kernel.append(mean_ms)
    row["device_kernels"] = med(kernel)
    refined, stats, _ = ops.pose_graph_align(corners, pose, unc, rec, return_stats=True)
    torch.cuda.synchronize()
    host = [R.host_result(s) for s in scenes]
    want = np.concatenate([h["refined"] for h in host])
    row["boxes_per_sample"] = [sum(len(c) for c in s["corners"]) for s in scenes]
    row["landmarks_per_sample"] = [int(v) for v in stats["landmarks"].cpu()]
    row["edges_per_sample"] = [int(v) for v in stats["edges"].cpu()]
    row["lm_iterations_device"] = [int(v) for v in stats["iterations"].cpu()]
    row["lm_trial_steps_device"] = [int(v) for v in stats["trials"].cpu()]
    row["lm_iterations_host"] = [int(h["iterations"]) for h in host]
    row["status_device"] = [int(v) for v in stats["status"].cpu()]
    row["pose_disagreement_device_vs_host"] = R.pose_disagreement(refined.cpu().numpy(), want)
    row["host_over_device_call"] = round(row["host_path"]["median_us"] / row["device_call"]["median_us"], 2)
    return row


def _summary(calls):
    return {name: (len(evs), sum(e[0].elapsed_time(e[1]) for e in evs) / max(len(evs), 1)) for name, evs in calls.items()}


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["baseline"] = "this repository's numpy float64 host path (box_align_v2.box_alignment_relative_np); the reference's g2o path was not run"
    out["d_ref"] = R.d_ref()
    out["one_frame"] = measure([frame(1000)])
    print("one frame", out["one_frame"], flush=True)
    out["batch_of_8"] = measure([frame(1000 + k) for k in range(8)])
    print("batch of 8", out["batch_of_8"], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "pose_graph_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
