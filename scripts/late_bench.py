"""Late fusion: the pooled decode + NMS kernel chain (heal_decode_nms_agents) against what it replaces, and the late scene step.

Decode, per configuration (full-size maps, 256 x 256 x 2 anchors per agent, heads built to about 600 candidates per agent; one
case with more than 4096 pooled candidates, which takes the radix-select path):
  (a) agents    ops.decode_nms_agents(sync=False): one launch chain for all agents;
  (b) fallback  VoxelPostprocessor._post_process_multi: the per-cav tensor path (HEAL_LATE_FUSED=0), host synchronisations included;
  (c) k8_each   n sequential ops.decode_nms(sync=False) calls, one per agent: a floor for the front end (it runs n NMS tails
                and pools nothing, so it is not a late-fusion result).
`event_us`: a HIP event pair around the eager call after warm-up, median with (min, max) -- the only timing (b) allows, since its
host reads cannot be captured; `graph_us` for (a) and (c): ops.graph_period_ms, the device time as a captured graph runs it.

Scene: configs.m1_late on the full range, 5 LiDAR agents, heads calibrated to about 600 candidates per agent: the eager
LateScenePipeline.step, the graph replay, and the per-cav loop of inference_late_fusion + post_process on the tensor path
(HEAL_LATE_FUSED=0), as wall-clock medians per scene and scenes/s.

    python scripts/late_bench.py [out.json] [--decode-only | --step-only]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import configs, ops, synth  # noqa: E402
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor  # noqa: E402

DECODE_CASES = [("n2", 2, 43), ("n3", 3, 43), ("n5", 5, 43), ("n5_select_path", 5, 95)]   # name, agents, 3 x 3 clusters per agent
ROUNDS = 3


def spread(ts, scale=1e3):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * scale, 1), "min_us": round(ts[0] * scale, 1), "max_us": round(ts[-1] * scale, 1)}


def event_ms(fn, warm=3, iters=15):
    for _ in range(warm):
        fn()
    st = torch.cuda.current_stream()
    st.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def wall_ms(fn, warm=3, iters=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def decode_cases(out):
    post = VoxelPostprocessor(configs.m1_late()["postprocess"], train=False)
    anchors_np = post.generate_anchor_box()
    anchors = torch.from_numpy(anchors_np).cuda()
    anchors32 = anchors.float().contiguous()
    p = post.params
    args = (p["target_args"]["score_threshold"], p["dir_args"]["dir_offset"], p["dir_args"]["num_bins"], p["nms_thresh"])
    faster = True
    for name, n, clusters in DECODE_CASES:
        rng = np.random.default_rng(100 + n + clusters)
        tfms = synth.pairwise_t_matrix(synth.agent_poses(40 + n, n), n)[:n, 0]
        cavs = [synth.make_cav(rng, anchors_np, tfms[k], clusters) for k in range(n)]
        synth.deal_ladder(rng, cavs)
        cls = torch.from_numpy(np.concatenate([c["cls"] for c in cavs])).cuda()
        reg = torch.from_numpy(np.concatenate([c["reg"] for c in cavs])).cuda()
        dirs = torch.from_numpy(np.concatenate([c["dir"] for c in cavs])).cuda()
        t_dev = torch.from_numpy(tfms).cuda()
        lists = ([cls[k:k + 1] for k in range(n)], [reg[k:k + 1] for k in range(n)], [dirs[k:k + 1] for k in range(n)])
        data = {k: {"transformation_matrix": t_dev[k].float(), "anchor_box": anchors} for k in range(n)}
        outs = {k: {"cls_preds": lists[0][k], "reg_preds": lists[1][k], "dir_preds": lists[2][k]} for k in range(n)}

        def agents():
            return ops.decode_nms_agents(*lists, [anchors32] * n, t_dev, *args, p["gt_range"], sync=False)

        def fallback():
            return post._post_process_multi(data, outs)

        def k8_each():
            for k in range(n):
                ops.decode_nms(lists[0][k], lists[1][k], lists[2][k], anchors32, *args, tfms[k].astype(np.float32), p["gt_range"],
                               sync=False)

        c, s, cnt = agents()
        fb, fs = fallback()
        kept = int(cnt.item())
        row = {"agents": n, "anchors_pooled": int(n * anchors_np.size // 7),
               "candidates_above_threshold": int(sum(int(x["_cand"].sum()) for x in cavs)), "boxes_kept": kept,
               "same_boxes_as_fallback": bool(fb is not None and fb.shape[0] == kept
                                              and torch.allclose(c[:kept], fb, rtol=1e-4, atol=1e-4))}
        ev = {"agents": [], "fallback": [], "k8_each": []}
        gr = {"agents": [], "k8_each": []}
        for _ in range(ROUNDS):                            # alternating rounds: every path sees the same neighbours on the machine
            for key, fn in (("agents", agents), ("fallback", fallback), ("k8_each", k8_each)):
                ev[key] += event_ms(fn, iters=10)
            for key, fn in (("agents", agents), ("k8_each", k8_each)):
                gr[key].append(ops.graph_period_ms(fn, reps=10, iters=5))
        row["event_us"] = {k: spread(v) for k, v in ev.items()}
        row["graph_us"] = {k: spread(v) for k, v in gr.items()}
        row["speedup_over_fallback"] = round(row["event_us"]["fallback"]["median_us"] / row["event_us"]["agents"]["median_us"], 2)
        faster = faster and row["event_us"]["agents"]["median_us"] < row["event_us"]["fallback"]["median_us"]
        out[name] = row
        print(name, row, flush=True)
    out["fused_faster_than_fallback_at_every_configuration"] = faster
    return faster


def scene_step(out):
    from heal_amd.opencood.tools import inference_utils as iu
    from heal_amd.pipeline import LateScenePipeline, Scene
    dev = torch.device("cuda:0")
    pipe = LateScenePipeline(configs.m1_late(), dev, seed=3)
    scene = Scene(5, seed=7, device=dev)
    pipe.calibrate_cls_bias(scene, target_candidates=600)
    n = scene.n_agents
    batch = {k: {"inputs_m1": {"points": [scene.points[k]]}, "anchor_box": pipe.anchor_box,
                 "transformation_matrix": torch.from_numpy(scene.pairwise[0, k, 0]).float().to(dev)} for k in range(n)}

    class DS:
        def post_process(self, b, o):
            return pipe.post.post_process(b, o) + (None,)

    def loop():
        return iu.inference_late_fusion(batch, pipe.model, DS())

    with torch.no_grad():
        boxes, _ = pipe.step(scene)
        row = {"agents": n, "boxes_kept": 0 if boxes is None else int(boxes.shape[0])}
        times = {"eager_step": [], "per_cav_loop_fused_post": [], "per_cav_loop_tensor_post": [], "graph_replay": []}
        pipe.capture(scene)
        for _ in range(ROUNDS):
            times["eager_step"] += wall_ms(lambda: pipe.step(scene), iters=8)
            os.environ["HEAL_LATE_FUSED"] = "1"
            times["per_cav_loop_fused_post"] += wall_ms(loop, iters=8)
            os.environ["HEAL_LATE_FUSED"] = "0"
            times["per_cav_loop_tensor_post"] += wall_ms(loop, iters=8)
            os.environ["HEAL_LATE_FUSED"] = "1"
            times["graph_replay"] += wall_ms(lambda: pipe.replay(scene), iters=8)
    for k, v in times.items():
        row[k] = spread(v)
        row[k]["scenes_per_s"] = round(1e6 / row[k]["median_us"], 1)
    out["scene_5_lidar_agents"] = row
    print("scene_5_lidar_agents", row, flush=True)


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    if "--step-only" not in sys.argv:
        with torch.no_grad():
            decode_cases(out)
    if "--decode-only" not in sys.argv:
        scene_step(out)
    if argv:
        with open(argv[0], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
