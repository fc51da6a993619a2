"""The anchor-free centre head: the kernel path (heal_center_loss under autograd, heal_center_decode_nms, heal_center_boxes) against
this repository's torch composition on the same GPU (HEAL_LOSS_FUSED=0 for the criterion, VoxelPostprocessor's tensor path for the
post-processor), at 4 samples x 128 x 128 cells (+-51.2 m, voxel 0.4, out_size_factor 2) with 40 objects per sample and
max_objs 500.

What is timed, both paths in 5 alternating rounds (medians with (min, max)):
  criterion call    CenterPointLoss: one forward + torch.autograd.grad with respect to both maps.  The call synchronises with the
                    host (loss_dict), so it cannot be captured: a host clock around ITERS calls that end in a device synchronise.
  post_process      one cav, ~300 cells above the score threshold, 3-D reg_preds: ops.center_decode_nms against
                    _post_process_multi (the tensor path the late form takes).  Both read the box count on the host.
  kernels alone     ops.center_loss with both gradients written, ops.center_boxes and ops.center_decode_nms(sync=False) under
                    ops.graph_period_ms (all launches of the operator, as a captured graph runs them).  The bytes of the two
                    streaming operators are the compulsory ones -- every map read once, every gradient / box written once --
                    and the share is of the 6.3 TB/s a streaming kernel reaches on this chip.

    python scripts/center_bench.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import configs, ops  # noqa: E402
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor  # noqa: E402
from heal_amd.opencood.loss.center_point_loss import CenterPointLoss  # noqa: E402

STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
B, H, W, OBJECTS = 4, 128, 128, 40
RANGE = [-51.2, -51.2, -3, 51.2, 51.2, 1]
ROUNDS, ITERS, WARMUP = 5, 20, 3


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def host_period_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ITERS


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["stream_TBs"] = STREAM_TBS
    out["shape"] = {"B": B, "H": H, "W": W, "objects_per_sample": OBJECTS, "max_objs": 500}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    dev = "cuda"
    rng = np.random.default_rng(0)
    hypes = configs.lidar_centerpoint("max", RANGE)
    crit = CenterPointLoss(hypes["loss"]["args"])
    cls = torch.from_numpy((rng.standard_normal((B, 1, H, W)) * 2 - 2).astype(np.float32)).to(dev).requires_grad_(True)
    bbox = torch.from_numpy((rng.standard_normal((B, 8, H, W)) * 0.5).astype(np.float32)).to(dev).requires_grad_(True)
    boxes = np.zeros((B, 100, 7), np.float32)
    boxes[:, :OBJECTS] = np.concatenate([rng.uniform(-50, 50, (B, OBJECTS, 2)), rng.uniform(-1.5, -0.5, (B, OBJECTS, 1)),
                                         rng.uniform((1.3, 1.5, 3.5), (2.0, 2.2, 5.5), (B, OBJECTS, 3)),
                                         rng.uniform(-3.1, 3.1, (B, OBJECTS, 1))], axis=2)
    mask = np.zeros((B, 100), np.float32)
    mask[:, :OBJECTS] = 1
    target = {"object_bbx_center": torch.from_numpy(boxes).to(dev), "object_bbx_mask": torch.from_numpy(mask).to(dev)}

    def crit_step():
        loss = crit({"cls_preds": cls, "bbox_preds": bbox}, target)
        return loss, torch.autograd.grad(loss, [cls, bbox])

    # post_process: one cav, ~300 candidate cells
    post = VoxelPostprocessor(hypes["postprocess"], train=False)
    logits = rng.uniform(-8.0, -4.0, (1, 1, H, W)).astype(np.float32)
    cells = rng.choice(H * W, 300, replace=False)
    logits.reshape(-1)[cells] = rng.uniform(-1.0, 3.0, 300)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    table = np.zeros((H, W, 7), np.float32)
    table[..., 0], table[..., 1], table[..., 2] = RANGE[0] + (xs + 0.5) * 0.8, RANGE[1] + (ys + 0.5) * 0.8, -1.0
    table[..., 3:6] = (1.56, 1.6, 3.9)
    table[..., 6] = rng.uniform(-3.1, 3.1, (H, W))
    heads = {"cls_preds": torch.from_numpy(logits).to(dev), "reg_preds": torch.from_numpy(table.reshape(1, H * W, 7)).to(dev)}
    data = {"ego": {"transformation_matrix": torch.eye(4), "anchor_box": None}}

    def post_kernel():
        with torch.no_grad():
            return post.post_process(data, {"ego": heads})

    def post_torch():
        with torch.no_grad():
            return post._post_process_multi(data, {"ego": heads})

    rows = {}
    times = {"fused": [], "torch": []}
    for _ in range(ROUNDS):                         # alternating rounds: the paths see the same neighbours on the machine
        for k, flag in (("fused", "1"), ("torch", "0")):
            os.environ["HEAL_LOSS_FUSED"] = flag
            times[k].append(host_period_ms(crit_step))
    os.environ["HEAL_LOSS_FUSED"] = "1"
    rows["criterion"] = {k: med(v) for k, v in times.items()}
    times = {"fused": [], "torch": []}
    for _ in range(ROUNDS):
        times["fused"].append(host_period_ms(post_kernel))
        times["torch"].append(host_period_ms(post_torch))
    rows["post_process"] = {k: med(v) for k, v in times.items()}

    la, ga = crit_step()
    os.environ["HEAL_LOSS_FUSED"] = "0"
    lb, gb = crit_step()
    os.environ["HEAL_LOSS_FUSED"] = "1"
    row = rows["criterion"]
    row["loss_rel_diff"] = abs(float(la.detach()) - float(lb.detach())) / abs(float(lb.detach()))
    row["grad_rel_diff_max"] = max(rel(x, y) for x, y in zip(ga, gb))
    (pa, sa), (pb, sb) = post_kernel(), post_torch()
    row = rows["post_process"]
    row["boxes"] = int(pa.shape[0])
    row["same_boxes"] = bool(pa.shape == pb.shape and float((pa - pb).abs().max()) <= 1e-4 and float((sa - sb).abs().max()) <= 1e-6)
    ok = True
    for name in ("criterion", "post_process"):
        row = rows[name]
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        print(name, row, flush=True)

    # the kernels alone
    cfg = crit._kernel_cfg()
    maps = (cls.detach(), bbox.detach())
    bufs = [torch.empty_like(t) for t in maps]
    post_args = (hypes["postprocess"]["target_args"]["score_threshold"], 0.7853, 2, hypes["postprocess"]["nms_thresh"],
                 np.eye(4, dtype=np.float32), hypes["postprocess"]["gt_range"])
    kernels = {
        "center_loss": (lambda: ops.center_loss(*maps, target["object_bbx_center"], target["object_bbx_mask"], grad_out=bufs, **cfg),
                        2 * 4 * (maps[0].numel() + maps[1].numel())),
        "center_boxes": (lambda: ops.center_boxes(maps[1], RANGE, [0.4, 0.4, 4], 2), 4 * (8 + 7) * B * H * W),
        "center_decode_nms": (lambda: ops.center_decode_nms(heads["cls_preds"], heads["reg_preds"], None, *post_args, sync=False),
                              None),
    }
    for name, (fn, nbytes) in kernels.items():
        row = med([ops.graph_period_ms(fn, reps=20, iters=5) for _ in range(ROUNDS)])
        if nbytes is not None:
            k_s = row["median_us"] * 1e-6
            row["MB_compulsory"] = round(nbytes / 1e6, 2)
            row["TBs"] = round(nbytes / k_s / 1e12, 3)
            row["frac_of_stream_rate"] = round(nbytes / k_s / 1e12 / STREAM_TBS, 4)
        rows["kernel_" + name] = row
        print("kernel", name, row, flush=True)
    out.update(rows)
    out["fused_faster_at_every_row"] = ok
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
