"""The criterion of the training step, forward + backward: the kernel path (heal_det_loss, heal_occ_loss, heal_depth_focal_loss
under autograd) against the torch compositions of heal_amd/opencood/loss/ on the same GPU (HEAL_LOSS_FUSED=0), at the workload's
head shape: N = 4 agents, two anchors, 256 x 256 (feature_stride 2), pyramid levels (1, 2, 4), and the Lift-Splat depth map
[16, 48, 48, 64] (4 agents x 4 cameras, 48 bins, 384 x 512 images at img_downsample 8).  Labels are float64, as collate_batch
and resolve_deferred_labels deliver them.

What is timed, both paths in 5 alternating rounds (medians with (min, max)):
  criterion calls   PointPillarLoss (det), PointPillarPyramidLoss 'single' without depth items (det + occ) and with them (full):
                    one forward + torch.autograd.grad with respect to every map.  The calls synchronise with the host (loss_dict), so
                    they cannot be captured: a host clock around ITERS calls that end in a device synchronise.
  depth term        FocalLoss + mean + weight against ops.depth_focal_loss_term, no host synchronisation: ops.graph_period_ms.
  kernels alone     ops.det_loss / occ_loss / depth_focal_loss with the gradients written, ops.graph_period_ms (all launches of
                    the operator, as a captured graph runs them).  Their bytes are the compulsory ones -- every map read once,
                    every gradient written once, every label read once -- and the share is of the 6.3 TB/s a streaming kernel
                    reaches on this chip.

    python scripts/loss_bench.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import configs, ops  # noqa: E402
from heal_amd.opencood.loss.point_pillar_depth_loss import FocalLoss  # noqa: E402
from heal_amd.opencood.loss.point_pillar_loss import PointPillarLoss  # noqa: E402
from heal_amd.opencood.loss.point_pillar_pyramid_loss import PointPillarPyramidLoss  # noqa: E402

STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
N, A, H, W = 4, 2, 256, 256
LEVELS = (1, 2, 4)
DEPTH = (16, 48, 48, 64)
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


def alternate(paths, timer):
    times = {k: [] for k in paths}
    for _ in range(ROUNDS):                         # alternating rounds: the paths see the same neighbours on the machine
        for k, (flag, fn) in paths.items():
            os.environ["HEAL_LOSS_FUSED"] = flag
            times[k].append(timer(fn))
    os.environ["HEAL_LOSS_FUSED"] = "1"
    return {k: med(v) for k, v in times.items()}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["stream_TBs"] = STREAM_TBS
    out["shape"] = {"N": N, "A": A, "H": H, "W": W, "levels": list(LEVELS), "depth": list(DEPTH), "labels": "float64"}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    dev = "cuda"
    leaf = lambda *shape, s=1.0: (torch.randn(shape, generator=gen) * s).to(dev).requires_grad_(True)      # noqa: E731
    cls, reg, dirp = leaf(N, A, H, W), leaf(N, 7 * A, H, W, s=0.3), leaf(N, 2 * A, H, W)
    occ = [leaf(N, 1, H // k, W // k) for k in LEVELS]
    depth_logit = leaf(*DEPTH)
    depth_idx = torch.randint(0, DEPTH[1], (DEPTH[0],) + DEPTH[2:], generator=gen).to(dev)
    pos = (torch.rand((N, H, W, A), generator=gen) > 0.995).double()
    neg = ((torch.rand((N, H, W, A), generator=gen) > 0.05).double() * (1 - pos)).to(dev)
    pos = pos.to(dev)
    tgt = {"pos_equal_one": pos, "neg_equal_one": neg, "targets": (torch.randn((N, H, W, 7 * A), generator=gen) * 0.4).double().to(dev)}
    args = configs.lidar_pyramid()["loss"]["args"]
    det_crit, pyr_crit = PointPillarLoss(args), PointPillarPyramidLoss(args)
    heads = {"cls_preds": cls, "reg_preds": reg, "dir_preds": dirp}

    def det_step():
        loss = det_crit(dict(heads), tgt)
        return loss, torch.autograd.grad(loss, [cls, reg, dirp])

    def pyr_step():
        loss = pyr_crit(dict(heads, occ_single_list=occ, pyramid="single"), tgt)
        return loss, torch.autograd.grad(loss, [cls, reg, dirp] + occ)

    def full_step():
        loss = pyr_crit(dict(heads, occ_single_list=occ, pyramid="single", depth_items_m2=(depth_logit, depth_idx)), tgt)
        return loss, torch.autograd.grad(loss, [cls, reg, dirp] + occ + [depth_logit])
    focal = FocalLoss(alpha=0.25, gamma=2.0, reduction="none")

    def depth_step():
        if ops.depth_focal_loss_supported(depth_logit, depth_idx):
            loss = ops.depth_focal_loss_term(depth_logit, depth_idx, None, alpha=0.25, weight=args["depth"]["weight"])
        else:
            loss = focal(depth_logit, depth_idx).mean() * args["depth"]["weight"]
        return loss, torch.autograd.grad(loss, [depth_logit])

    rows = {}
    for name, step in (("det", det_step), ("det_occ", pyr_step), ("full", full_step)):
        rows[name] = alternate({"fused": ("1", step), "torch": ("0", step)}, host_period_ms)
    rows["depth_term"] = alternate({"fused": ("1", depth_step), "torch": ("0", depth_step)},
                                   lambda fn: ops.graph_period_ms(fn, reps=20, iters=5))
    ok = True
    for name, step in (("det", det_step), ("det_occ", pyr_step), ("full", full_step), ("depth_term", depth_step)):
        os.environ["HEAL_LOSS_FUSED"] = "1"
        la, ga = step()
        os.environ["HEAL_LOSS_FUSED"] = "0"
        lb, gb = step()
        os.environ["HEAL_LOSS_FUSED"] = "1"
        row = rows[name]
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        row["loss_rel_diff"] = abs(float(la.detach()) - float(lb.detach())) / abs(float(lb.detach()))
        row["grad_rel_diff_max"] = max(rel(x, y) for x, y in zip(ga, gb))
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        print(name, row, flush=True)

    # the kernels alone
    det_cfg = dict(pos_cls_weight=args["pos_cls_weight"], alpha=args["cls"]["alpha"], sigma=args["reg"]["sigma"],
                   weights=(args["cls"]["weight"], args["reg"]["weight"], args["dir"]["weight"]),
                   anchor_yaw=np.deg2rad(np.array(args["dir"]["args"]["anchor_yaw"], dtype=np.float64)),
                   dir_offset=args["dir"]["args"]["dir_offset"])
    maps = [t.detach() for t in (cls, reg, dirp)]
    occ_d = [t.detach() for t in occ]
    bufs = [torch.empty_like(t) for t in maps]
    obufs = [torch.empty_like(t) for t in occ_d]
    dbuf = torch.empty_like(depth_logit)
    pix = N * H * W
    kernels = {
        "det_loss": (lambda: ops.det_loss(*maps, pos, neg, tgt["targets"], grad_out=bufs, **det_cfg),
                     pix * (10 * A * 4 * 2 + 9 * A * 8)),
        "occ_loss": (lambda: ops.occ_loss(occ_d, pos, neg, args["pyramid"]["relative_downsample"], args["pyramid"]["weight"],
                                          args["pos_cls_weight"], args["cls"]["alpha"], grad_out=obufs),
                     sum(8 * t.numel() for t in occ_d) + pix * 2 * A * 8),
        "depth_focal_loss": (lambda: ops.depth_focal_loss(depth_logit.detach(), depth_idx, None, 0.25, 1.0, grad_out=dbuf),
                             8 * depth_logit.numel() + 8 * depth_idx.numel()),
    }
    for name, (fn, nbytes) in kernels.items():
        ts = [ops.graph_period_ms(fn, reps=20, iters=5) for _ in range(ROUNDS)]
        row = med(ts)
        k_s = row["median_us"] * 1e-6
        row["MB_compulsory"] = round(nbytes / 1e6, 1)
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
