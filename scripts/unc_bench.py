"""CoAlign's uncertainty detector: the kernel path (heal_unc_loss under autograd, heal_decode_nms_agents_unc) against this
repository's torch composition on the same GPU (HEAL_LOSS_FUSED=0 for the criterion, the post-processor's tensor path), at the
full-range head-map size of configs.lidar_uncertainty(): 4 samples x 256 x 256 cells x 2 anchors, dim 3, l2 + von Mises under
limit_period, float64 labels (what the datasets deliver), 0.5 % positive anchors.

What is timed, both paths in 5 alternating rounds (medians with (min, max)):
  criterion call    PointPillarUncertaintyLoss: one forward + torch.autograd.grad with respect to the four head maps.  The call
                    synchronises with the host (loss_dict), so it cannot be captured: a host clock around ITERS calls that end
                    in a device synchronise.
  post_process      return_uncertainty=True, one cav with ~600 anchors above the score threshold: ops.decode_nms_agents_unc
                    against _post_process_unc_tensors.  Both read the box count on the host.
  kernel alone      ops.unc_loss with the four gradients written, under ops.graph_period_ms (all three launches, as a captured
                    graph runs them).  The bytes are the compulsory ones -- every map and label read once, every gradient written
                    once -- and the share is of the 6.3 TB/s a streaming kernel reaches on this chip.

    python scripts/unc_bench.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import configs, ops, synth  # noqa: E402
from heal_amd.opencood.data_utils.post_processor.uncertainty_voxel_postprocessor import UncertaintyVoxelPostprocessor  # noqa: E402
from heal_amd.opencood.loss.point_pillar_uncertainty_loss import PointPillarUncertaintyLoss  # noqa: E402

STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
N, A, H, W, DIM = 4, 2, 256, 256, 3
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
    out["shape"] = {"N": N, "A": A, "H": H, "W": W, "dim": DIM, "labels": "float64"}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hypes = configs.lidar_uncertainty()
    crit = PointPillarUncertaintyLoss(hypes["loss"]["args"])
    maps = {"cls_preds": torch.randn((N, A, H, W), generator=g), "reg_preds": torch.randn((N, 7 * A, H, W), generator=g) * 0.3,
            "unc_preds": (torch.rand((N, DIM * A, H, W), generator=g) * 2 - 1) * 4.0,
            "dir_preds": torch.randn((N, 2 * A, H, W), generator=g)}
    maps = {k: v.to(dev).requires_grad_(True) for k, v in maps.items()}
    pos = (torch.rand((N, H, W, A), generator=g) > 0.995).double()
    neg = (torch.rand((N, H, W, A), generator=g) > 0.2).double() * (1 - pos)
    target = {"pos_equal_one": pos.to(dev), "neg_equal_one": neg.to(dev),
              "targets": (torch.randn((N, H, W, 7 * A), generator=g) * 0.4).double().to(dev)}

    def crit_step():
        loss = crit(dict(maps), target)
        return loss, torch.autograd.grad(loss, list(maps.values()))

    # post_process: one cav, ~600 candidate anchors in 3 x 3 clusters (both anchors), its own pose
    post = UncertaintyVoxelPostprocessor(hypes["postprocess"], train=False)
    rng = np.random.default_rng(0)
    cav = synth.make_cav(rng, post.generate_anchor_box(), synth.x_to_world([1.0, -0.5, 0.05, 0.0, 10.0, 0.0]), 43)
    synth.deal_ladder(rng, [cav])
    heads = {"cls_preds": torch.from_numpy(cav["cls"]).to(dev), "reg_preds": torch.from_numpy(cav["reg"]).to(dev),
             "dir_preds": torch.from_numpy(cav["dir"]).to(dev),
             "unc_preds": ((torch.rand((1, DIM * A, H, W), generator=g) * 2 - 1) * 4.0).to(dev)}
    data = {"ego": {"transformation_matrix": torch.from_numpy(cav["tfm"]),
                    "anchor_box": torch.from_numpy(cav["anchors"]).to(dev)}}

    def post_kernel():
        with torch.no_grad():
            return post.post_process(data, {"ego": heads}, return_uncertainty=True)

    def post_torch():
        with torch.no_grad():
            return post._post_process_unc_tensors([data["ego"]], [heads])

    assert post._unc_fused_ok([heads])
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

    calls = {}
    ops.TIMING = calls
    la, ga = crit_step()
    ops.TIMING = None
    assert any(c.startswith("unc_loss") for c in calls), calls
    os.environ["HEAL_LOSS_FUSED"] = "0"
    lb, gb = crit_step()
    os.environ["HEAL_LOSS_FUSED"] = "1"
    row = rows["criterion"]
    row["positives"] = int(pos.sum())
    row["loss_rel_diff"] = abs(float(la.detach()) - float(lb.detach())) / abs(float(lb.detach()))
    row["grad_rel_diff_max"] = max(rel(x, y) for x, y in zip(ga, gb))
    (pa, sa, ua), (pb, sb, ub) = post_kernel(), post_torch()
    row = rows["post_process"]
    row["boxes"] = int(pa.shape[0])
    row["same_boxes"] = bool(pa.shape == pb.shape and float((pa - pb).abs().max()) <= 1e-3 and float((sa - sb).abs().max()) <= 1e-6
                             and torch.equal(ua, ub))
    ok = True
    for name in ("criterion", "post_process"):
        row = rows[name]
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        print(name, row, flush=True)

    # the kernel alone
    cfg = dict(pos_cls_weight=crit.pos_cls_weight, alpha=crit.cls["alpha"], sigma=crit.reg["sigma"],
               weights=(crit.cls["weight"], crit.reg["weight"], crit.uncertainty["weight"], crit.dir["weight"]), dim=DIM,
               xy_loss_type="l2", angle_loss_type="von-mise", angle_weight=0.5, lambda_V=0.001, s0=1.0, limit_period=True,
               anchor_yaw=np.deg2rad(np.array(crit.dir["args"]["anchor_yaw"], dtype=np.float64)),
               dir_offset=crit.dir["args"]["dir_offset"])
    plain = [m.detach() for m in maps.values()]
    bufs = [torch.empty_like(t) for t in plain]
    labels = (target["pos_equal_one"], target["neg_equal_one"], target["targets"])
    nbytes = 2 * 4 * sum(m.numel() for m in plain) + 8 * sum(t.numel() for t in labels)
    row = med([ops.graph_period_ms(lambda: ops.unc_loss(*plain, *labels, grad_out=bufs, **cfg), reps=20, iters=5)
               for _ in range(ROUNDS)])
    k_s = row["median_us"] * 1e-6
    row["MB_compulsory"] = round(nbytes / 1e6, 2)
    row["TBs"] = round(nbytes / k_s / 1e12, 3)
    row["frac_of_stream_rate"] = round(nbytes / k_s / 1e12 / STREAM_TBS, 4)
    rows["kernel_unc_loss"] = row
    print("kernel unc_loss", row, flush=True)
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
