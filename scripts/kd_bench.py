"""DiscoNet's distillation term, forward + backward: the fused path (ops.KdKlLoss: heal_kd_kl_loss writes the loss and the
student's gradient in one pass, backward scales the gradient by the incoming one) against the reference's torch composition on
the same GPU (HEAL_KD_FUSED=0: permuted copies, log_softmax, softmax, kl_div, mean and their autograd backward), at
  (2, 256, 256, 256)   LiDAROnly/lidar_disco.yaml's own size (batch 2, full range),
  (1, 256, 256, 256), (2, 256, 128, 128), (2, 64, 256, 256).
Both paths go through PointPillarDiscoNetLoss.kd_term and the YAML's weight (10000 x loss), and torch.autograd.grad with respect
to the student.  Times are ops.graph_period_ms (the call captured 20 times into a graph, median replay time per call), taken in 5
alternating rounds of the paths; medians with (min, max).  The kernel alone (both launches of heal_kd_kl_loss, gradient written)
is timed the same way; its bytes are the compulsory ones -- each operand read once, the gradient written once -- and its share is
of the 6.3 TB/s a streaming kernel reaches on this chip.

    python scripts/kd_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import ops  # noqa: E402
from heal_amd.opencood.loss.point_pillar_disconet_loss import PointPillarDiscoNetLoss  # noqa: E402

STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
KD_WEIGHT = 10000.0           # lidar_disco.yaml loss.args.kd.weight
SHAPES = [(2, 256, 256, 256), (1, 256, 256, 256), (2, 256, 128, 128), (2, 64, 256, 256)]
ROUNDS = 5


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["stream_TBs"] = STREAM_TBS
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    ok = True
    for shape in SHAPES:
        student = (torch.randn(shape, generator=gen) * 1.5).cuda().requires_grad_(True)
        teacher = (torch.randn(shape, generator=gen) * 1.5).cuda()
        grad_buf = torch.empty_like(teacher)
        nbytes = 4.0 * student.numel()

        def step():
            loss = PointPillarDiscoNetLoss.kd_term(student, teacher) * KD_WEIGHT
            return loss, torch.autograd.grad(loss, student)[0]
        paths = {"fused": ("1", step), "torch": ("0", step),
                 "kernel": ("1", lambda: ops.kd_kl_loss(student, teacher, grad_out=grad_buf))}
        times = {k: [] for k in paths}
        for _ in range(ROUNDS):                     # alternating rounds: the paths see the same neighbours on the machine
            for k, (env, fn) in paths.items():
                os.environ["HEAL_KD_FUSED"] = env
                times[k].append(ops.graph_period_ms(fn, reps=20, iters=5))
        os.environ["HEAL_KD_FUSED"] = "1"
        la, ga = step()
        os.environ["HEAL_KD_FUSED"] = "0"
        lb, gb = step()
        os.environ["HEAL_KD_FUSED"] = "1"
        torch.cuda.synchronize()
        row = {k: med(times[k]) for k in paths}
        k_s = row["kernel"]["median_us"] * 1e-6
        row["MB_per_tensor"] = round(nbytes / 1e6, 1)
        row["MB_compulsory"] = round(3 * nbytes / 1e6, 1)
        row["kernel_TBs"] = round(3 * nbytes / k_s / 1e12, 3)
        row["kernel_frac_of_stream_rate"] = round(3 * nbytes / k_s / 1e12 / STREAM_TBS, 4)
        # the fused step also scales the saved gradient by the incoming one: one more read and write of the map
        row["fused_TBs_incl_scaling_pass"] = round(5 * nbytes / (row["fused"]["median_us"] * 1e-6) / 1e12, 3)
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        row["loss_rel_diff"] = abs(float(la.detach()) - float(lb.detach())) / abs(float(lb.detach()))
        row["grad_rel_diff"] = float((ga - gb).abs().max() / gb.abs().max())
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        name = "x".join(str(v) for v in shape)
        out[name] = row
        print(name, row, flush=True)
        del student, teacher, grad_buf, ga, gb
        torch.cuda.empty_cache()
    out["fused_faster_at_every_shape"] = ok
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
