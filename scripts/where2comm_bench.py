"""Where2comm and Who2com fusion: the fused paths against the reference's torch composition on the same GPU (`fused = False` on the
instance: reference arithmetic, not the kernels under test), at
  5 agents, 128 x 128 x 256   configs.lidar_baseline("where2comm" | "who2com") on the full range,
  3 agents,  64 x  64 x 256.
Where2commFusion: (a) `fused = False`, (b) the fused path (two heal_conv1x1 projections, heal_warp_mha_fuse, the NCHW tail), (c)
heal_warp_mha_fuse alone with its share of the 6.3 TB/s streaming rate over its algorithmic bytes ((2 n + 2) C H W 4 read,
2 C H W 4 written).  Who2comFusion: (a) and (b).
Times are ops.graph_period_ms (the call captured 20 times into a graph, median replay time per call), taken in 5 alternating rounds
of the paths; medians with (min, max).

    python scripts/where2comm_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import ops, synth  # noqa: E402
from heal_amd.opencood.models.fuse_modules.fusion_in_one import Where2commFusion, Who2comFusion  # noqa: E402
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm  # noqa: E402

STREAM_TBS = 6.3              # the streaming rate the project's memory-bound kernels are held against
C = 256
SHAPES = [(5, 128, 128), (3, 64, 64)]
ROUNDS = 5


def kernel_bytes(n, H, W):
    """heal_warp_mha_fuse: Q, the ego map and every agent's K and V read once; the context and the warped ego written."""
    return 4.0 * C * H * W * ((2 * n + 2) + 2)


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def main():
    from tests.golden.w2c_fill import fill_w2c
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    w2c = fill_w2c(Where2commFusion(C)).cuda().eval()
    who = fill_w2c(Who2comFusion(C)).cuda().eval()
    ok = True
    for n, H, W in SHAPES:
        x = (torch.randn((n, C, H, W), generator=gen) * 1.5).cuda()
        pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=40.0), 5)[None]
        aff = torch.as_tensor(normalize_pairwise_tfm(pw, H * 0.8, W * 0.8, 1)).cuda()     # on the device: every path captures
        rl = torch.tensor([n])
        rows = aff[0][0, :n]
        row = {"MB_kernel_algorithmic": round(kernel_bytes(n, H, W) / 1e6, 1)}

        def run(model, fused):
            model.fused = fused
            return model(x, rl, aff)

        with torch.no_grad():
            w2c.fused = who.fused = True
            assert w2c.fused_ok(x, [n]) and who.fused_ok(x, [n])
            wq, wkv, bq, bk, bv = w2c._weights()[:5]
            kv, q = ops.conv1x1(x, wkv), ops.conv1x1(x[:1], wq)
            heads = w2c.mha_fusion.attn.num_heads
            paths = {
                "where2comm_torch": lambda: run(w2c, False),
                "where2comm_fused": lambda: run(w2c, True),
                "warp_mha_fuse": lambda: ops.warp_mha_fuse(q[0], kv, x[0], bq, bk, bv, heads, rows, True),
                "who2com_torch": lambda: run(who, False),
                "who2com_fused": lambda: run(who, True),
            }
            times = {k: [] for k in paths}
            for _ in range(ROUNDS):                     # alternating rounds: the paths see the same neighbours on the machine
                for k, fn in paths.items():
                    times[k].append(ops.graph_period_ms(fn, reps=20, iters=5))
            errs = {}
            for name, model in (("where2comm", w2c), ("who2com", who)):
                a, b = run(model, True), run(model, False)
                errs[name] = float((a - b).abs().max() / b.abs().max())
            w2c.fused = who.fused = True
        for k in paths:
            row[k] = med(times[k])
        k_s = row["warp_mha_fuse"]["median_us"] * 1e-6
        row["warp_mha_fuse_frac_of_streaming_rate"] = round(kernel_bytes(n, H, W) / k_s / 1e12 / STREAM_TBS, 4)
        for name in ("where2comm", "who2com"):
            row[f"{name}_speedup_fused_over_torch"] = round(row[f"{name}_torch"]["median_us"] / row[f"{name}_fused"]["median_us"], 2)
            row[f"{name}_fused_vs_torch_rel_err"] = errs[name]
            ok = ok and row[f"{name}_fused"]["median_us"] < row[f"{name}_torch"]["median_us"]
        out[f"n{n}_{H}x{W}x{C}"] = row
        print(f"n{n}_{H}x{W}x{C}", row, flush=True)
        del x, kv, q
    out["fused_faster_at_every_shape"] = ok
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
