"""DiscoNet fusion: the fused path (heal_conv1x1 for the ego term + one heal_disco_fuse launch per scene) against the reference's
torch composition on the same GPU (HEAL_DISCO_FUSED=0: reference arithmetic, not the kernel under test), at
  5 agents, 128 x 128 x 256   configs.lidar_baseline("disconet") on the full range,
  5 agents, 256 x 256 x 256   the disco YAMLs (stride-1 shrinker),
  3 agents,  64 x  64 x 256.
Times are ops.graph_period_ms (the call captured 20 times into a graph, median replay time per call), taken in 5 alternating rounds
of both paths; medians with (min, max).  The kernel alone and heal_warp_att_fuse_levels on the same maps (two gathers and no MLP:
an upper bound on what the second gather costs) are timed the same way.  FLOPs and bytes are computed from shapes; shares are of
the fp32 MFMA peak bench.py uses and of the HBM peak.

    python scripts/disconet_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import ops, synth  # noqa: E402
from heal_amd.opencood.models.fuse_modules.fusion_in_one import DiscoFusion  # noqa: E402
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm  # noqa: E402

FP32_PEAK_TFLOPS = 157.3      # bench.py
HBM_PEAK_TBS = 8.0            # MI355X HBM3E
C = 256
SHAPES = [(5, 128, 128), (5, 256, 256), (3, 64, 64)]
ROUNDS = 5
M1, M2, M3 = ops.DISCO_WIDTHS


def kernel_flops(n, H, W):
    """heal_disco_fuse: the neighbour half of layer 1, layers 2-4 and the weighted sum."""
    return 2.0 * n * H * W * (M1 * C + M2 * M1 + M3 * M2 + M3) + 2.0 * n * C * H * W


def kernel_bytes(n, H, W):
    """Compulsory traffic: every agent's map once, the ego term, the fused map."""
    return 4.0 * H * W * (n * C + M1 + C)


def reference_bytes(n, H, W):
    """The torch composition, tensors written and read again: the warped stack (w + r twice), the concatenation (w + r), the three
    hidden maps (w + r through conv, BatchNorm and ReLU: 3 x), the weighted product (w + r), the input and the output."""
    hw = 4.0 * H * W
    return hw * (n * C + 3 * n * C + 2 * n * 2 * C + 2 * 3 * n * (M1 + M2 + M3) + 2 * n * C + C)


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def main():
    from tests.golden.disco_fill import fill_disco
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    model = fill_disco(DiscoFusion(C)).cuda().eval()
    ok = True
    for n, H, W in SHAPES:
        x = torch.randn((n, C, H, W), generator=gen).cuda()
        pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=40.0), 5)[None]
        aff = torch.as_tensor(normalize_pairwise_tfm(pw, H * 0.8, W * 0.8, 1)).cuda()     # on the device: both paths capture
        rl = torch.tensor([n])
        rows = aff[0][0, :n]
        row = {"GFLOP_kernel": round(kernel_flops(n, H, W) / 1e9, 2), "MB_compulsory": round(kernel_bytes(n, H, W) / 1e6, 1),
               "MB_torch_composition": round(reference_bytes(n, H, W) / 1e6, 1)}
        with torch.no_grad():
            assert model.fused_ok(x, [n])
            w1n, w1e, b1, w2, b2, w3, b3, w4, b4 = model._weights()
            e0 = model._ego_term(x[0], w1e, b1)
            paths = {
                "fused": ("1", lambda: model(x, rl, aff)),
                "torch": ("0", lambda: model(x, rl, aff)),
                "kernel": ("1", lambda: ops.disco_fuse(x, rows, True, e0, w1n, w2, b2, w3, b3, w4, b4)),
                "ego_term": ("1", lambda: model._ego_term(x[0], w1e, b1)),
                "warp_att_two_gathers": ("1", lambda: ops.warp_att_fuse_levels([x], rows, True, "att")),
            }
            times = {k: [] for k in paths}
            for _ in range(ROUNDS):                     # alternating rounds: both paths see the same neighbours on the machine
                for k, (env, fn) in paths.items():
                    os.environ["HEAL_DISCO_FUSED"] = env
                    times[k].append(ops.graph_period_ms(fn, reps=20, iters=5))
            os.environ["HEAL_DISCO_FUSED"] = "1"
            a = model(x, rl, aff)
            os.environ["HEAL_DISCO_FUSED"] = "0"
            b = model(x, rl, aff)
            os.environ["HEAL_DISCO_FUSED"] = "1"
        for k in paths:
            row[k] = med(times[k])
        k_s = row["kernel"]["median_us"] * 1e-6
        row["kernel_frac_mfma_peak"] = round(kernel_flops(n, H, W) / k_s / 1e12 / FP32_PEAK_TFLOPS, 4)
        row["kernel_frac_hbm_peak"] = round(kernel_bytes(n, H, W) / k_s / 1e12 / HBM_PEAK_TBS, 4)
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        row["fused_vs_torch_rel_err"] = float((a - b).abs().max() / b.abs().max())
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        out[f"n{n}_{H}x{W}x{C}"] = row
        print(f"n{n}_{H}x{W}x{C}", row, flush=True)
        del x, a, b, e0
    out["fused_faster_at_every_shape"] = ok
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
