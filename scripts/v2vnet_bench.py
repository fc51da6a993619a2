"""V2VNet fusion at full size (lidar_v2vnet.yaml: +-102.4 m, 128 x 128 x 256 after the shrinker, 2 rounds, ConvGRU; n = 5 and 3
agents): heal_v2v_message per launch (the first round's n egos and the last round's single ego, agent split A/B), the whole fusion
on the HIP path against the torch composition on the same GPU (HEAL_V2VNET_FUSED=0), and the full HeterModelBaseline step eager
and replayed from a captured graph.  FLOPs are computed from shapes; shares are of the fp32 MFMA peak bench.py uses.

    python scripts/v2vnet_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import configs, ops, synth  # noqa: E402
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm  # noqa: E402
from heal_amd.pipeline import Scene, ScenePipeline  # noqa: E402

FP32_PEAK_TFLOPS = 157.3      # bench.py
H, W, C, T = 128, 128, 256, 2


def events_ms(fn, reps=10, warm=3):
    """Median wall time of fn() on the current stream (HIP events), milliseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def conv_flops(cin, cout, n=1):
    return 2.0 * 9 * cin * cout * H * W * n


def reference_flops(n):
    """fusion_in_one.py:255-316 as written: every round, every ego i: msg_cnn (2C -> C) over n neighbours, conv_gates (3C -> 2C),
    conv_can (3C -> C); the mlp."""
    per_ego = conv_flops(2 * C, C, n) + conv_flops(3 * C, 2 * C) + conv_flops(3 * C, C)
    return T * n * per_ego + 2.0 * H * W * C * C


def hip_flops(n):
    """The device path: rounds 1 .. T-1 for every ego, the last for ego 0: the stacked x_i convolution
    (C -> 3C), the neighbour convolutions (C -> C per agent), the agg convolution (C -> 2C); the mlp."""
    egos = (T - 1) * n + 1
    return egos * (conv_flops(C, 3 * C) + conv_flops(C, C, n) + conv_flops(C, 2 * C)) + 2.0 * H * W * C * C


def frac(flops, ms):
    return round(flops / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4)


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    from tests.golden.detfill import fill_module
    from heal_amd.opencood.tools.train_utils import create_model
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    # ---- the kernel alone: executed FLOPs = direct-equivalent FLOPs (an implicit GEMM computes the direct sum) ----------------
    w = (torch.randn((C, C, 3, 3), generator=gen) * 0.02).cuda()
    for n in (5, 3):
        for n_ego in (n, 1):
            xs = torch.randn((n_ego, n, C, H, W), generator=gen).cuda()
            mask = torch.rand((n_ego, n, H, W), generator=gen).cuda()
            e = torch.randn((n_ego, 3 * C, H, W), generator=gen).cuda()
            fl = conv_flops(C, C, n * n_ego)
            for split in sorted({1, ops.v2v_message_nsplit(n_ego, n, C, H, W, ops.v2v_message_tile_h(n_ego, C, H, W, 0))}):
                ms = ops.graph_period_ms(lambda: ops.v2v_message(xs, mask, e, w, None, "mean", nsplit=split))
                key = f"kernel_mean_n{n}_egos{n_ego}_split{split}"
                out[key] = {"us": round(ms * 1e3, 1), "GFLOP_executed": round(fl / 1e9, 1),
                            "GFLOP_direct_equivalent": round(fl / 1e9, 1), "frac_mfma": frac(fl, ms)}
                print(key, out[key], flush=True)
            ms = ops.graph_period_ms(lambda: ops.v2v_message(xs, mask, e, w, None, "max"))
            out[f"kernel_max_n{n}_egos{n_ego}"] = {"us": round(ms * 1e3, 1), "frac_mfma": frac(fl, ms)}
            print(f"kernel_max_n{n}_egos{n_ego}", out[f"kernel_max_n{n}_egos{n_ego}"], flush=True)
            del xs, mask, e
    # ---- the fusion: HIP path vs torch composition ------------------------------------------------------------------------------
    hypes = configs.lidar_baseline("v2vnet")
    model = fill_module(create_model(hypes)).cuda().eval()
    for n in (5, 3):
        x = (torch.randn((n, C, H, W), generator=gen) * 0.5).cuda()
        pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=40.0), 5)[None]
        aff = normalize_pairwise_tfm(pw, 204.8, 204.8, 1)
        rl = torch.tensor([n])
        row = {"GFLOP_reference": round(reference_flops(n) / 1e9, 1), "GFLOP_hip": round(hip_flops(n) / 1e9, 1)}
        with torch.no_grad():
            for path in ("1", "0"):
                os.environ["HEAL_V2VNET_FUSED"] = path
                ms = events_ms(lambda: model.fusion_net(x, rl, aff), reps=5, warm=2)
                key = "hip" if path == "1" else "torch"
                row[f"{key}_ms"] = round(ms, 3)
                row[f"{key}_frac_mfma"] = frac(hip_flops(n) if path == "1" else reference_flops(n), ms)
            os.environ["HEAL_V2VNET_FUSED"] = "1"
            a = model.fusion_net(x, rl, aff)
            os.environ["HEAL_V2VNET_FUSED"] = "0"
            b = model.fusion_net(x, rl, aff)
            os.environ["HEAL_V2VNET_FUSED"] = "1"
            row["hip_vs_torch_rel_err"] = float((a - b).abs().max() / b.abs().max())
        row["speedup"] = round(row["torch_ms"] / row["hip_ms"], 2)
        out[f"fusion_n{n}"] = row
        print(f"fusion_n{n}", row, flush=True)
        del x
    del model
    torch.cuda.empty_cache()
    # ---- the whole model step: eager and graph-replayed ---------------------------------------------------------------------------
    pipe = ScenePipeline(hypes, "cuda:0", seed=0)
    for n in (5, 3):
        scene = Scene(n, seed=40 + n, device="cuda:0")
        with torch.no_grad():
            eager = events_ms(lambda: pipe.step(scene), reps=10)
            pipe.capture(scene, warmup=2)
            graph = events_ms(lambda: pipe.replay(scene), reps=10)
        out[f"model_step_n{n}"] = {"eager_ms": round(eager, 3), "graph_ms": round(graph, 3)}
        print(f"model_step_n{n}", out[f"model_step_n{n}"], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
