"""CoBEVT fusion at full size (lidar_cobevt.yaml: 5 agents, +-102.4 m, 128 x 128 x 256 after the shrinker; n = 5 and n = 3 real
agents): heal_agent_window_attention per launch (window and grid grouping), the whole fusion on the HIP path against the torch
composition on the same GPU (HEAL_COBEVT_FUSED=0), and the full HeterModelBaseline step eager and replayed from a captured graph.
FLOP rates are fractions of the fp32 MFMA peak bench.py uses.

    python scripts/cobevt_bench.py [out.json]
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
L, H, W, C, HEADS, D = 5, 128, 128, 256, 8, 32


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


def fusion_flops(n):
    """Per block, two attention half-blocks (to_qkv 768 + to_out 256 outputs) and two feed-forwards (256 + 256) over the L H W tokens;
    attention over the n valid agents' keys (6 half-blocks); the mlp_head linear."""
    tokens = L * H * W
    lin = 3 * 2.0 * tokens * C * (2 * (3 * C + C) + 2 * (C + C))
    att = 6 * 4.0 * tokens * n * 16 * C
    return lin + att + 2.0 * H * W * C * C


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
    # ---- the kernel alone ------------------------------------------------------------------------------------------------------
    qkv = torch.randn((L, H, W, 3 * HEADS * D), generator=gen).cuda()
    bias = torch.randn((HEADS, 16 * L, 16 * L), generator=gen).cuda()
    res = torch.empty((L, H, W, HEADS * D), device="cuda")
    for n in (5, 3):
        for mode in ("window", "grid"):
            ms = ops.graph_period_ms(lambda: ops.agent_window_attention(qkv, bias, n, mode, HEADS, D, 4, D ** -0.5, out=res))
            fl = 4.0 * L * H * W * n * 16 * HEADS * D
            out[f"kernel_{mode}_n{n}"] = {"us": round(ms * 1e3, 1), "GFLOP": round(fl / 1e9, 2), "frac_mfma": frac(fl, ms),
                                         "GB/s": round(16.0 * L * H * W * HEADS * D / (ms * 1e-3) / 1e9, 1)}
            print(f"kernel_{mode}_n{n}", out[f"kernel_{mode}_n{n}"], flush=True)
    del qkv, res
    # ---- the fusion: HIP path vs torch composition ------------------------------------------------------------------------------
    hypes = configs.lidar_baseline("cobevt")
    model = fill_module(create_model(hypes)).cuda().eval()
    for n in (5, 3):
        x = (torch.randn((n, C, H, W), generator=gen) * 0.5).cuda()
        pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=40.0), 5)[None]
        aff = normalize_pairwise_tfm(pw, 204.8, 204.8, 1)
        rl = torch.tensor([n])
        row = {"GFLOP": round(fusion_flops(n) / 1e9, 1)}
        with torch.no_grad():
            for path in ("1", "0"):
                os.environ["HEAL_COBEVT_FUSED"] = path
                ms = events_ms(lambda: model.fusion_net(x, rl, aff))
                key = "hip" if path == "1" else "torch"
                row[f"{key}_ms"] = round(ms, 3)
                row[f"{key}_frac_mfma"] = frac(fusion_flops(n), ms)
            os.environ["HEAL_COBEVT_FUSED"] = "1"
            a = model.fusion_net(x, rl, aff)
            os.environ["HEAL_COBEVT_FUSED"] = "0"
            b = model.fusion_net(x, rl, aff)
            os.environ["HEAL_COBEVT_FUSED"] = "1"
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
