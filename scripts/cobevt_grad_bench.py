"""CoBEVT fusion under autograd at full size (lidar_cobevt.yaml: 5 agents, 128 x 128 x 256 after the shrinker; n = 5 and n = 3 real
agents): heal_agent_window_attention_backward per launch (window and grid grouping), and one training step of the fusion (forward +
backward of mean(out^2), the module in train()) with `grad_kernel` off (the library's composition) and on (ops.AgentWindowAttention),
alternated in one process: step time, peak allocated memory of the step, and the two paths' outputs and gradients against each other
(dropout off for that comparison).  FLOP rates are fractions of the fp32 MFMA peak bench.py uses.

    python scripts/cobevt_grad_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import _capi, ops, synth  # noqa: E402
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm  # noqa: E402

FP32_PEAK_TFLOPS = 157.3      # bench.py
L, H, W, C, HEADS, D = 5, 128, 128, 256, 8, 32
ARGS = {"input_dim": C, "mlp_dim": 256, "agent_size": L, "window_size": 4, "dim_head": D, "drop_out": 0.1, "depth": 3}


def frac(flops, ms):
    return round(flops / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4)


def step(model, x, rl, aff):
    model.zero_grad(set_to_none=True)
    x.grad = None
    out = model(x, rl, aff)
    out.square().mean().backward()
    return out


def timed_steps(models, x, rl, aff, reps=7, warm=2):
    """Median step time (HIP events around forward + backward) and the peak allocated bytes of one step, per path; the paths
    alternate so that a drift of the machine hits both."""
    for _ in range(warm):
        for m in models.values():
            step(m, x, rl, aff)
    torch.cuda.synchronize()
    ts, peak = {k: [] for k in models}, {}
    for _ in range(reps):
        for key, m in models.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(m, x, rl, aff)
            e1.record()
            e1.synchronize()
            ts[key].append(e0.elapsed_time(e1))
            peak[key] = max(peak.get(key, 0), torch.cuda.max_memory_allocated() - base)
            m.zero_grad(set_to_none=True)
            x.grad = None
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}, {k: (min(v), max(v)) for k, v in ts.items()}, peak


def main():
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import CoBEVT
    from tests.golden.detfill import fill_module
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    scale = D ** -0.5
    # ---- the backward kernel alone (its two launches: the groups, then the sum of the dbias partials) -------------------------------
    qkv = torch.randn((L, H, W, 3 * HEADS * D), generator=gen).cuda()
    bias = torch.randn((HEADS, 16 * L, 16 * L), generator=gen).cuda()
    gout = torch.randn((L, H, W, HEADS * D), generator=gen).cuda()
    out["parts"] = int(_capi.lib().heal_agent_window_attention_backward_parts(L, H, W, HEADS))
    with torch.no_grad():
        for n in (5, 3):
            for mode in ("window", "grid"):
                ms = ops.graph_period_ms(lambda: ops.agent_window_attention_backward(qkv, bias, gout, n, mode, HEADS, D, 4, scale))
                fl = 14.0 * L * H * W * n * 16 * HEADS * D
                out[f"kernel_{mode}_n{n}"] = {"us": round(ms * 1e3, 1), "GFLOP": round(fl / 1e9, 2), "frac_mfma": frac(fl, ms),
                                             "GB/s": round(28.0 * L * H * W * HEADS * D / (ms * 1e-3) / 1e9, 1)}
                print(f"kernel_{mode}_n{n}", out[f"kernel_{mode}_n{n}"], flush=True)
    del qkv, gout
    torch.cuda.empty_cache()
    # ---- one training step of the fusion: the library's composition against the kernel path -----------------------------------------
    models = {"torch": fill_module(CoBEVT(dict(ARGS))).cuda().train(),
              "kernel": fill_module(CoBEVT(dict(ARGS, grad_kernel=True))).cuda().train()}
    for n in (5, 3):
        x = (torch.randn((n, C, H, W), generator=gen) * 0.5).cuda().requires_grad_(True)
        pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=40.0), 5)[None]
        aff = normalize_pairwise_tfm(pw, 204.8, 204.8, 1)
        rl = torch.tensor([n])
        med, spread, peak = timed_steps(models, x, rl, aff)
        row = {}
        for key in models:
            row[f"{key}_step_ms"] = round(med[key], 2)
            row[f"{key}_step_ms_min_max"] = [round(v, 2) for v in spread[key]]
            row[f"{key}_peak_MB"] = round(peak[key] / 2 ** 20, 1)
        row["speedup"] = round(med["torch"] / med["kernel"], 3)
        # the same step without dropout: the two paths against each other
        res = {}
        for key, m in models.items():
            drops = [d for d in m.modules() if isinstance(d, torch.nn.Dropout)]
            saved = [d.p for d in drops]
            for d in drops:
                d.p = 0.0
            o = step(m, x, rl, aff)
            res[key] = [o.detach(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
            for d, p in zip(drops, saved):
                d.p = p
            m.zero_grad(set_to_none=True)
        row["kernel_vs_torch_max_rel_err"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(res["kernel"], res["torch"]))
        del res
        x.grad = None
        out[f"fusion_step_n{n}"] = row
        print(f"fusion_step_n{n}", row, flush=True)
        del x
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
