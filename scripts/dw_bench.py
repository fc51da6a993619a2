"""The streaming kernels of the camera branch one by one: every heal_depthwise_conv (the 16 MBConv stages of the two EfficientNet-b0
trunks and the 7 x 7 of the ConvNeXt aligners), every heal_se_gate with its real tile count, and heal_layernorm_nchw, at the shapes one
scene5 step calls them with.

The shapes are COLLECTED, not typed: ops.depthwise_conv / ops.se_gate / ops.layernorm_nchw are wrapped while one eager step of the
scene5 model runs, and every distinct call is kept with its count.  Each is then timed alone: `--chain` calls captured into one HIP
graph (no host launch gap; each call on its own input and output buffers, as many sets as fit `--footprint-mb` so that a large map is
not served from the 256 MiB Infinity Cache), HIP events around a replay, median of `--iters` replays divided by the chain length.
Printed with the compulsory bytes (input + output once, weights, sums) and the fraction of the achievable HBM rate (6.3 TB/s) they
amount to.  A 5 us launch cannot be above 0.1 of it: for the small maps the time is the figure, the fraction only says how far the
launch floor is from the bytes.

    python scripts/dw_bench.py [--iters 15] [--chain 20] [--out profiles/dw_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM = 6.3e12


def collect(dev):
    from bench import WORKLOADS
    from heal_amd import configs, ops
    from heal_amd.pipeline import Scene, ScenePipeline
    mods, _ = WORKLOADS["scene5"]
    pipe = ScenePipeline(configs.heal_heter(tuple(sorted(set(mods))), max_cav=5), dev, seed=0)
    scene = Scene(len(mods), seed=4, device=dev, modalities=mods)
    seen = {}
    real = {k: getattr(ops, k) for k in ("depthwise_conv", "se_gate", "layernorm_nchw")}

    def note(key):
        seen[key] = seen.get(key, 0) + 1

    def depthwise_conv(x, weight, bias, stride, pad, act="none", channel_sums=None):
        note(("depthwise", tuple(x.shape), int(weight.shape[-1]), int(stride), tuple(int(p) for p in pad), act, bool(channel_sums)))
        return real["depthwise_conv"](x, weight, bias, stride, pad, act, channel_sums)

    def se_gate(mean, w_reduce, b_reduce, w_expand, b_expand, scale=1.0, tiles=1):
        note(("se_gate", int(mean.shape[0]), int(mean.shape[1]), int(w_reduce.shape[0]), int(tiles)))
        return real["se_gate"](mean, w_reduce, b_reduce, w_expand, b_expand, scale, tiles)

    def layernorm_nchw(x, gamma, beta, eps):
        note(("layernorm", tuple(x.shape)))
        return real["layernorm_nchw"](x, gamma, beta, eps)

    ops.depthwise_conv, ops.se_gate, ops.layernorm_nchw = depthwise_conv, se_gate, layernorm_nchw
    try:
        pipe.forward(scene)
        torch.cuda.synchronize()
    finally:
        for k, f in real.items():
            setattr(ops, k, f)
    return seen


def graph_us(make_call, n_sets, chain, iters):
    """make_call(i) -> a closure running the operator on buffer set i.  Median us per call of `chain` calls replayed as one graph."""
    calls = [make_call(i) for i in range(n_sets)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for c in calls:
            c()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(chain):
                calls[i % n_sets]()
        for _ in range(3):
            g.replay()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / chain)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--footprint-mb", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dw_bench needs a GPU"
    dev = torch.device("cuda:0")
    from heal_amd import ops
    with torch.no_grad():
        seen = collect(dev)
    rows = []
    g = torch.Generator().manual_seed(0)

    def sets(nbytes):
        return int(max(1, min(a.chain, -(-a.footprint_mb * 2 ** 20 // max(nbytes, 1)))))

    for key, count in sorted(seen.items(), key=lambda kv: str(kv[0])):
        if key[0] == "depthwise":
            _, shape, k, stride, pad, act, with_sums = key
            n, C, H, W = shape
            Ho, Wo = (H + pad[2] + pad[3] - k) // stride + 1, (W + pad[0] + pad[1] - k) // stride + 1
            T = ops.depthwise_tiles(Ho, Wo)
            nbytes = 4 * (n * C * H * W + n * C * Ho * Wo + C * k * k + C + (n * C * T if with_sums else 0))
            w = (torch.randn((C, 1, k, k), generator=g) * 0.3).to(dev)
            b = torch.randn((C,), generator=g).to(dev)
            ns = sets(nbytes)
            xs = [torch.randn(shape, generator=g).to(dev) for _ in range(ns)]

            def make(i, xs=xs, w=w, b=b, stride=stride, pad=pad, act=act, with_sums=with_sums):
                return lambda: ops.depthwise_conv(xs[i], w, b, stride, pad, act, channel_sums=with_sums or None)
            name = f"depthwise k{k} s{stride} {n}x{C}x{H}x{W} -> {Ho}x{Wo} {act}{' +sums T=%d' % T if with_sums else ''}"
        elif key[0] == "se_gate":
            _, n, C, S, T = key
            nbytes = 4 * (n * C * T + 2 * S * C + S + C + n * C)
            w1 = (torch.randn((S, C, 1, 1), generator=g) / C ** 0.5).to(dev)
            b1 = torch.randn((S,), generator=g).to(dev)
            w2 = (torch.randn((C, S, 1, 1), generator=g) / S ** 0.5).to(dev)
            b2 = torch.randn((C,), generator=g).to(dev)
            ns = sets(nbytes)
            ms = [torch.randn((n, C, T), generator=g).to(dev) for _ in range(ns)]

            def make(i, ms=ms, w1=w1, b1=b1, w2=w2, b2=b2, T=T):
                return lambda: ops.se_gate(ms[i], w1, b1, w2, b2, scale=1.0 / (256 * T), tiles=T)
            name = f"se_gate n{n} C{C} S{S} tiles {T}"
        else:
            _, shape = key
            n, C, H, W = shape
            nbytes = 4 * (2 * n * C * H * W + 2 * C)
            gam, bet = torch.randn((C,), generator=g).to(dev), torch.randn((C,), generator=g).to(dev)
            ns = sets(nbytes)
            xs = [torch.randn(shape, generator=g).to(dev) for _ in range(ns)]

            def make(i, xs=xs, gam=gam, bet=bet):
                return lambda: ops.layernorm_nchw(xs[i], gam, bet, 1e-6)
            name = f"layernorm_nchw {n}x{C}x{H}x{W}"
        with torch.no_grad():
            med, best = graph_us(make, ns, a.chain, a.iters)
        row = {"op": name, "calls_per_step": count, "us": round(med, 2), "us_min": round(best, 2), "compulsory_bytes": nbytes,
               "floor_us": round(nbytes / HBM * 1e6, 2), "fraction_of_hbm": round(nbytes / HBM * 1e6 / med, 3), "buffer_sets": ns}
        rows.append(row)
        print(f"{name:<72} x{count:<2} {med:8.2f} us  {nbytes / 1e6:8.2f} MB  floor {row['floor_us']:6.2f} us  "
              f"{row['fraction_of_hbm']:.3f} of 6.3 TB/s", flush=True)
        del make
        torch.cuda.empty_cache()
    total = sum(r["us"] * r["calls_per_step"] for r in rows)
    print(f"sum over one step: {total:.1f} us in {sum(r['calls_per_step'] for r in rows)} launches")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/dw_bench.py: per-call medians inside a HIP graph, shapes collected from one scene5 step",
                       "hbm_rate": HBM, "chain": a.chain, "iters": a.iters, "rows": rows, "sum_us_per_step": round(total, 1)}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
