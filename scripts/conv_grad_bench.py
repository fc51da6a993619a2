"""Dense convolutions of one training step, forward + backward per shape: this library's kernels (ops.ConvGrad: heal_conv3x3 /
heal_conv1x1 forward and data gradient, heal_conv_wgrad; HEAL_CONV_GRAD=kernel) against the library composition autograd runs by
default (MIOpen forward, data gradient and weight gradient).

The shapes are COLLECTED, not typed: a forward hook on every nn.Conv2d records what one training step of the pyramid LiDAR model
(configs.lidar_pyramid, two agents) calls as a module, once without and once with the switch: the difference is what
bev_blocks.grad_conv routes to ops.ConvGrad, the second count what stays on the library under the switch.
Per shape: warm-up, then HIP events around each of `--iters` forward + backward calls, median.  heal_conv_wgrad is also timed alone and
reported as a fraction of the fp32 MFMA peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz).  The whole step is timed
both ways as well.  Decides whether HEAL_CONV_GRAD=kernel becomes the default.

    python scripts/conv_grad_bench.py [--iters 15] [--out profiles/conv_grad_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn as nn

from heal_amd import configs, ops
from heal_amd.opencood.tools.train_utils import create_model
from heal_amd.pipeline import Scene, fill_deterministic

PEAK_F32_MFMA = 157.3e12


def median_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def set_mode(kernel):
    if kernel:
        os.environ["HEAL_CONV_GRAD"] = "kernel"
    else:
        os.environ.pop("HEAL_CONV_GRAD", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "conv_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "conv_grad_bench needs a GPU"
    dev = torch.device("cuda:0")
    hypes = configs.lidar_pyramid()
    model = fill_deterministic(create_model(hypes), 0).to(dev).train()
    data = Scene(2, seed=9, device=dev).model_input()

    def step():
        model.zero_grad(set_to_none=True)
        out = model(data)
        loss = sum(out[k].square().mean() for k in ("cls_preds", "reg_preds", "dir_preds"))
        loss.backward()

    # ---- the shapes of one step: a forward hook on every nn.Conv2d sees the convolutions that are CALLED AS MODULES.  Without the
    # switch that is all of them; under the switch the ones bev_blocks.grad_conv hands to ops.ConvGrad no longer are, so the
    # difference of the two counts is exactly what the switch routes, and the second count what stays on the library.
    def collect(kernel):
        set_mode(kernel)
        seen, hooks = {}, []

        def hook(conv, inputs, _out):
            x = inputs[0]
            key = (int(x.shape[0]), conv.in_channels, conv.out_channels, int(x.shape[2]), int(x.shape[3]), conv.kernel_size[0],
                   conv.stride[0], conv.padding[0], conv.groups, conv.bias is not None)
            seen[key] = seen.get(key, 0) + 1

        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                hooks.append(m.register_forward_hook(hook))
        before = ops.CONV_GRAD_CALLS["forward"]
        step()
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        return seen, ops.CONV_GRAD_CALLS["forward"] - before

    everything, none_routed = collect(False)
    left, n_routed = collect(True)
    assert none_routed == 0
    seen = {}
    for key, calls in everything.items():
        if calls > left.get(key, 0):
            n, cin, cout, H, W, k, s, pad, _groups, has_bias = key
            if pad == 0 and k == 3:          # a ZeroPad2d(1) in front, folded into the kernel's own padding
                H, W = H - 2, W - 2
            seen[(n, cin, cout, H, W, k, s, has_bias)] = calls - left.get(key, 0)
    assert sum(seen.values()) == n_routed, (sum(seen.values()), n_routed)
    transposed = {}
    for m in model.modules():
        if isinstance(m, nn.ConvTranspose2d):
            tk = (m.in_channels, m.out_channels, m.kernel_size, m.stride)
            transposed[tk] = transposed.get(tk, 0) + 1

    # ---- the whole step, both ways
    step_ms = {}
    for name, kernel in (("library", False), ("kernel", True)):
        set_mode(kernel)
        step_ms[name] = median_ms(step, max(5, a.iters // 3), warm=2)
    model.zero_grad(set_to_none=True)

    # ---- per shape
    rows = []
    for (n, cin, cout, H, W, k, s, has_bias), calls in sorted(seen.items()):
        torch.manual_seed(cin * 7 + cout)
        conv = nn.Conv2d(cin, cout, k, s, k // 2, bias=has_bias).to(dev)
        x = torch.randn(n, cin, H, W, device=dev, requires_grad=True)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        ct = torch.randn(n, cout, Ho, Wo, device=dev)

        def lib():
            x.grad = None
            conv.zero_grad(set_to_none=True)
            conv(x).backward(ct)

        def mine():
            x.grad = None
            conv.zero_grad(set_to_none=True)
            ops.ConvGrad.apply(x, conv.weight, conv.bias, s).backward(ct)

        lib()
        ref = (x.grad.clone(), conv.weight.grad.clone())
        before = dict(ops.CONV_GRAD_CALLS)
        mine()
        dx_route = "kernel" if ops.CONV_GRAD_CALLS["dx_kernel"] > before["dx_kernel"] else "library"
        diff = [float((g - r).abs().max() / r.abs().max().clamp_min(1e-30)) for g, r in zip((x.grad, conv.weight.grad), ref)]
        t_lib, t_mine = median_ms(lib, a.iters), median_ms(mine, a.iters)
        with torch.no_grad():
            xd = x.detach()
            t_w = median_ms(lambda: ops.conv_wgrad(xd, ct, k, s), a.iters)
        flops = 2.0 * n * Ho * Wo * cin * cout * k * k
        rows.append({"n": n, "cin": cin, "cout": cout, "H": H, "W": W, "k": k, "stride": s, "bias": has_bias, "calls_per_step": calls,
                     "library_fwd_bwd_ms": round(t_lib, 4), "kernel_fwd_bwd_ms": round(t_mine, 4), "dx_route": dx_route,
                     "conv_wgrad_ms": round(t_w, 4), "conv_wgrad_splits": int(ops._capi.lib().heal_conv_wgrad_splits(n, cin, cout, H, W, k, s)),
                     "conv_wgrad_tflops": round(flops / (t_w * 1e-3) / 1e12, 2),
                     "conv_wgrad_fraction_of_fp32_mfma_peak": round(flops / (t_w * 1e-3) / PEAK_F32_MFMA, 4),
                     "dx_rel_diff_vs_library": diff[0], "dw_rel_diff_vs_library": diff[1]})
        print(f"n{n} {cin:4d}->{cout:4d} {H:3d}x{W:3d} k{k} s{s} x{calls:2d}: library {t_lib:7.3f} ms | kernels {t_mine:7.3f} ms (dx {dx_route}) | "
              f"wgrad alone {t_w:7.3f} ms = {rows[-1]['conv_wgrad_tflops']:6.2f} TFLOP/s ({100 * rows[-1]['conv_wgrad_fraction_of_fp32_mfma_peak']:.1f}% of peak) "
              f"| dx / dW rel diff {diff[0]:.1e} / {diff[1]:.1e}", flush=True)
    tot_lib = sum(r["library_fwd_bwd_ms"] * r["calls_per_step"] for r in rows)
    tot_mine = sum(r["kernel_fwd_bwd_ms"] * r["calls_per_step"] for r in rows)
    result = {
        "what": "dense convolutions of one training step of configs.lidar_pyramid() (2 agents, full range), forward + backward per shape; "
                "median of HIP-event timings; library = autograd on MIOpen, kernel = ops.ConvGrad (HEAL_CONV_GRAD=kernel)",
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "fp32_mfma_peak_tflops": PEAK_F32_MFMA / 1e12,
        "step_ms": {k: round(v, 3) for k, v in step_ms.items()},
        "routed_convs_sum_ms": {"library": round(tot_lib, 3), "kernel": round(tot_mine, 3)},
        "routed_convs_fraction_of_library_step": round(tot_lib / step_ms["library"], 4),
        "shapes": rows,
        "left_to_the_library_under_the_switch": {
            "conv2d (n, cin, cout, H, W, kernel, stride, padding, groups, bias) -> calls": {str(k): v for k, v in sorted(left.items())},
            "conv_transpose2d (cin, cout, kernel, stride) -> modules": {str(k): v for k, v in sorted(transposed.items())},
            "data gradient of the stride-2 convolutions": [f"{r['cin']}->{r['cout']} k{r['k']} {r['H']}x{r['W']}" for r in rows
                                                           if r["dx_route"] == "library"]},
    }
    print(f"step: library {step_ms['library']:.2f} ms, kernel {step_ms['kernel']:.2f} ms; routed convolutions fwd+bwd summed: "
          f"library {tot_lib:.2f} ms, kernel {tot_mine:.2f} ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
