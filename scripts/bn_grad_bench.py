"""BatchNorm2d (+ residual) (+ ReLU) sites of one training step, forward + backward per shape: this library's kernels
(ops.BatchNormAct: heal_bn_stats, heal_bn_act_forward, heal_bn_act_backward; ops.bn_grad("kernel")) against the library composition
autograd runs by default (batch_norm, add, relu: three operators, three autograd nodes).

The shapes are COLLECTED, not typed: bev_blocks.grad_bn_act is wrapped for one training step of the pyramid LiDAR model
(configs.lidar_pyramid, two agents) and records every site with its ReLU / residual form; a forward hook on every nn.BatchNorm2d
counts the calls that do not come through it.  Per shape: 3 warm-ups, then HIP events around each of `--iters` forward + backward
calls, the two paths ALTERNATING, median.  Each kernel is also timed alone and reported with the bytes it has to move and its share
of the 6.3 TB/s streaming rate.  The whole step (forward, loss, backward) is timed in both modes in the same run, alternating, median
of 5.  Decides whether ops.bn_grad("kernel") becomes the default.

    python scripts/bn_grad_bench.py [--iters 15] [--out profiles/bn_grad_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from heal_amd import configs, ops
from heal_amd.opencood.models.sub_modules import base_bev_backbone, bev_blocks
from heal_amd.opencood.tools.train_utils import create_model
from heal_amd.pipeline import Scene, fill_deterministic

STREAM_BYTES_PER_S = 6.3e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating_medians(fns, iters, warm=3):
    """Median milliseconds of each callable: `warm` calls of each, then `iters` rounds in which they take turns."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bn_grad_bench needs a GPU"
    dev = torch.device("cuda:0")
    model = fill_deterministic(create_model(configs.lidar_pyramid()), 0).to(dev).train()
    data = Scene(2, seed=9, device=dev).model_input()

    def step():
        model.zero_grad(set_to_none=True)
        out = model(data)
        loss = sum(out[k].square().mean() for k in ("cls_preds", "reg_preds", "dir_preds"))
        loss.backward()

    # ---- the sites of one step
    seen, outside, hooks = {}, {}, []
    real = bev_blocks.grad_bn_act
    inside = [0]

    def recording(bn, x, relu, residual=None):
        key = (int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(x.shape[3]), bool(relu), residual is not None, bool(bn.training))
        seen[key] = seen.get(key, 0) + 1
        inside[0] += 1
        try:
            return real(bn, x, relu, residual)
        finally:
            inside[0] -= 1

    def hook(bn, inputs, _out):
        if not inside[0]:
            key = tuple(int(v) for v in inputs[0].shape)
            outside[key] = outside.get(key, 0) + 1

    bev_blocks.grad_bn_act = base_bev_backbone.grad_bn_act = recording
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            hooks.append(m.register_forward_hook(hook))
    try:
        step()
        torch.cuda.synchronize()
    finally:
        bev_blocks.grad_bn_act = base_bev_backbone.grad_bn_act = real
        for h in hooks:
            h.remove()

    # ---- the whole step, both modes in the same run, taking turns
    def step_in(mode):
        def run():
            with ops.bn_grad(mode):
                step()
        return run
    before = dict(ops.BN_GRAD_CALLS)
    step_ms = dict(zip(("torch", "kernel"), alternating_medians([step_in("torch"), step_in("kernel")], 5, warm=2)))
    routed = {k: ops.BN_GRAD_CALLS[k] - before[k] for k in before}
    model.zero_grad(set_to_none=True)

    # ---- per shape
    rows = []
    for (n, C, H, W, relu, has_res, training), calls in sorted(seen.items()):
        torch.manual_seed(C + H)
        bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(dev).train(training)
        x = torch.randn(n, C, H, W, device=dev, requires_grad=True)
        r = torch.randn(n, C, H, W, device=dev, requires_grad=True) if has_res else None
        ct = torch.randn(n, C, H, W, device=dev)

        def clear():
            x.grad = None
            bn.zero_grad(set_to_none=True)
            if r is not None:
                r.grad = None

        def lib():
            clear()
            y = bn(x)
            if r is not None:
                y = y + r
            (F.relu(y) if relu else y).backward(ct)

        def mine():
            clear()
            ops.BatchNormAct.apply(x, r, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps,
                                   relu).backward(ct)

        lib()
        ref = (x.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())
        mine()
        diff = [float((g - w).abs().max() / w.abs().max().clamp_min(1e-30)) for g, w in zip((x.grad, bn.weight.grad, bn.bias.grad), ref)]
        t_lib, t_mine = alternating_medians([lib, mine], a.iters)
        # each kernel alone: the bytes the operator has to move (inputs read once per pass that needs them, outputs written once)
        numel = 4.0 * x.numel()
        with torch.no_grad():
            xd = x.detach()
            rd = r.detach() if r is not None else None
            mean, rstd = ops.bn_stats(xd, bn.eps)
            y = ops.bn_act_forward(xd, rd, mean, rstd, bn.weight, bn.bias, relu)
            maps = 2 + int(relu)
            kernels = {
                "bn_stats": (lambda: ops.bn_stats(xd, bn.eps), numel),
                "bn_act_forward": (lambda: ops.bn_act_forward(xd, rd, mean, rstd, bn.weight, bn.bias, relu), numel * (2 + int(has_res))),
                "bn_act_backward": (lambda: ops.bn_act_backward(ct, xd, y if relu else None, mean, rstd, bn.weight, relu, training,
                                                                want=(True, has_res and relu, True, True)),
                                    numel * (2 * maps + 1 + int(has_res and relu))),
            }
            names = list(kernels)
            alone = alternating_medians([kernels[k][0] for k in names], a.iters)
        row = {"n": n, "C": C, "H": H, "W": W, "relu": relu, "residual": has_res, "training": training, "calls_per_step": calls,
               "map_MB": round(numel / 1e6, 2), "torch_fwd_bwd_ms": round(t_lib, 4), "kernel_fwd_bwd_ms": round(t_mine, 4),
               "dx_rel_diff_vs_torch": diff[0], "dgamma_rel_diff_vs_torch": diff[1], "dbeta_rel_diff_vs_torch": diff[2]}
        for k, ms in zip(names, alone):
            nbytes = kernels[k][1]
            row[k] = {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                      "share_of_6.3_TB_per_s": round(nbytes / (ms * 1e-3) / STREAM_BYTES_PER_S, 4)}
        rows.append(row)
        print(f"n{n} C{C:4d} {H:3d}x{W:3d} relu={int(relu)} res={int(has_res)} x{calls:2d}: torch {t_lib:7.3f} ms | kernels {t_mine:7.3f} ms | "
              + " | ".join(f"{k} {row[k]['ms']:.3f} ms {100 * row[k]['share_of_6.3_TB_per_s']:.0f}%" for k in names)
              + f" | dx / dgamma / dbeta rel diff {diff[0]:.1e} / {diff[1]:.1e} / {diff[2]:.1e}", flush=True)
    tot_lib = sum(r["torch_fwd_bwd_ms"] * r["calls_per_step"] for r in rows)
    tot_mine = sum(r["kernel_fwd_bwd_ms"] * r["calls_per_step"] for r in rows)
    stamp = os.path.join(ROOT, "heal_amd", "lib", "libheal_amd.stamp")
    result = {
        "what": "BatchNorm2d (+ residual) (+ ReLU) sites of one training step of configs.lidar_pyramid() (2 agents, full range), forward + "
                "backward per shape; medians of HIP-event timings, the two paths alternating; torch = batch_norm / add / relu under "
                "autograd, kernel = ops.BatchNormAct (ops.bn_grad('kernel'))",
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "streaming_rate_TB_per_s": STREAM_BYTES_PER_S / 1e12,
        "library_stamp": open(stamp).read().strip()[:12] if os.path.exists(stamp) else None,
        "step_ms": {k: round(v, 3) for k, v in step_ms.items()},
        "step_sites_by_route_over_the_timed_steps": routed,
        "sites_per_step": sum(seen.values()),
        "sites_sum_ms": {"torch": round(tot_lib, 3), "kernel": round(tot_mine, 3)},
        "sites_fraction_of_torch_step": round(tot_lib / step_ms["torch"], 4),
        "shapes": rows,
        "batchnorm2d_calls_outside_grad_bn_act (shape -> calls)": {str(k): v for k, v in sorted(outside.items())},
    }
    print(f"step: torch {step_ms['torch']:.2f} ms, kernel {step_ms['kernel']:.2f} ms; {sum(seen.values())} sites fwd+bwd summed: "
          f"torch {tot_lib:.2f} ms, kernel {tot_mine:.2f} ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
