"""warp_affine_simple of the gradient path, forward + backward: this library's kernels (ops.WarpAffine: heal_warp_affine_forward and
the gather-form heal_warp_affine_backward; ops.warp_grad("kernel")) against F.affine_grid + F.grid_sample under autograd.

Part one: forward + backward per shape (n x C x H x W: 5 x 256 x 128 x 128, 5 x 256 x 256 x 256, 2 x 64 x 64 x 64), rigid rows; 3
warm-ups, then HIP events around each of `--iters` (>= 5) calls, the two paths ALTERNATING in one run, median.  Each kernel is also
timed alone and reported with its compulsory bytes (read the map once, write it once: 8 n C H W) as a share of the 6.3 TB/s
streaming rate.
Part two: one training step (forward, loss, backward) of configs.lidar_coalign("att") and configs.lidar_baseline("att"), 3 agents, in
both modes, alternating, median of 5.  Decides nothing by itself: the default stays "torch".

    python scripts/warp_grad_bench.py [--iters 9] [--out profiles/warp_grad_bench.json]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from heal_amd import configs, ops
from heal_amd.opencood.tools.train_utils import create_model
from heal_amd.pipeline import Scene, fill_deterministic

STREAM_BYTES_PER_S = 6.3e12
SHAPES = [(5, 256, 128, 128), (5, 256, 256, 256), (2, 64, 64, 64)]


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


def rigid_rows(n, H, W, seed):
    """The ego's identity and n - 1 seeded rigid rows (any angle, the centre shifted by up to 15 % of the map)."""
    rng = np.random.default_rng(seed)
    rows = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]]
    for _ in range(n - 1):
        th, tx, ty = rng.uniform(0, 2 * math.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)
        c, s = math.cos(th), math.sin(th)
        rows.append([c, -s * H / W, tx, s * W / H, c, ty])
    return np.asarray(rows, dtype=np.float64).reshape(n, 2, 3)


def bench_shape(n, C, H, W, iters, dev):
    torch.manual_seed(C + H)
    rows = rigid_rows(n, H, W, n + H)
    M = torch.from_numpy(rows).to(dev)
    x = torch.randn(n, C, H, W, device=dev, requires_grad=True)
    ct = torch.randn(n, C, H, W, device=dev)
    assert ops.warp_affine_train_supported(x, rows)

    def lib():
        x.grad = None
        F.grid_sample(x, F.affine_grid(M, [n, C, H, W], align_corners=False).to(x), align_corners=False).backward(ct)

    def mine():
        x.grad = None
        ops.WarpAffine.apply(x, rows, True).backward(ct)

    lib()
    ref = x.grad.clone()
    mine()
    diff = float((x.grad - ref).abs().max() / ref.abs().max())
    t_lib, t_mine = alternating_medians([lib, mine], iters)
    nbytes = 8.0 * n * C * H * W
    with torch.no_grad():
        xd = x.detach()
        alone = alternating_medians([lambda: ops.warp_affine(xd, rows, True), lambda: ops.warp_affine_backward(ct, rows, True),
                                     lambda: F.grid_sample(xd, F.affine_grid(M, [n, C, H, W], align_corners=False).to(xd),
                                                           align_corners=False)], iters)
    row = {"n": n, "C": C, "H": H, "W": W, "map_MB": round(4.0 * n * C * H * W / 1e6, 2), "torch_fwd_bwd_ms": round(t_lib, 4),
           "kernel_fwd_bwd_ms": round(t_mine, 4), "dx_rel_diff_vs_torch": diff,
           "torch_affine_grid_grid_sample_forward_ms": round(alone[2], 4)}
    for k, ms in zip(("warp_affine_forward", "warp_affine_backward"), alone):
        row[k] = {"ms": round(ms, 4), "compulsory_bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                  "share_of_6.3_TB_per_s": round(nbytes / (ms * 1e-3) / STREAM_BYTES_PER_S, 4)}
    print(f"{n} x {C} x {H} x {W}: torch {t_lib:.3f} ms | kernels {t_mine:.3f} ms | forward {alone[0]:.3f} ms "
          f"{100 * row['warp_affine_forward']['share_of_6.3_TB_per_s']:.0f}% | backward {alone[1]:.3f} ms "
          f"{100 * row['warp_affine_backward']['share_of_6.3_TB_per_s']:.0f}% | dx rel diff {diff:.1e}", flush=True)
    return row


def bench_step(name, hypes, dev):
    model = fill_deterministic(create_model(hypes), 0).to(dev).train()
    data = Scene(3, seed=9, device=dev).model_input()

    def step():
        model.zero_grad(set_to_none=True)
        out = model(data)
        sum(out[k].square().mean() for k in ("cls_preds", "reg_preds", "dir_preds")).backward()

    def step_in(mode):
        def run():
            with ops.warp_grad(mode):
                step()
        return run
    routed = {}
    for mode in ("torch", "kernel"):
        before = dict(ops.WARP_GRAD_CALLS)
        step_in(mode)()
        routed[mode] = {k: ops.WARP_GRAD_CALLS[k] - before[k] for k in before}
    ms = dict(zip(("torch", "kernel"), alternating_medians([step_in("torch"), step_in("kernel")], 5, warm=2)))
    print(f"{name}: step torch {ms['torch']:.2f} ms, kernel {ms['kernel']:.2f} ms; warps per step {routed}", flush=True)
    return {"step_ms": {k: round(v, 3) for k, v in ms.items()}, "warps_per_step_by_route": routed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "warp_grad_bench needs a GPU"
    assert a.iters >= 5
    dev = torch.device("cuda:0")
    shapes = [bench_shape(*s, a.iters, dev) for s in SHAPES]
    steps = {"lidar_coalign(att)": bench_step("lidar_coalign(att)", configs.lidar_coalign("att"), dev),
             "lidar_baseline(att)": bench_step("lidar_baseline(att)", configs.lidar_baseline("att"), dev)}
    stamp = os.path.join(ROOT, "heal_amd", "lib", "libheal_amd.stamp")
    result = {
        "what": "warp_affine_simple forward + backward per shape, and one training step of two models (3 agents, full range) in both "
                "ops.warp_grad modes; medians of HIP-event timings, the two paths alternating in one run; torch = F.affine_grid + "
                "F.grid_sample under autograd, kernel = ops.WarpAffine",
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "streaming_rate_TB_per_s": STREAM_BYTES_PER_S / 1e12,
        "library_stamp": open(stamp).read().strip()[:12] if os.path.exists(stamp) else None,
        "shapes": shapes, "training_steps": steps,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
