"""Where2comm's communication path: the fused path (heal_comm_mask + one heal_warp_att_fuse_levels_masked launch per scene) against the
reference's torch composition on the same GPU (HEAL_COMM_FUSED=0: sigmoid, max, Conv2d, threshold, override, max_pool2d per level,
x * mask, affine_grid + grid_sample and the per-pixel attention), at the shape DESIGN.md section 18 uses for Where2comm: one scene
of 5 agents x 256 x 128 x 128 single-scale, and three levels of 64 / 128 / 256 channels at 128 / 64 / 32 cells for the multi-scale
form (the levels as `backbone.resnet` hands them over: what is timed is the communication + fusion, not the backbone).

What is timed, both paths in 5 alternating rounds (medians with (min, max)), each as a captured graph (ops.graph_period_ms):
  single_scale / multi_scale   masks (all levels) + masked fusion of every level, mode ATTEN
  kernels alone                ops.comm_mask and ops.warp_att_fuse_levels(masks=...) with the bytes they must move -- the logits
                               read once and the masks written once; every agent's map and mask read once and the fused map written
                               once -- as a share of the 6.3 TB/s a streaming kernel reaches on this chip

    python scripts/w2c_comm_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import ops  # noqa: E402
from heal_amd.opencood.models.comm_modules.where2comm import Communication  # noqa: E402
from heal_amd.opencood.models.fuse_modules.where2comm_attn import Where2comm  # noqa: E402

STREAM_TBS = 6.3
N, HW = 5, 128
LEVELS = [(64, 128), (128, 64), (256, 32)]
ROUNDS = 5


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["stream_TBs"] = STREAM_TBS
    out["shape"] = {"agents": N, "single_scale": [256, HW, HW], "multi_scale": [[c, s, s] for c, s in LEVELS], "filter": 5}
    torch.cuda.set_stream(torch.cuda.Stream())
    dev = "cuda"
    rng = np.random.default_rng(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    rm = (torch.randn((N, 2, HW, HW), generator=g) * 1.5).to(dev)
    poses = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (1, N, N, 1, 1))
    for j in range(1, N):
        t = rng.uniform(-np.pi, np.pi)
        poses[0, 0, j] = [[np.cos(t), -np.sin(t), rng.uniform(-0.4, 0.4)], [np.sin(t), np.cos(t), rng.uniform(-0.4, 0.4)]]
    aff = torch.from_numpy(poses).to(dev)
    comm = Communication({"thre": 0.68, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}).to(dev).eval()
    lens = [N]

    def module(multi_scale):
        return Where2comm({"voxel_size": [0.4, 0.4, 4], "downsample_rate": 1, "multi_scale": multi_scale, "layer_nums": [1, 1, 1],
                           "num_filters": [c for c, _ in LEVELS], "agg_operator": {"mode": "ATTEN", "feature_dim": 256},
                           "communication": {"thre": 0.68, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}}).to(dev).eval()
    forms = {"single_scale": (module(False), [(torch.randn((N, 256, HW, HW), generator=g) * 0.25).to(dev)]),
             "multi_scale": (module(True), [(torch.randn((N, c, s, s), generator=g) * c ** -0.25).to(dev) for c, s in LEVELS])}

    def step(form):
        m, feats = forms[form]
        with torch.no_grad():
            masks, rate = m._masks(rm, lens, len(feats), rm.device)
            mods = m.fuse_modules if form == "multi_scale" else [m.fuse_modules]
            return m._fuse(mods, feats, masks, [False] * len(feats), lens, aff), rate

    rows, ok = {}, True
    for form in forms:
        times = {"fused": [], "torch": []}
        for _ in range(ROUNDS):                      # alternating rounds: the paths see the same neighbours on the machine
            for k, flag in (("fused", "1"), ("torch", "0")):
                os.environ["HEAL_COMM_FUSED"] = flag
                times[k].append(ops.graph_period_ms(lambda: step(form), reps=10, iters=5))
        row = {k: med(v) for k, v in times.items()}
        os.environ["HEAL_COMM_FUSED"] = "1"
        ya, ra = step(form)
        os.environ["HEAL_COMM_FUSED"] = "0"
        yb, rb = step(form)
        os.environ["HEAL_COMM_FUSED"] = "1"
        row["rel_diff_max"] = max(rel(a, b) for a, b in zip(ya, yb))
        row["same_rate"] = bool(float(ra) == float(rb))
        row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
        ok = ok and row["fused"]["median_us"] < row["torch"]["median_us"]
        rows[form] = row
        print(form, row, flush=True)

    # the kernels alone
    w, b = comm.gaussian_filter.weight, comm.gaussian_filter.bias
    masks3, _, _ = ops.comm_mask(rm, lens, w, b, 0.68, 3)
    ss, ms = forms["single_scale"][1], forms["multi_scale"][1]
    sd = [float(np.sqrt(c)) for c, _ in LEVELS]
    kernels = {
        "comm_mask_1_level": (lambda: ops.comm_mask(rm, lens, w, b, 0.68, 1), 4 * (rm.numel() + N * HW * HW)),
        "comm_mask_3_levels": (lambda: ops.comm_mask(rm, lens, w, b, 0.68, 3), 4 * (rm.numel() + sum(m.numel() for m in masks3))),
        "fuse_masked_single_scale": (lambda: ops.warp_att_fuse_levels(ss, aff[0, 0], True, "att", [16.0], masks=masks3[:1]),
                                     4 * (ss[0].numel() + masks3[0].numel() + 256 * HW * HW)),
        "fuse_unmasked_single_scale": (lambda: ops.warp_att_fuse_levels(ss, aff[0, 0], True, "att", [16.0]),
                                       4 * (ss[0].numel() + 256 * HW * HW)),
        "fuse_masked_multi_scale": (lambda: ops.warp_att_fuse_levels(ms, aff[0, 0], True, "att", sd, masks=masks3),
                                    4 * sum(f.numel() + m.numel() + f.numel() // N for f, m in zip(ms, masks3))),
        "fuse_unmasked_multi_scale": (lambda: ops.warp_att_fuse_levels(ms, aff[0, 0], True, "att", sd),
                                      4 * sum(f.numel() + f.numel() // N for f in ms)),
    }
    for name, (fn, nbytes) in kernels.items():
        row = med([ops.graph_period_ms(fn, reps=20, iters=5) for _ in range(ROUNDS)])
        k_s = row["median_us"] * 1e-6
        row["MB_compulsory"] = round(nbytes / 1e6, 2)
        row["TBs"] = round(nbytes / k_s / 1e12, 3)
        row["frac_of_stream_rate"] = round(nbytes / k_s / 1e12 / STREAM_TBS, 4)
        rows["kernel_" + name] = row
        print("kernel", name, row, flush=True)
    out.update(rows)
    out["ones_share_of_the_masks"] = round(float(masks3[0].mean()), 3)
    out["fused_faster_at_every_row"] = ok
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
