"""The aligners of AlignNet beyond ConvNeXt: the library-operator path (default) against the reference's torch composition on the
same GPU (HEAL_ALIGN_FUSED=0), at the aligner's input in the 5-agent scene -- agents, channels and map size are read from
configs.lidar_pyramid(): max_cav agents x the backbone's last filter count x the LiDAR range over the voxel size and the backbone's
strides (5 x 64 x 256 x 256).

What is timed, both paths in 5 alternating rounds (medians with (min, max)), each figure the period of a captured graph
(ops.graph_period_ms):
  sdta_block        one SDTAEncoder (dim 64)
  sdta              the whole aligner, num_of_blocks 3, dim 64
  resnet1x1, resnet3x3, scaligner, cbam   num_of_blocks 3 (scaligner: num_of_layers 2), dim 64
  fanet             dim 64
  kernel alone      ops.xca_weights on the scene's qkv map (both launches).  The bytes are the compulsory ones -- q and k read once,
                    8 C N per image -- and the share is of the 6.3 TB/s a streaming kernel reaches on this chip.

    python scripts/align_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_amd import configs, ops  # noqa: E402
from heal_amd.opencood.models.sub_modules.bev_blocks import AlignNet  # noqa: E402

STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
ROUNDS, REPS, ITERS = 5, 5, 5
ALIGNERS = {
    "sdta": {"num_of_blocks": 3},
    "resnet1x1": {"num_of_blocks": 3},
    "resnet3x3": {"num_of_blocks": 3},
    "scaligner": {"num_of_blocks": 3, "num_of_layers": 2},
    "cbam": {"num_of_blocks": 3},
    "fanet": {},
}


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def scene_shape():
    hypes = configs.lidar_pyramid()
    m1 = hypes["model"]["args"]["m1"]
    r, vs = m1["encoder_args"]["lidar_range"], m1["encoder_args"]["voxel_size"]
    stride = int(np.prod(m1["backbone_args"]["layer_strides"]))
    H, W = int(round((r[4] - r[1]) / vs[1])) // stride, int(round((r[3] - r[0]) / vs[0])) // stride
    return int(hypes["train_params"]["max_cav"]), int(m1["backbone_args"]["num_filters"][-1]), H, W


def randomise(model, gen):
    """O(1) layer scales, distinct temperatures and non-trivial BatchNorm statistics: both paths then do the work of a trained model."""
    with torch.no_grad():
        for name, v in model.state_dict().items():
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("gamma", "gamma_xca"):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen))
            elif leaf == "temperature":
                v.copy_(torch.linspace(1.0, 8.0, v.numel()).reshape(v.shape))
            elif leaf == "running_var":
                v.copy_(0.5 + 1.5 * torch.rand(v.shape, generator=gen))
            elif leaf == "running_mean":
                v.copy_(torch.rand(v.shape, generator=gen) - 0.5)


def ab(fn, x):
    """{fused, torch} medians of fn(x) under the two settings of HEAL_ALIGN_FUSED, and the largest relative difference of the results."""
    times = {"fused": [], "torch": []}
    for _ in range(ROUNDS):                         # alternating rounds: the paths see the same neighbours on the machine
        for k, flag in (("fused", "1"), ("torch", "0")):
            os.environ["HEAL_ALIGN_FUSED"] = flag
            times[k].append(ops.graph_period_ms(lambda: fn(x), reps=REPS, iters=ITERS))
    os.environ["HEAL_ALIGN_FUSED"] = "1"
    a = fn(x)
    os.environ["HEAL_ALIGN_FUSED"] = "0"
    b = fn(x)
    os.environ["HEAL_ALIGN_FUSED"] = "1"
    row = {k: med(v) for k, v in times.items()}
    row["rel_diff_max"] = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
    return row


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["stream_TBs"] = STREAM_TBS
    B, C, H, W = scene_shape()
    out["shape"] = {"B": B, "C": C, "H": H, "W": W}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((B, C, H, W), generator=gen).cuda()
    rows = {}
    with torch.no_grad():
        for name, extra in ALIGNERS.items():
            model = AlignNet({"core_method": name, "args": dict(extra, dim=C)}).eval()
            randomise(model, gen)
            model = model.cuda()
            if name == "sdta":
                block = model.channel_align.model[1]
                calls = ops.XCA_CALLS["weights"]
                block(x)
                assert ops.XCA_CALLS["weights"] == calls + 1, "the SDTA block did not take the kernel path"
                rows["sdta_block"] = ab(block, x)
                print("sdta_block", rows["sdta_block"], flush=True)
            rows[name] = ab(model, x)
            print(name, rows[name], flush=True)
            del model
            torch.cuda.empty_cache()

        # the kernel alone
        heads, N = 4, H * W
        qkv = torch.randn((B, 3 * C, H, W), generator=gen).cuda()
        temp = torch.linspace(1.0, 8.0, heads).cuda()
        pw = (torch.randn((C, C), generator=gen) / C ** 0.5).cuda()
        row = med([ops.graph_period_ms(lambda: ops.xca_weights(qkv, temp, pw, heads), reps=20, iters=5) for _ in range(ROUNDS)])
        nbytes = 8.0 * C * N * B
        k_s = row["median_us"] * 1e-6
        row["parts_x_range"] = list(ops.xca_parts(B, heads, N))
        row["MB_compulsory"] = round(nbytes / 1e6, 2)
        row["TBs"] = round(nbytes / k_s / 1e12, 3)
        row["frac_of_stream_rate"] = round(nbytes / k_s / 1e12 / STREAM_TBS, 4)
        rows["kernel_xca_weights"] = row
        print("kernel xca_weights", row, flush=True)
    out.update(rows)
    out["fused_faster"] = {k: v["fused"]["median_us"] < v["torch"]["median_us"] for k, v in rows.items() if "fused" in v}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
