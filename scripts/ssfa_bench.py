"""The SSFA neck of the SECOND + SSFA detectors at 5 x 128 x 100 x 352 -- the SECOND BEV map of the +-140.8 m x +-40 m range at
stride 8 (configs.second_ssfa's default range), five frames: this library's operators against the reference's torch composition on the
same GPU.

What is timed, both sides in 5 alternating rounds (medians with (min, max)), each figure the period of a captured graph
(ops.graph_period_ms):
  neck      SSFA.forward, HEAL_SSFA_FUSED=1 against HEAL_SSFA_FUSED=0 (eval mode, BatchNorm with non-trivial statistics)
  deconv    ONE heal_deconv3x3_s2 launch (256 -> 256 at 50 x 176, bias, ReLU, residual on the first 128 channels) against what it
            replaces: two F.conv_transpose2d (256 -> 128) + eval BatchNorm + ReLU and the residual add.  FLOPs are the useful ones,
            2 x 9 Cin Cout per input pixel; the share is of the 157.3 TFLOP/s fp32 matrix peak
  blend     ONE heal_ssfa_blend launch against its composition (two 128 -> 1 convolutions + BatchNorm, cat, softmax, two products and
            a sum).  The bytes are the compulsory ones -- two maps read, one written -- and the share is of the 6.3 TB/s a streaming
            kernel reaches on this chip

    python scripts/ssfa_bench.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from heal_amd import configs, ops  # noqa: E402
from heal_amd.opencood.models.sub_modules.cia_ssd_utils import SSFA  # noqa: E402

FP32_PEAK_TFLOPS = 157.3      # bench.py
STREAM_TBS = 6.3              # what a streaming kernel reaches (copy rate), of 8.0 TB/s HBM3E peak
ROUNDS, REPS, ITERS = 5, 5, 5
FRAMES = 5


def med(ts):
    ts = sorted(ts)
    return {"median_us": round(ts[len(ts) // 2] * 1e3, 1), "min_us": round(ts[0] * 1e3, 1), "max_us": round(ts[-1] * 1e3, 1)}


def scene_shape():
    hypes = configs.second_ssfa()
    r, vs = hypes["model"]["args"]["lidar_range"], hypes["model"]["args"]["voxel_size"]
    stride = hypes["postprocess"]["anchor_args"]["feature_stride"]
    return (FRAMES, hypes["model"]["args"]["ssfa"]["feature_num"], int(round((r[4] - r[1]) / vs[1])) // stride,
            int(round((r[3] - r[0]) / vs[0])) // stride)


def randomise(model, gen):
    with torch.no_grad():
        for name, v in model.state_dict().items():
            leaf = name.rsplit(".", 1)[-1]
            if leaf == "running_var":
                v.copy_(0.5 + 1.5 * torch.rand(v.shape, generator=gen))
            elif leaf == "running_mean":
                v.copy_(torch.rand(v.shape, generator=gen) - 0.5)


def ab(fused, composed):
    """{fused, torch} medians of the two callables in alternating rounds, and the largest relative difference of their results."""
    times = {"fused": [], "torch": []}
    for _ in range(ROUNDS):                         # alternating rounds: the two sides see the same neighbours on the machine
        for k, fn in (("fused", fused), ("torch", composed)):
            times[k].append(ops.graph_period_ms(fn, reps=REPS, iters=ITERS))
    a, b = fused(), composed()
    row = {k: med(v) for k, v in times.items()}
    row["rel_diff_max"] = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    row["speedup_fused_over_torch"] = round(row["torch"]["median_us"] / row["fused"]["median_us"], 2)
    return row


def main():
    out = {}
    stamp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heal_amd", "lib", "libheal_amd.stamp")
    out["library_stamp"] = open(stamp).read().strip()[:12] if os.path.exists(stamp) else None
    out["device"] = torch.cuda.get_device_name(0)
    out["fp32_peak_TFLOPs"], out["stream_TBs"] = FP32_PEAK_TFLOPS, STREAM_TBS
    n, C, H, W = scene_shape()
    out["shape"] = {"n": n, "C": C, "H": H, "W": W}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    model = SSFA({"feature_num": C}).eval()
    randomise(model, gen)
    model = model.cuda()
    x = torch.randn((n, C, H, W), generator=gen).cuda()
    rows = {}
    with torch.no_grad():
        def neck(flag):
            def run():
                os.environ["HEAL_SSFA_FUSED"] = flag
                try:
                    return model(x)
                finally:
                    os.environ["HEAL_SSFA_FUSED"] = "1"
            return run
        calls = dict(ops.SSFA_CALLS)
        neck("1")()
        assert ops.SSFA_CALLS == {"deconv": calls["deconv"] + 1, "blend": calls["blend"] + 1}, "SSFA did not take the kernel path"
        rows["neck"] = ab(neck("1"), neck("0"))
        print("neck", rows["neck"], flush=True)

        # the transposed convolution alone: both deblocks
        x1 = torch.relu(torch.randn((n, 2 * C, H // 2, W // 2), generator=gen)).cuda()
        res = torch.relu(torch.randn((n, C, H, W), generator=gen)).cuda()
        frag, bias = model._deconv_pair()
        d0, d1 = model.deconv_block_0, model.deconv_block_1

        def deconv_torch():
            return torch.cat([d0(x1) + res, d1(x1)], dim=1)
        row = ab(lambda: ops.deconv3x3_s2(x1, frag, bias, relu=True, residual=res), deconv_torch)
        two = med([ops.graph_period_ms(lambda: (d0(x1) + res, d1(x1)), reps=REPS, iters=ITERS) for _ in range(ROUNDS)])
        row["torch_without_cat"] = two              # the composition keeps two maps; the cat above only makes the results comparable
        raw = med([ops.graph_period_ms(lambda: F.conv_transpose2d(x1, torch.cat([d0[0].weight, d1[0].weight], 1), None, 2, 1, 1),
                                       reps=REPS, iters=ITERS) for _ in range(ROUNDS)])
        row["library_conv_transpose2d_256_256_alone"] = raw
        flops = 2.0 * 9 * n * (2 * C) * (2 * C) * (H // 2) * (W // 2)
        k_s = row["fused"]["median_us"] * 1e-6
        row["GFLOP_useful"] = round(flops / 1e9, 2)
        row["TFLOPs"] = round(flops / k_s / 1e12, 2)
        row["frac_of_fp32_mfma_peak"] = round(flops / k_s / 1e12 / FP32_PEAK_TFLOPS, 4)
        row["fused_over_torch_without_cat"] = round(two["median_us"] / row["fused"]["median_us"], 2)
        rows["deconv"] = row
        print("deconv", row, flush=True)

        # the blend alone
        a, b = (torch.randn((n, C, H, W), generator=gen).cuda() for _ in range(2))
        from heal_amd.opencood.models.sub_modules.bev_blocks import fold_bn
        (wa, ba), (wb, bb) = fold_bn(*model.w_0[:2]), fold_bn(*model.w_1[:2])

        def blend_torch():
            s = torch.softmax(torch.cat([model.w_0(a), model.w_1(b)], dim=1), dim=1)
            return a * s[:, 0:1] + b * s[:, 1:]
        row = ab(lambda: ops.ssfa_blend(a, b, wa, ba, wb, bb), blend_torch)
        nbytes = 12.0 * n * C * H * W
        k_s = row["fused"]["median_us"] * 1e-6
        row["MB_compulsory"] = round(nbytes / 1e6, 2)
        row["TBs"] = round(nbytes / k_s / 1e12, 3)
        row["frac_of_stream_rate"] = round(nbytes / k_s / 1e12 / STREAM_TBS, 4)
        rows["blend"] = row
        print("blend", row, flush=True)
    out.update(rows)
    out["fused_faster"] = {k: v["fused"]["median_us"] < v["torch"]["median_us"] for k, v in rows.items()}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
