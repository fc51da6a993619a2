"""CoAlign multiscale fusion at full size (lidar_coalign.yaml: +-102.4 m, levels 64 x 256 x 256, 128 x 128 x 128, 256 x 64 x 64):
heal_warp_att_fuse_levels (one launch for the three levels) against the reference's torch composition on the same GPU
(HEAL_MSATT_FUSED=0) for 5 and 2 agents, the 256-channel level alone against the existing per-agent warp + permute + K6 chain
(AttFusion at 256 channels), and the whole HeterModelBaselineMs step replayed from a captured graph with the fused path on and
off.  The variants alternate round by round; every figure is the median over the rounds with (min, max).  Shares are of the
achievable-HBM bound of the compulsory bytes 4 * H * W * (n * C + C) per level.

    python scripts/coalign_bench.py [out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/coalign_bench.py --step-only     # one 5-agent scene step, a run of its own
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from heal_amd import configs, ops, synth  # noqa: E402
from heal_amd.opencood.models.fuse_modules.fusion_in_one import AttFusion, MaxFusion, fuse_levels  # noqa: E402
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm  # noqa: E402
from heal_amd.pipeline import Scene, ScenePipeline  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3       # bench.py's roofline constant for this part
LEVELS = [(64, 256, 256), (128, 128, 128), (256, 64, 64)]
ROUNDS = 5


def compulsory_bytes(n, levels):
    return sum(4.0 * H * W * (n * C + C) for C, H, W in levels)


def alternate(variants, rounds=ROUNDS, reps=5, warm=2):
    """variants: {name: fn}.  Every round times each variant once (mean of `reps` back-to-back calls between two HIP events), in
    turn -> {name: {"us": median, "min": .., "max": ..}}."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / reps * 1e3)
    out = {}
    for name, v in ts.items():
        v.sort()
        out[name] = {"us": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
    return out


def with_env(value, fn):
    def run():
        os.environ["HEAL_MSATT_FUSED"] = value
        try:
            return fn()
        finally:
            os.environ["HEAL_MSATT_FUSED"] = "1"
    return run


def step_only(n=5, steps=3):
    """A few eager steps of the full-size 5-agent scene and nothing else: what a kernel trace of the step needs."""
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
        pipe = ScenePipeline(configs.lidar_coalign(), "cuda:0", seed=0)
        scene = Scene(n, seed=40 + n, device="cuda:0")
        for _ in range(steps):
            pipe.step(scene)
    torch.cuda.synchronize()


def main():
    if "--step-only" in sys.argv:
        return step_only()
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS}
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        # ---- the fusion alone ----------------------------------------------------------------------------------------------------
        for n in (5, 2):
            feats = [(torch.randn((n, C, H, W), generator=gen) * C ** -0.25).cuda() for C, H, W in LEVELS]
            pw = synth.pairwise_t_matrix(synth.agent_poses(10 + n, n, r_min=5.0, r_max=60.0), 5)[None]
            aff = normalize_pairwise_tfm(pw, 204.8, 204.8, 1)
            for mode, net in (("att", torch.nn.ModuleList([AttFusion(C) for C, _, _ in LEVELS])),
                              ("max", torch.nn.ModuleList([MaxFusion() for _ in LEVELS]))):
                row = alternate({"fused": with_env("1", lambda: fuse_levels(net, feats, [n], aff)),
                                 "torch": with_env("0", lambda: fuse_levels(net, feats, [n], aff))})
                nbytes = compulsory_bytes(n, LEVELS)
                row["compulsory_MB"] = round(nbytes / 1e6, 1)
                row["fused_share_of_hbm"] = round(nbytes / (row["fused"]["us"] * 1e-6) / (HBM_ACHIEVABLE_TBS * 1e12), 3)
                row["speedup"] = round(row["torch"]["us"] / row["fused"]["us"], 2)
                a = fuse_levels(net, feats, [n], aff)
                b = with_env("0", lambda: fuse_levels(net, feats, [n], aff))()
                row["fused_vs_torch_rel_err"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
                out[f"fusion_{mode}_n{n}"] = row
                print(f"fusion_{mode}_n{n}", row, flush=True)
            # the 256-channel level alone: the new kernel with one level, the existing chain (one heal_warp_agent per agent, stack,
            # permute copy, K6, transpose back), the torch composition
            x = feats[2]
            att = AttFusion(256)
            net1 = torch.nn.ModuleList([att])
            row = alternate({"fused_one_level": with_env("1", lambda: fuse_levels(net1, [x], [n], aff)),
                             "k5_k6_chain": lambda: att(x, [n], aff),
                             "torch": with_env("0", lambda: fuse_levels(net1, [x], [n], aff))})
            nbytes = compulsory_bytes(n, LEVELS[2:])
            row["compulsory_MB"] = round(nbytes / 1e6, 1)
            row["fused_share_of_hbm"] = round(nbytes / (row["fused_one_level"]["us"] * 1e-6) / (HBM_ACHIEVABLE_TBS * 1e12), 3)
            row["chain_vs_fused_rel_err"] = float((att(x, [n], aff)[0] - fuse_levels(net1, [x], [n], aff)[0][0]).abs().max()
                                                  / att(x, [n], aff).abs().max())
            out[f"level256_n{n}"] = row
            print(f"level256_n{n}", row, flush=True)
            del feats, x
        torch.cuda.empty_cache()
        # ---- the whole model step, replayed from a captured graph ----------------------------------------------------------------
        for n in (5, 2):
            scene = Scene(n, seed=40 + n, device="cuda:0")
            pipes = {}
            for name, value in (("fused", "1"), ("torch", "0")):
                os.environ["HEAL_MSATT_FUSED"] = value       # the path is chosen when the step is captured
                pipes[name] = ScenePipeline(configs.lidar_coalign(), "cuda:0", seed=0)
                pipes[name].capture(scene, warmup=2)
            os.environ["HEAL_MSATT_FUSED"] = "1"
            row = alternate({k: (lambda p=p: p.replay(scene)) for k, p in pipes.items()}, reps=3)
            row["scenes_per_s_fused"] = round(1e6 / row["fused"]["us"], 1)
            row["scenes_per_s_torch"] = round(1e6 / row["torch"]["us"], 1)
            out[f"scene_replay_n{n}"] = row
            print(f"scene_replay_n{n}", row, flush=True)
            del pipes
            torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
