"""Generate tests/golden/w2c_comm_small.npz and w2c_comm_state_dict_keys.json by IMPORTING the reference (build container only).

    python -m tests.golden.gen_golden_w2c_comm

Where2comm's communication path: comm_modules/where2comm.py (Communication), fuse_modules/where2comm_attn.py (Where2comm) and
models/center_point_where2comm.py.  Inputs, settings and the reference's outputs only.  where2comm_attn.py starts with
`from turtle import update`: `turtle` is stubbed first.

Mask cases (tests/golden/w2c_comm_margins.py names them): the REFERENCE's Communication.forward on the CPU, then F.max_pool2d per
further level as Where2comm.forward applies it (:264-275).  Stored per case: the logits, the filter's weight and bias, the threshold,
the masks of every level (uint8), the rate, and the first agents' counts before the override.  The margin of w2c_comm_margins.py is
asserted on what is written, and the reference's own fp32 masks must equal the float64 restatement's (tests/comm_refs.py).

Module cases (prefix att_ / max_ x ss_ / plain_ / res_): Where2comm on a 32 x 32 map of 0.8 m cells (+-12.8 m), scenes of 3 and 2
agents, 64 input channels; the multi-scale forms with the reference's BaseBEVBackbone / ResNetBEVBackbone (one block per level,
widths 64 / 128 / 256, strides 1 / 2 / 2, weights from detfill.fill_module).  The input maps are not stored: they are the closed
form module_input() below, which the tests evaluate themselves.  One neighbour of the first scene sits 11 m from the ego, so part of
its footprint leaves the map (asserted).  The outputs are stored on every OUT_STRIDE-th channel.
Model case (m_): CenterPointWhere2comm (ATTEN, multi-scale, resnet) on the three agents of center_small.npz's model case (the same
model_inputs(); asserted equal, so the voxels are not stored twice), weights from w2c_comm_margins.model_fill (detfill.fill_module -- the filter's included, which makes
it a perturbed filter with a bias -- and a gain on the score head, without which the confidence map is nearly constant).  The threshold is picked where the reference's smoothed confidence keeps the margin."""
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from heal_amd import configs, synth
from tests import comm_refs as CR
from tests.golden import ref_import as R
from tests.golden import w2c_comm_margins as WM
from tests.golden.detfill import fill_module
from tests.golden.gen_golden import OUT, _rng, save
from tests.golden.gen_golden_kd import M_RANGE, model_inputs

OUT_STRIDE = {"ss": 8, "ms": 48}          # channels kept of the fused maps: 64 / 8 and 384 / 48 (at least two per level)
BACKBONE = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256], "upsample_strides": [1, 2, 4],
            "num_upsample_filter": [128, 128, 128]}


def ref_modules():
    R.install()
    sys.modules.setdefault("turtle", types.ModuleType("turtle"))
    sys.modules["turtle"].__dict__.setdefault("update", None)
    return (R.ref("opencood.models.comm_modules.where2comm"), R.ref("opencood.models.fuse_modules.where2comm_attn"),
            R.ref("opencood.models.center_point_where2comm"))


def module_input(n, C, H, W):
    """The module cases' feature maps in closed form: integer codes over 8 (exact in fp32), never stored."""
    idx = np.arange(n * C * H * W, dtype=np.float64)
    code = np.round(12.0 * np.sin(idx * 0.6180339887 + 0.37) * np.cos(idx * 0.0137))
    return (code / 8.0).astype(np.float32).reshape(n, C, H, W)


def logits(rng, n, A, H, W):
    """Confidence logits with structure at the scale of a few cells (so that the pooled levels keep zeros) under noise."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = rng.standard_normal((n, A, H, W)) * 0.8 - 0.3
    for i in range(n):
        for a in range(A):
            fy, fx, ph = rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5), rng.uniform(0, 2 * np.pi)
            out[i, a] += 2.5 * np.sin(2 * np.pi * (fy * ys / max(H, 8) + fx * xs / max(W, 8)) + ph)
    return out.astype(np.float32)


def settle(psm, weight, bias, record_len, n_levels, prefix):
    """Pick the threshold, then nudge the logits of pixels whose smoothed value is within the margin of it."""
    thre = None
    for _ in range(200):
        s = CR.smoothed(psm, weight, bias)
        if thre is None:
            thre = float(np.float32(WM.pick_threshold(s)))
        bad = np.argwhere(np.abs(s - thre) < 2 * WM.MARGIN)
        if not len(bad):
            break
        for n, y, x in bad:
            psm[n, :, y, x] += np.float32(0.25 if s[n, y, x] > thre else -0.25)
    else:
        raise AssertionError(f"{prefix}: the margin did not settle")
    return thre


def gen_mask_cases(comm_mod, out):
    for i, (prefix, (H, W, A, k, levels)) in enumerate(WM.MASK_CASES.items()):
        rng = _rng(900 + i)
        n = sum(WM.RECORD_LEN)
        psm = logits(rng, n, A, H, W)
        if prefix == "ext_":
            hit = rng.random((n, A, H, W)) < 0.1
            psm[hit] = np.where(rng.random(int(hit.sum())) < 0.5, 30.0, -30.0).astype(np.float32)
        args = {"thre": 0.5}
        if k:
            args["gaussian_smooth"] = {"k_size": k, "c_sigma": 1.0}
        module = comm_mod.Communication(args).eval()
        weight = bias = None
        if k:
            if prefix == "par_":
                with torch.no_grad():
                    module.gaussian_filter.weight.mul_(torch.from_numpy(rng.uniform(0.6, 1.4, (1, 1, k, k)).astype(np.float32)))
                    module.gaussian_filter.bias.fill_(0.05)
            weight = module.gaussian_filter.weight.detach().numpy().reshape(k, k).copy()
            bias = module.gaussian_filter.bias.detach().numpy().copy()
            if prefix != "par_":
                assert np.array_equal(weight, WM.gaussian_weight(k, 1.0)) and bias[0] == 0
        module.thre = settle(psm, weight, bias if k else 0.0, WM.RECORD_LEN, levels, prefix)
        maps = torch.split(torch.from_numpy(psm), WM.RECORD_LEN)
        with torch.no_grad():
            _, mask, rate = module(maps, torch.tensor(WM.RECORD_LEN), torch.zeros((2, 5, 5, 4, 4)))
            lv = [mask]
            for _ in range(1, levels):
                lv.append(F.max_pool2d(lv[-1], kernel_size=2))
            # the first agents' counts before the override: the module's own filter and comparison once more (:52-63)
            count = []
            for m in maps:
                c = m[:1].sigmoid().max(dim=1)[0].unsqueeze(1)
                count.append(int(((module.gaussian_filter(c) if k else c) > module.thre).sum()))
        c = dict(psm=psm, thre=module.thre, n_levels=levels, record_len=WM.RECORD_LEN, k=k, weight=weight, bias=bias)
        ch = WM.chain(c)
        assert ch["margin"] >= WM.MARGIN, (prefix, ch["margin"])
        assert WM.is_mixed(ch["raw"], prefix), prefix
        if min(H, W) >= 8:                                       # the coarsest level still tells a wrong pooling from a right one
            top = ch["masks"][-1][list(WM.FREE)]
            assert 0 < top.mean() < 1, (prefix, top.mean())
        for l in range(levels):                                  # the reference's fp32 result against the float64 restatement
            assert np.array_equal(lv[l].numpy()[:, 0].astype(np.uint8), ch["masks"][l]), (prefix, l)
        assert count == ch["count"].tolist() and np.float32(rate) == ch["rate"], (prefix, count, ch["count"], rate, ch["rate"])
        out.update({prefix + "psm": psm, prefix + "thre": np.float32(module.thre), prefix + "rate": np.float32(rate),
                    prefix + "count": np.array(count, np.int32)})
        if k:
            out.update({prefix + "weight": weight, prefix + "bias": bias})
        for l in range(levels):
            out[f"{prefix}mask{l}"] = lv[l].numpy().astype(np.uint8)
        print(f"{prefix}: thre {module.thre:.6f} margin {ch['margin']:.2e} rate {float(rate):.4f} count {count} ones per level "
              f"{[int(m.sum()) for m in lv]}")
    assert np.abs(out["ext_psm"]).max() == 30 and out["par_bias"][0] == np.float32(0.05)
    assert [out["odd_mask1"].shape[2:], out["odd_mask2"].shape[2:]] == [(6, 5), (3, 2)]


def module_pairwise():
    """Scene 0: three agents, agent 1 at 11 m (part of its footprint leaves the +-12.8 m map); scene 1: two agents."""
    p0 = synth.agent_poses(931, 3, r_min=3.0, r_max=6.0)
    p0[1][0], p0[1][1] = 11.0 * np.cos(0.7), 11.0 * np.sin(0.7)
    p1 = synth.agent_poses(932, 2, r_min=3.0, r_max=6.0)
    return np.stack([synth.pairwise_t_matrix(p0, 5), synth.pairwise_t_matrix(p1, 5)])


def module_args(mode, multi_scale, thre):
    return {"voxel_size": [WM.MODULE_VOXEL, WM.MODULE_VOXEL, 4], "downsample_rate": 1, "multi_scale": multi_scale,
            "layer_nums": BACKBONE["layer_nums"], "num_filters": BACKBONE["num_filters"],
            "agg_operator": {"mode": mode, "feature_dim": 64},
            "communication": {"thre": thre, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}}


def gen_module_cases(attn_mod, out):
    bb_plain = R.ref("opencood.models.sub_modules.base_bev_backbone")
    bb_res = R.ref("opencood.models.sub_modules.base_bev_backbone_resnet")
    tu = R.ref("opencood.models.sub_modules.torch_transformation_utils")
    n, HW = sum(WM.RECORD_LEN), WM.MODULE_HW
    x = torch.from_numpy(module_input(n, 64, HW, HW))
    rng = _rng(940)
    rm = logits(rng, n, 1, HW, HW)
    w = WM.gaussian_weight(5, 1.0)
    thre = settle(rm, w, 0.0, WM.RECORD_LEN, 3, "module")
    ch = CR.mask_chain(rm, WM.RECORD_LEN, w, 0.0, thre, 3)
    assert ch["margin"] >= WM.MARGIN and WM.is_mixed(ch["raw"], "module")
    pw = module_pairwise()
    out.update({"mod_rm": rm, "mod_thre": np.float32(thre), "mod_pairwise": pw, "mod_rate": ch["rate"]})
    # part of a footprint leaves the map: the warp of a map of ones has zeros for agent 1 of scene 0
    aff = torch.from_numpy(pw.copy())[:, :, :, [0, 1], :][:, :, :, :, [0, 1, 3]]
    aff[..., 0, 2] = aff[..., 0, 2] / (WM.MODULE_VOXEL * HW) * 2
    aff[..., 1, 2] = aff[..., 1, 2] / (WM.MODULE_VOXEL * HW) * 2
    cover = tu.warp_affine_simple(torch.ones((3, 1, HW, HW)), aff[0, 0, :3], (HW, HW))
    share = float((cover[1] == 0).float().mean())
    assert 0.1 < share < 0.9, share
    for prefix, (mode, multi_scale, form) in WM.MODULE_CASES.items():
        module = attn_mod.Where2comm(module_args(mode, multi_scale, thre)).eval()
        backbone = None
        if form is not None:
            cfg = copy.deepcopy(BACKBONE)
            backbone = fill_module((bb_res.ResNetBEVBackbone if form == "resnet" else bb_plain.BaseBEVBackbone)(cfg, 64)).eval()
        with torch.no_grad():
            y, rate, extra = module(x.clone(), torch.from_numpy(rm), torch.tensor(WM.RECORD_LEN), torch.from_numpy(pw.copy()), backbone)
        assert extra == {} and np.float32(rate) == ch["rate"], (prefix, rate, ch["rate"])
        stride = OUT_STRIDE["ms" if multi_scale else "ss"]
        out[prefix + "out"] = y.numpy()[:, ::stride]
        print(prefix, tuple(y.shape), "rate", float(rate), "|y| max", float(y.abs().max()))


def model_args(hypes, thre=None):
    args = copy.deepcopy(hypes["model"]["args"])
    lidar_range = args["lidar_range"]
    args["point_pillar_scatter"]["grid_size"] = np.round(
        (np.array(lidar_range[3:]) - np.array(lidar_range[:3])) / np.array(args["voxel_size"])).astype(np.int64)
    if thre is not None:
        args["fusion_args"]["communication"]["thre"] = thre
    return args


def gen_model_case(model_mod, out):
    s_in, _, pw = model_inputs()
    center = np.load(os.path.join(OUT, "center_small.npz"))
    for k, v in s_in.items():
        assert np.array_equal(center[f"m3_{k}"], v), k            # the tests read the voxels from center_small.npz
    assert np.array_equal(center["m3_pairwise"], pw)
    hypes = configs.lidar_centerpoint_where2comm("ATTEN", True, "resnet", True, M_RANGE)
    data = lambda: {"processed_lidar": {k: torch.from_numpy(v) for k, v in s_in.items()}, "record_len": torch.tensor([3]),   # noqa: E731
                    "pairwise_t_matrix": torch.from_numpy(pw.copy())}
    probe = WM.model_fill(model_mod.CenterPointWhere2comm(model_args(hypes))).eval()
    with torch.no_grad():
        psm = probe(data())["cls_preds_single"].numpy()           # does not depend on the threshold
    f = probe.fusion_net.naive_communication.gaussian_filter
    w, b = f.weight.detach().numpy().reshape(5, 5), f.bias.detach().numpy()
    # the logits cannot be nudged here: the threshold goes into the widest gap of the values whose comparison reaches an output
    # (agent 0: the count; agent 1: its mask; agent 2 is forced and not the ego), inside the middle of agent 1's values
    s = CR.smoothed(psm, w, b)
    v = np.sort(s[:2].reshape(-1))
    lo, hi = np.quantile(s[1], [0.3, 0.7])
    gaps = [(v[i + 1] - v[i], 0.5 * (v[i] + v[i + 1])) for i in range(len(v) - 1) if lo <= v[i] and v[i + 1] <= hi]
    thre = float(np.float32(max(gaps)[1]))
    ch = CR.mask_chain(psm, [3], w, b, thre, 3)
    margin = float(np.abs(s[:2] - thre).min())
    assert margin >= WM.MARGIN and 0.1 < ch["raw"][1].mean() < 0.9, (margin, ch["raw"][1].mean())
    assert float(psm.std()) > 0.5, psm.std()                      # the masks follow the features, not the filter's border response
    model = WM.model_fill(model_mod.CenterPointWhere2comm(model_args(hypes, thre))).eval()
    with torch.no_grad():
        o = model(data())
    assert sorted(o) == sorted(WM.MODEL_KEYS), sorted(o)
    assert np.float32(o["comm_rate"]) == ch["rate"]
    out["m_thre"] = np.float32(thre)
    out["m_mask0"] = ch["masks"][0]
    for key in WM.MODEL_KEYS:
        out["m_" + key] = np.asarray(o[key].numpy(), np.float32)
    print(f"model: thre {thre:.6f} margin {margin:.2e} rate {float(o['comm_rate']):.4f} free agent ones {ch['raw'][1].mean():.3f}")
    keys = {}
    for name, h in (("ms_resnet", configs.lidar_centerpoint_where2comm("ATTEN", True, "resnet")),
                    ("ms_plain", configs.lidar_centerpoint_where2comm("MAX", True, "plain")),
                    ("ss", configs.lidar_centerpoint_where2comm("ATTEN", False, "resnet")),
                    ("no_comm", configs.lidar_centerpoint_where2comm("MAX", False, "plain", communication=False))):
        keys[name] = {k: list(t.shape) for k, t in model_mod.CenterPointWhere2comm(model_args(h)).state_dict().items()}
    with open(os.path.join(OUT, "w2c_comm_state_dict_keys.json"), "w") as fh:
        json.dump(keys, fh, indent=0, sort_keys=True)


def gen_w2c_comm_small():
    comm_mod, attn_mod, model_mod = ref_modules()
    out = {}
    gen_mask_cases(comm_mod, out)
    gen_module_cases(attn_mod, out)
    gen_model_case(model_mod, out)
    save("w2c_comm_small", **out)


if __name__ == "__main__":
    gen_w2c_comm_small()
