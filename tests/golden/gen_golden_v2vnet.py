"""Generate tests/golden/v2vnet_small.npz and v2vnet_state_dict_keys.json by IMPORTING the reference (build container only).

    python -m tests.golden.gen_golden_v2vnet

V2VNet fusion (opencood/models/fuse_modules/fusion_in_one.py:203-318, sub_modules/convgru.py) on small maps, filled with the
closed-form weights of tests/golden/detfill.py; the fixture stores inputs and outputs only.  Module cases run at in_channels
C_SMALL on 8 x 8 maps (conv_gru.H / W set to the map), affines with rotation and sub-pixel translation (fractional ROI masks).
Cases (prefix_):
  n5_ n3_ n1_  one scene of 5 / 3 / 1 agents (lidar_v2vnet.yaml: avg, gru, 2 iterations, 1 GRU layer);
  b2_          two scenes with record_len [1, 3];
  max_         agg_operator max;
  nogru_       gru_flag false (x_i + agg_i);
  it1_ it3_    num_iteration 1 and 3;
  l2_          a two-layer ConvGRU;
  odd_         a 13 x 11 map (not a multiple of the kernel's 16 x 8 tile; H*W odd);
  e2e_         HeterModelBaseline (lidar_v2vnet.yaml on +-12.8 m: a 16 x 16 fusion map, conv_gru 16 x 16) with 3 agents.
"""
import copy
import glob
import json
import os

import numpy as np
import torch

from heal_amd import synth
from tests.golden import ref_import as R
from tests.golden.detfill import fill_module
from tests.golden.gen_golden import OUT, _rng, load_hypes, replace_ranges, save, small_lidar_inputs
from tests.golden.gen_golden_cobevt import _plain

YAML_ROOT = "/root/reference/opencood/hypes_yaml"
C_SMALL, H, W = 128, 8, 8
HW_M = 51.2
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
X_SCALE = 8.0                 # inputs are stored as int8 codes: x = code / X_SCALE (exact in fp32)
MAX_CAV = 5

# prefix -> (record_len, overrides of the v2vnet block, (H, W))
CASES = {
    "n5_": ([5], {}, (H, W)),
    "n3_": ([3], {}, (H, W)),
    "n1_": ([1], {}, (H, W)),
    "b2_": ([1, 3], {}, (H, W)),
    "max_": ([3], {"agg_operator": "max"}, (H, W)),
    "nogru_": ([3], {"gru_flag": False}, (H, W)),
    "it1_": ([3], {"num_iteration": 1}, (H, W)),
    "it3_": ([3], {"num_iteration": 3}, (H, W)),
    "l2_": ([3], {"layers": 2}, (H, W)),
    "odd_": ([3], {}, (13, 11)),
}


def v2vnet_args(overrides, hw, channels=C_SMALL):
    """lidar_v2vnet.yaml's v2vnet block with in_channels, conv_gru.H / W and the case's overrides."""
    args = copy.deepcopy(load_hypes("LiDAROnly/lidar_v2vnet.yaml")["model"]["args"]["v2vnet"])
    args["in_channels"] = channels
    args["conv_gru"]["H"], args["conv_gru"]["W"] = hw
    for k, v in overrides.items():
        if k == "layers":     # kernel_size is a list with one entry per layer (convgru.py:101-106)
            args["conv_gru"]["num_layers"] = v
            args["conv_gru"]["kernel_size"] = [[3, 3]] * v
        else:
            args[k] = v
    return args


def _case(fio, tu, out, prefix, seed):
    record_len, over, hw = CASES[prefix]
    rng = _rng(seed)
    n_total = int(sum(record_len))
    code = np.clip(np.round(rng.standard_normal((n_total, C_SMALL) + hw) * X_SCALE), -127, 127).astype(np.int8)
    x = code.astype(np.float32) / np.float32(X_SCALE)
    pws = []
    for b, n in enumerate(record_len):
        poses = synth.agent_poses(seed + 10 * b, n, r_min=4.0, r_max=12.0)
        pws.append(synth.pairwise_t_matrix(poses, MAX_CAV))
    pw = np.stack(pws)
    aff = tu.normalize_pairwise_tfm(torch.from_numpy(pw.copy()), HW_M, HW_M, 1)
    model = fill_module(fio.V2VNetFusion(v2vnet_args(over, hw))).eval()
    with torch.no_grad():
        y = model(torch.from_numpy(x), torch.tensor(record_len), aff)
    out.update({f"{prefix}x_code": code, f"{prefix}pairwise": pw, f"{prefix}record_len": np.array(record_len),
                f"{prefix}out": y.numpy()})


def gen_v2vnet_small():
    fio = R.ref("opencood.models.fuse_modules.fusion_in_one")
    tu = R.ref("opencood.utils.transformation_utils")
    out = {"HW_m": np.array([HW_M, HW_M]), "x_scale": np.array(X_SCALE)}
    for k, prefix in enumerate(CASES):
        _case(fio, tu, out, prefix, 41 + k)
    m = R.ref("opencood.models.heter_model_baseline")
    args = copy.deepcopy(load_hypes("LiDAROnly/lidar_v2vnet.yaml")["model"]["args"])
    replace_ranges(args, E2E_RANGE)
    args["v2vnet"]["conv_gru"]["H"] = args["v2vnet"]["conv_gru"]["W"] = 16
    model = fill_module(m.HeterModelBaseline(args)).eval()
    n = 3
    vf, vc, vn = small_lidar_inputs([91, 92, 93], lidar_range=E2E_RANGE, n_points=1000)
    poses = synth.agent_poses(95, n, r_min=3.0, r_max=8.0)
    pw = synth.pairwise_t_matrix(poses, 5)[None]
    data = {"inputs_m1": {"voxel_features": torch.from_numpy(vf), "voxel_coords": torch.from_numpy(vc),
                          "voxel_num_points": torch.from_numpy(vn)},
            "agent_modality_list": ["m1"] * n, "record_len": torch.tensor([n]),
            "pairwise_t_matrix": torch.from_numpy(pw.copy())}
    with torch.no_grad():
        o = model(data)
    out.update({"e2e_voxel_features": vf, "e2e_voxel_coords": vc, "e2e_voxel_num_points": vn, "e2e_pairwise": pw,
                "e2e_cls": o["cls_preds"].numpy(), "e2e_reg": o["reg_preds"].numpy(), "e2e_dir": o["dir_preds"].numpy()})
    save("v2vnet_small", **out)


def v2vnet_yamls():
    out = []
    for f in sorted(glob.glob(os.path.join(YAML_ROOT, "**", "*.yaml"), recursive=True)):
        with open(f) as fh:
            if "fusion_method: v2vnet" in fh.read():
                out.append(f)
    return out


def gen_v2vnet_state_dict_keys():
    """relative yaml path -> {"scope": "model" | "fusion_net", "keys": {key: shape}, "model": the YAML's `model` block}: the
    reference's whole HeterModelBaseline where it can be built here, otherwise its V2VNetFusion keyed as `fusion_net.*`."""
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    tools = R.ref("opencood.tools.train_utils")
    fio = R.ref("opencood.models.fuse_modules.fusion_in_one")
    table = {}
    for f in v2vnet_yamls():
        hy = yu.load_yaml(f)
        rel = os.path.relpath(f, YAML_ROOT)
        try:
            with torch.no_grad():
                model = tools.create_model(hy)
            scope, sd = "model", model.state_dict()
        except Exception:  # noqa: BLE001 - the encoders of some modalities need packages the build container lacks
            scope = "fusion_net"
            sd = {f"fusion_net.{k}": v for k, v in fio.V2VNetFusion(hy["model"]["args"]["v2vnet"]).state_dict().items()}
        table[rel] = {"scope": scope, "keys": {k: list(v.shape) for k, v in sd.items()}, "model": _plain(hy["model"])}
        print(f"{rel}: {scope}, {len(sd)} keys")
    if len(table) != 3:
        raise RuntimeError(f"expected the three v2vnet YAMLs, found {len(table)}")
    with open(os.path.join(OUT, "v2vnet_state_dict_keys.json"), "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    gen_v2vnet_small()
    gen_v2vnet_state_dict_keys()
