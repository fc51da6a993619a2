"""Generate tests/golden/where2comm_small.npz, who2com_small.npz and where2comm_state_dict_keys.json by IMPORTING the reference
(build container only).

    python -m tests.golden.gen_golden_where2comm

Where2commFusion and Who2comFusion (opencood/models/fuse_modules/fusion_in_one.py:431-539).  The reference's where2comm_attn.py
starts with `from turtle import update` (an editor's stray import, which needs tkinter): an empty `turtle` module is
registered in sys.modules before the import.  Everything that computes is the REFERENCE's own code.  Weights come from
tests/golden/w2c_fill.py; the fixtures store inputs and outputs only, inputs as int8 codes (x = code / 8).
Cases (prefix_) of where2comm_small.npz:
  n5_ n3_ n1_  one scene of 5 / 3 / 1 agents, C = 128 on an 8 x 8 map (64 pixels: the smallest map heal_conv1x1 takes);
  b2_          two scenes with record_len [1, 3];
  odd_         a 13 x 11 map (H*W odd: the torch path on the device);
  c64_         C = 64;
  far_         3 agents 36 .. 44 m from the ego on a 51.2 m map: their footprints leave part of the ego map uncovered;
  e2e_         HeterModelBaseline (v2xset/LiDAROnly/lidar_attfuse.yaml on +-12.8 m with fusion_method: where2comm and where2comm: 256
               substituted) with 3 agents.
who2com_small.npz: n3_ n1_ b2_ odd_ and e2e_ likewise (inputs of std 0.4, so that AttFusion's softmax is not one-hot on the ego)."""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

from heal_amd import synth
from tests.golden import ref_import as R
from tests.golden.gen_golden import OUT, _rng, replace_ranges, save, small_lidar_inputs
from tests.golden.w2c_fill import fill_w2c

YAML_ROOT = "/root/reference/opencood/hypes_yaml"
E2E_YAML = "v2xset/LiDAROnly/lidar_attfuse.yaml"
HW_M = 51.2
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
X_SCALE = 8.0                 # inputs are stored as int8 codes: x = code / X_SCALE (exact in fp32)
MAX_CAV = 5

# prefix -> (record_len, channels, (H, W), (r_min, r_max) of the neighbours' distance from the ego in metres)
W2C_CASES = {
    "n5_": ([5], 128, (8, 8), (4.0, 12.0)),
    "n3_": ([3], 128, (8, 8), (4.0, 12.0)),
    "n1_": ([1], 128, (8, 8), (4.0, 12.0)),
    "b2_": ([1, 3], 128, (8, 8), (4.0, 12.0)),
    "odd_": ([3], 128, (13, 11), (4.0, 12.0)),
    "c64_": ([3], 64, (8, 8), (4.0, 12.0)),
    "far_": ([3], 128, (8, 8), (36.0, 44.0)),
}
WHO_CASES = {k: W2C_CASES[k] for k in ("n3_", "n1_", "b2_", "odd_")}
X_STD = {"where2comm": 1.5, "who2com": 0.4}


def ref_fusion_in_one():
    R.install()
    sys.modules.setdefault("turtle", types.ModuleType("turtle"))
    sys.modules["turtle"].__dict__.setdefault("update", None)
    return R.ref("opencood.models.fuse_modules.fusion_in_one")


def _case(cls, method, cases, tu, out, prefix, seed):
    record_len, channels, hw, (r_min, r_max) = cases[prefix]
    rng = _rng(seed)
    n_total = int(sum(record_len))
    code = np.clip(np.round(rng.standard_normal((n_total, channels) + hw) * X_STD[method] * X_SCALE), -127, 127).astype(np.int8)
    x = code.astype(np.float32) / np.float32(X_SCALE)
    pws = []
    for b, n in enumerate(record_len):
        poses = synth.agent_poses(seed + 10 * b, n, r_min=r_min, r_max=r_max)
        pws.append(synth.pairwise_t_matrix(poses, MAX_CAV))
    pw = np.stack(pws)
    aff = tu.normalize_pairwise_tfm(torch.from_numpy(pw.copy()), HW_M, HW_M, 1)
    model = fill_w2c(cls(channels)).eval()
    with torch.no_grad():
        y = model(torch.from_numpy(x), torch.tensor(record_len), aff)
    out.update({f"{prefix}x_code": code, f"{prefix}pairwise": pw, f"{prefix}record_len": np.array(record_len),
                f"{prefix}out": y.numpy()})


def _e2e(method, yu, out):
    m = R.ref("opencood.models.heter_model_baseline")
    args = copy.deepcopy(yu.load_yaml(os.path.join(YAML_ROOT, E2E_YAML))["model"]["args"])
    replace_ranges(args, E2E_RANGE)
    args["fusion_method"] = method
    args[method] = 256
    model = fill_w2c(m.HeterModelBaseline(args)).eval()
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


def gen_small():
    fio = ref_fusion_in_one()
    tu = R.ref("opencood.utils.transformation_utils")
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    for method, cls, cases, name, seed0 in (("where2comm", fio.Where2commFusion, W2C_CASES, "where2comm_small", 161),
                                           ("who2com", fio.Who2comFusion, WHO_CASES, "who2com_small", 181)):
        out = {"HW_m": np.array([HW_M, HW_M]), "x_scale": np.array(X_SCALE)}
        for k, prefix in enumerate(cases):
            _case(cls, method, cases, tu, out, prefix, seed0 + k)
        _e2e(method, yu, out)
        save(name, **out)


def gen_state_dict_keys():
    """{"where2comm" | "who2com": {key: shape}}: the reference's two modules at 256 channels, keyed as `fusion_net.*`."""
    fio = ref_fusion_in_one()
    table = {}
    for method, cls in (("where2comm", fio.Where2commFusion), ("who2com", fio.Who2comFusion)):
        table[method] = {f"fusion_net.{k}": list(v.shape) for k, v in cls(256).state_dict().items()}
        print(f"{method}: {len(table[method])} keys")
    with open(os.path.join(OUT, "where2comm_state_dict_keys.json"), "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    gen_small()
    gen_state_dict_keys()
