"""Generate tests/golden/disconet_small.npz and disconet_state_dict_keys.json by IMPORTING the reference (build container only).

    python -m tests.golden.gen_golden_disconet

DiscoNet fusion (opencood/models/fuse_modules/fusion_in_one.py:153-201).  The reference's DiscoFusion imports PixelWeightLayer
from opencood/models/fuse_modules/disco_fuse.py, a file its tree does not contain: this repository's disco_fuse module (four plain
torch layers, heal_amd/opencood/models/fuse_modules/disco_fuse.py) is registered in sys.modules under that name before the
reference's fusion_in_one is imported.  The warp, the concatenation, the softmax and the weighted sum are then the REFERENCE's own
code; only the four layers are ours.  Weights come from tests/golden/disco_fill.py (detfill + a conv1_4 that does not clamp every
logit); the fixture stores inputs and outputs only, inputs as int8 codes (x = code / 8).
Cases (prefix_):
  n5_ n3_ n1_  one scene of 5 / 3 / 1 agents, C = 128 on an 8 x 8 map;
  b2_          two scenes with record_len [1, 3];
  odd_         a 13 x 11 map (not a multiple of the kernel's 16 x 4 tile; H*W odd);
  c64_         C = 64;
  e2e_         HeterModelBaseline (v2xset/LiDAROnly/lidar_disco.yaml on +-12.8 m: a 32 x 32 fusion map) with 3 agents.
"""
import copy
import glob
import json
import os
import sys

import numpy as np
import torch

from heal_amd import synth
from tests.golden import ref_import as R
from tests.golden.disco_fill import fill_disco
from tests.golden.gen_golden import OUT, _rng, replace_ranges, save, small_lidar_inputs
from tests.golden.gen_golden_cobevt import _plain

YAML_ROOT = "/root/reference/opencood/hypes_yaml"
E2E_YAML = "v2xset/LiDAROnly/lidar_disco.yaml"
HW_M = 51.2
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
X_SCALE = 8.0                 # inputs are stored as int8 codes: x = code / X_SCALE (exact in fp32)
X_STD = 1.5                   # standard deviation of the inputs: at 1.0 only 2-9 % of the logits are clamped by the last ReLU, at 2.0
                              # 30-55 %; 1.5 puts every case at 15-40 %, inside the 5-50 % tests/test_disconet_cpu.py asks for
MAX_CAV = 5

# prefix -> (record_len, channels, (H, W))
CASES = {
    "n5_": ([5], 128, (8, 8)),
    "n3_": ([3], 128, (8, 8)),
    "n1_": ([1], 128, (8, 8)),
    "b2_": ([1, 3], 128, (8, 8)),
    "odd_": ([3], 128, (13, 11)),
    "c64_": ([3], 64, (8, 8)),
}


def ref_fusion_in_one():
    """The reference's fusion_in_one with this repository's PixelWeightLayer standing in for the file the reference lacks."""
    from heal_amd.opencood.models.fuse_modules import disco_fuse
    R.install()
    sys.modules.setdefault("opencood.models.fuse_modules.disco_fuse", disco_fuse)
    return R.ref("opencood.models.fuse_modules.fusion_in_one")


def _case(fio, tu, out, prefix, seed):
    record_len, channels, hw = CASES[prefix]
    rng = _rng(seed)
    n_total = int(sum(record_len))
    code = np.clip(np.round(rng.standard_normal((n_total, channels) + hw) * X_STD * X_SCALE), -127, 127).astype(np.int8)
    x = code.astype(np.float32) / np.float32(X_SCALE)
    pws = []
    for b, n in enumerate(record_len):
        poses = synth.agent_poses(seed + 10 * b, n, r_min=4.0, r_max=12.0)
        pws.append(synth.pairwise_t_matrix(poses, MAX_CAV))
    pw = np.stack(pws)
    aff = tu.normalize_pairwise_tfm(torch.from_numpy(pw.copy()), HW_M, HW_M, 1)
    model = fill_disco(fio.DiscoFusion(channels)).eval()
    with torch.no_grad():
        y = model(torch.from_numpy(x), torch.tensor(record_len), aff)
    out.update({f"{prefix}x_code": code, f"{prefix}pairwise": pw, f"{prefix}record_len": np.array(record_len),
                f"{prefix}out": y.numpy()})


def gen_disconet_small():
    fio = ref_fusion_in_one()
    tu = R.ref("opencood.utils.transformation_utils")
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    out = {"HW_m": np.array([HW_M, HW_M]), "x_scale": np.array(X_SCALE)}
    for k, prefix in enumerate(CASES):
        _case(fio, tu, out, prefix, 61 + k)
    m = R.ref("opencood.models.heter_model_baseline")
    args = copy.deepcopy(yu.load_yaml(os.path.join(YAML_ROOT, E2E_YAML))["model"]["args"])
    replace_ranges(args, E2E_RANGE)
    model = fill_disco(m.HeterModelBaseline(args)).eval()
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
    save("disconet_small", **out)


def disconet_yamls():
    out = []
    for f in sorted(glob.glob(os.path.join(YAML_ROOT, "**", "*.yaml"), recursive=True)):
        with open(f) as fh:
            if "fusion_method: disconet" in fh.read():
                out.append(f)
    return out


def gen_disconet_state_dict_keys():
    """relative yaml path -> {"scope": "model" | "fusion_net", "keys": {key: shape}, "model": the YAML's `model` block}: the
    reference's whole HeterModelBaseline where it can be built here, otherwise its DiscoFusion keyed as `fusion_net.*`."""
    fio = ref_fusion_in_one()
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    tools = R.ref("opencood.tools.train_utils")
    table = {}
    for f in disconet_yamls():
        hy = yu.load_yaml(f)
        rel = os.path.relpath(f, YAML_ROOT)
        try:
            with torch.no_grad():
                model = tools.create_model(hy)
            scope, sd = "model", model.state_dict()
        except Exception:  # noqa: BLE001 - the encoders of some modalities need packages the build container lacks
            scope = "fusion_net"
            sd = {f"fusion_net.{k}": v for k, v in fio.DiscoFusion(hy["model"]["args"]["disconet"]["feat_dim"]).state_dict().items()}
        table[rel] = {"scope": scope, "keys": {k: list(v.shape) for k, v in sd.items()}, "model": _plain(hy["model"])}
        print(f"{rel}: {scope}, {len(sd)} keys")
    if len(table) != 9:
        raise RuntimeError(f"expected the nine disconet YAMLs, found {len(table)}")
    with open(os.path.join(OUT, "disconet_state_dict_keys.json"), "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    gen_disconet_small()
    gen_disconet_state_dict_keys()
