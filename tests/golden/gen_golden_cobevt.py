"""Generate tests/golden/cobevt_small.npz and cobevt_state_dict_keys.json by IMPORTING the reference (build container only).

    python -m tests.golden.gen_golden_cobevt

CoBEVT fusion (opencood/models/fuse_modules/fusion_in_one.py:374-430, swap_fusion_modules.py) on small maps, filled with the
closed-form weights of tests/golden/detfill.py; the fixture stores inputs and outputs only.  Cases (prefix_):
  l5n5_  agent_size 5, one scene of 5 agents;
  l5n3_  agent_size 5, one scene of 3 agents (key mask + the padded agents in the mlp_head mean);
  l2n1_  agent_size 2 (DAIR-V2X), one scene of 1 agent;
  b2_    agent_size 5, two scenes with record_len [1, 3];
  e2e_   HeterModelBaseline (lidar_cobevt.yaml on +-12.8 m) with 2 agents: cls / reg / dir.
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

YAML_ROOT = "/root/reference/opencood/hypes_yaml"
C, H, W = 256, 8, 8          # 8 x 8: the smallest map whose window and dilated-grid groupings differ (2 x 2 groups of 4 x 4)
HW_M = 51.2
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
X_SCALE = 8.0                 # inputs are stored as int8 codes: x = code / X_SCALE (exact in fp32)


def cobevt_args(agent_size):
    args = copy.deepcopy(load_hypes("LiDAROnly/lidar_cobevt.yaml")["model"]["args"]["cobevt"])
    args["agent_size"] = agent_size
    return args


def _case(fio, tu, out, prefix, agent_size, record_len, seed):
    rng = _rng(seed)
    n_total = int(sum(record_len))
    code = np.clip(np.round(rng.standard_normal((n_total, C, H, W)) * X_SCALE), -127, 127).astype(np.int8)
    x = code.astype(np.float32) / np.float32(X_SCALE)
    pws = []
    for b, n in enumerate(record_len):
        poses = synth.agent_poses(seed + 10 * b, n, r_min=4.0, r_max=12.0)
        pws.append(synth.pairwise_t_matrix(poses, agent_size))
    pw = np.stack(pws)
    aff = tu.normalize_pairwise_tfm(torch.from_numpy(pw.copy()), HW_M, HW_M, 1)
    model = fill_module(fio.CoBEVT(cobevt_args(agent_size))).eval()
    with torch.no_grad():
        y = model(torch.from_numpy(x), torch.tensor(record_len), aff)
    out.update({f"{prefix}x_code": code, f"{prefix}pairwise": pw, f"{prefix}record_len": np.array(record_len),
                f"{prefix}agent_size": np.array(agent_size), f"{prefix}out": y.numpy()})


def gen_cobevt_small():
    fio = R.ref("opencood.models.fuse_modules.fusion_in_one")
    tu = R.ref("opencood.utils.transformation_utils")
    out = {"HW_m": np.array([HW_M, HW_M]), "x_scale": np.array(X_SCALE)}
    _case(fio, tu, out, "l5n5_", 5, [5], 31)
    _case(fio, tu, out, "l5n3_", 5, [3], 32)
    _case(fio, tu, out, "l2n1_", 2, [1], 33)
    _case(fio, tu, out, "b2_", 5, [1, 3], 34)
    # end to end: HeterModelBaseline with fusion_method cobevt on a +-12.8 m range (a 16 x 16 fusion map)
    m = R.ref("opencood.models.heter_model_baseline")
    args = copy.deepcopy(load_hypes("LiDAROnly/lidar_cobevt.yaml")["model"]["args"])
    replace_ranges(args, E2E_RANGE)
    model = fill_module(m.HeterModelBaseline(args)).eval()
    n = 2
    vf, vc, vn = small_lidar_inputs([81, 82], lidar_range=E2E_RANGE, n_points=1000)
    poses = synth.agent_poses(90, n, r_min=3.0, r_max=8.0)
    pw = synth.pairwise_t_matrix(poses, 5)[None]
    data = {"inputs_m1": {"voxel_features": torch.from_numpy(vf), "voxel_coords": torch.from_numpy(vc),
                          "voxel_num_points": torch.from_numpy(vn)},
            "agent_modality_list": ["m1"] * n, "record_len": torch.tensor([n]),
            "pairwise_t_matrix": torch.from_numpy(pw.copy())}
    with torch.no_grad():
        o = model(data)
    out.update({"e2e_voxel_features": vf, "e2e_voxel_coords": vc, "e2e_voxel_num_points": vn, "e2e_pairwise": pw,
                "e2e_cls": o["cls_preds"].numpy(), "e2e_reg": o["reg_preds"].numpy(), "e2e_dir": o["dir_preds"].numpy()})
    save("cobevt_small", **out)


def _plain(o):
    if isinstance(o, dict):
        return {str(k): _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    if isinstance(o, np.ndarray):
        return _plain(o.tolist())
    if isinstance(o, np.generic):
        return o.item()
    return o


def cobevt_yamls():
    out = []
    for f in sorted(glob.glob(os.path.join(YAML_ROOT, "**", "*.yaml"), recursive=True)):
        with open(f) as fh:
            if "fusion_method: cobevt" in fh.read():
                out.append(f)
    return out


def gen_cobevt_state_dict_keys():
    """relative yaml path -> {"scope": "model" | "fusion_net", "keys": {key: shape}, "model": the YAML's `model` block as the
    reference's loader returns it (the tests build the mirror from it: the YAMLs do not travel)}: the reference's whole HeterModelBaseline
    where it can be built here (its third-party encoders stubbed or absent make the camera / SECOND models fail), otherwise the
    reference's CoBEVT built from the YAML's `cobevt` block, keyed as `fusion_net.*`."""
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    tools = R.ref("opencood.tools.train_utils")
    fio = R.ref("opencood.models.fuse_modules.fusion_in_one")
    table = {}
    for f in cobevt_yamls():
        hy = yu.load_yaml(f)
        rel = os.path.relpath(f, YAML_ROOT)
        try:
            with torch.no_grad():
                model = tools.create_model(hy)
            scope, sd = "model", model.state_dict()
        except Exception:  # noqa: BLE001 - the encoders of some modalities need packages the build container lacks
            scope = "fusion_net"
            sd = {f"fusion_net.{k}": v for k, v in fio.CoBEVT(hy["model"]["args"]["cobevt"]).state_dict().items()}
        table[rel] = {"scope": scope, "keys": {k: list(v.shape) for k, v in sd.items()}, "model": _plain(hy["model"])}
        print(f"{rel}: {scope}, {len(sd)} keys")
    if len(table) != 10:
        raise RuntimeError(f"expected the ten cobevt YAMLs, found {len(table)}")
    with open(os.path.join(OUT, "cobevt_state_dict_keys.json"), "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)


if __name__ == "__main__":
    gen_cobevt_small()
    gen_cobevt_state_dict_keys()
