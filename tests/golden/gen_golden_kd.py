"""Generate tests/golden/kd_small.npz and kd_state_dict_keys.json by IMPORTING the reference (build container only).

    python -m tests.golden.gen_golden_kd

DiscoNet's distillation (opv2v/LiDAROnly/lidar_disco.yaml): the loss point_pillar_disconet_loss, the student
point_pillar_disconet and the teacher point_pillar_disconet_teacher.  Inputs and outputs only.

Loss cases (prefix_): the REFERENCE's PointPillarDiscoNetLoss.forward on the CPU with the YAML's loss block (kd weight 10000).
Features are int8 codes: student = s_code / s_scale, teacher = t_code / t_scale.  Stored per case: the head maps and targets,
`total_loss`, `kd_loss` and the autograd gradient of the total with respect to `feature`.
  c256_  (2, 256, 8, 8)     the YAML's channel count
  c64_   (1, 64, 13, 11)    an odd map: H*W = 143 is no multiple of the kernel's 64-pixel tile
  c7_    (2, 7, 5, 3)       a channel count off the register-resident path, fewer pixels than a tile
  c2_    (1, 2, 1, 1)       one pixel, two channels (fewer channels than waves)
  gap_   (2, 64, 5, 7)      teacher codes at scale 1: at every third pixel one channel is 127 and the others are below 0, a
                            logit gap of more than 110, so most teacher probabilities underflow to 0 in fp32

Model goldens (m_): the reference's own student and teacher CAN be imported with the stubs of ref_import, given two stand-ins
that carry no arithmetic of theirs: `opencood.data_utils.post_processor.UncertaintyVoxelPostprocessor` (imported by the student's
file, never used) is set to None, and PixelWeightLayer, which the reference's tree lacks, is this repository's (as in
gen_golden_disconet.py).  So the fixture holds real outputs: 3 agents on a +-12.8 m range (a 32 x 32 map), the student's heads
and every 16th channel of its `feature`, the teacher's heads and every 16th channel of `teacher_feature` on the stacked
ego-frame cloud (heal_amd.synth.teacher_processed_lidar).  kd_state_dict_keys.json pins both models' state_dict names and
shapes for the YAML's own arguments.
"""
import copy
import importlib
import json
import os
import sys

import numpy as np
import torch

from heal_amd import synth
from oracle import cref
from tests.golden import ref_import as R
from tests.golden.detfill import fill_module
from tests.golden.disco_fill import fill_disco
from tests.golden.gen_golden import OUT, SEED_SHIFT, YAML_DIR, _rng, replace_ranges, save

YAML = "LiDAROnly/lidar_disco.yaml"
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
X_STD = 1.5
FEATURE_STRIDE = 16           # channels of the 256-channel maps kept in the fixture

# prefix -> ((N, C, H, W), student scale, teacher scale)
LOSS_CASES = {
    "c256_": ((2, 256, 8, 8), 8.0, 8.0),
    "c64_": ((1, 64, 13, 11), 8.0, 8.0),
    "c7_": ((2, 7, 5, 3), 8.0, 8.0),
    "c2_": ((1, 2, 1, 1), 8.0, 8.0),
    "gap_": ((2, 64, 5, 7), 8.0, 1.0),
}


def _codes(rng, shape, scale):
    return np.clip(np.round(rng.standard_normal(shape) * X_STD * scale), -127, 127).astype(np.int8)


def loss_case_inputs(prefix, seed):
    """The stored inputs of one loss case (numpy)."""
    (N, C, H, W), ss, ts = LOSS_CASES[prefix]
    rng = _rng(seed)
    s_code = _codes(rng, (N, C, H, W), ss)
    if prefix == "gap_":
        t_code = np.clip(np.round(rng.standard_normal((N, C, H, W)) * 20.0 - 40.0), -127, -1).astype(np.int8)
        flat = t_code.reshape(N, C, H * W)
        for p in range(0, H * W, 3):
            flat[:, (5 * p) % C, p] = 127
    else:
        t_code = _codes(rng, (N, C, H, W), ts)
    pos = (rng.random((N, H, W, 2)) > 0.9).astype(np.float32)
    neg = (rng.random((N, H, W, 2)) > 0.2).astype(np.float32) * (1 - pos)
    return {"s_code": s_code, "t_code": t_code, "s_scale": np.array(ss), "t_scale": np.array(ts),
            "cls": rng.standard_normal((N, 2, H, W)).astype(np.float32),
            "reg": (rng.standard_normal((N, 14, H, W)) * 0.3).astype(np.float32),
            "dir": rng.standard_normal((N, 4, H, W)).astype(np.float32),
            "pos": pos, "neg": neg, "tgt": (rng.standard_normal((N, H, W, 14)) * 0.4).astype(np.float32)}


def gen_loss_cases(out):
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    tu = R.ref("opencood.tools.train_utils")
    hy = yu.load_yaml(os.path.join(YAML_DIR, YAML))
    crit = tu.create_loss(hy)
    assert type(crit).__name__ == "PointPillarDiscoNetLoss"
    for k, prefix in enumerate(LOSS_CASES):
        d = loss_case_inputs(prefix, 300 + k)
        feature = torch.from_numpy(d["s_code"].astype(np.float32) / np.float32(d["s_scale"])).requires_grad_(True)
        teacher = torch.from_numpy(d["t_code"].astype(np.float32) / np.float32(d["t_scale"]))
        o = {"cls_preds": torch.from_numpy(d["cls"]), "reg_preds": torch.from_numpy(d["reg"]),
             "dir_preds": torch.from_numpy(d["dir"]), "feature": feature, "teacher_feature": teacher,
             "teacher_cls_preds": torch.from_numpy(d["cls"]), "teacher_reg_preds": torch.from_numpy(d["reg"])}
        t = {"pos_equal_one": torch.from_numpy(d["pos"]), "neg_equal_one": torch.from_numpy(d["neg"]),
             "targets": torch.from_numpy(d["tgt"])}
        total = crit(o, t)
        total.backward()
        if prefix == "gap_":
            p_t = torch.softmax(teacher.permute(0, 2, 3, 1).reshape(-1, teacher.shape[1]), dim=1)
            assert float((p_t == 0).float().mean()) > 0.2, "the gap case must underflow teacher probabilities"
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(feature.grad).all())
        out.update({f"{prefix}{name}": v for name, v in d.items()})
        out.update({f"{prefix}total_loss": np.float32(crit.loss_dict["total_loss"]),
                    f"{prefix}kd_loss": np.float32(crit.loss_dict["kd_loss"]), f"{prefix}grad": feature.grad.numpy()})
        print(f"{prefix}: total {crit.loss_dict['total_loss']:.6f} kd {crit.loss_dict['kd_loss']:.6f}")


def ref_models():
    """(student module, teacher module) of the reference, importable with the two stand-ins named in the module docstring."""
    from heal_amd.opencood.models.fuse_modules import disco_fuse
    R.install()         # (R.ref would install again and drop the attribute set below: import directly)
    sys.modules["opencood.data_utils.post_processor"].UncertaintyVoxelPostprocessor = None
    sys.modules.setdefault("opencood.models.fuse_modules.disco_fuse", disco_fuse)
    return (importlib.import_module("opencood.models.point_pillar_disconet"),
            importlib.import_module("opencood.models.point_pillar_disconet_teacher"))


def model_inputs(seeds=(191, 192, 193), pose_seed=195, n_points=1000):
    """Three agents' clouds near the ego, their poses, the per-agent voxels and the teacher's stacked voxels."""
    n = len(seeds)
    poses = synth.agent_poses(pose_seed + SEED_SHIFT, n, r_min=3.0, r_max=8.0)
    clouds = []
    for seed in seeds:
        pts = synth.lidar_frame(seed + SEED_SHIFT)
        near = (np.abs(pts[:, 0]) < M_RANGE[3] + 2) & (np.abs(pts[:, 1]) < M_RANGE[4] + 2)
        clouds.append(pts[near][:n_points])
    vox = lambda pts, b: cref.voxelize(pts, M_RANGE, (0.4, 0.4, 4), 32, 70000, batch_idx=b)     # noqa: E731
    parts = [vox(c, b) for b, c in enumerate(clouds)]
    student = {"voxel_features": np.concatenate([p[0] for p in parts]), "voxel_coords": np.concatenate([p[1] for p in parts]),
               "voxel_num_points": np.concatenate([p[2] for p in parts])}
    teacher = synth.teacher_processed_lidar([(clouds, poses)], M_RANGE, vox)
    return student, teacher, synth.pairwise_t_matrix(poses, 5)[None]


def _model_args(yu):
    hy = yu.load_yaml(os.path.join(YAML_DIR, YAML))
    args = copy.deepcopy(hy["model"]["args"])
    replace_ranges(args, M_RANGE)
    args["point_pillar_scatter"]["grid_size"] = np.round(
        (np.array(M_RANGE[3:]) - np.array(M_RANGE[:3])) / np.array(args["voxel_size"])).astype(np.int64)
    return hy, args


def gen_model_goldens(out):
    student_mod, teacher_mod = ref_models()
    yu = R.ref("opencood.hypes_yaml.yaml_utils")
    hy, args = _model_args(yu)
    student = fill_disco(student_mod.PointPillarDiscoNet(copy.deepcopy(args))).eval()
    teacher = fill_module(teacher_mod.PointPillarDiscoNetTeacher(copy.deepcopy(args))).eval()
    s_in, t_in, pw = model_inputs()
    tt = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}      # noqa: E731
    data = {"processed_lidar": tt(s_in), "teacher_processed_lidar": tt(t_in), "record_len": torch.tensor([3]),
            "lidar_pose": torch.zeros((3, 6)), "pairwise_t_matrix": torch.from_numpy(pw.copy())}
    with torch.no_grad():
        so, to = student(data), teacher(data)
    assert sorted(to) == ["dir_preds", "teacher_cls_preds", "teacher_feature", "teacher_reg_preds"]
    out.update({f"m_s_{k}": v for k, v in s_in.items()})
    out.update({f"m_t_{k}": v for k, v in t_in.items()})
    out.update({"m_pairwise": pw, "m_cls": so["cls_preds"].numpy(), "m_reg": so["reg_preds"].numpy(),
                "m_dir": so["dir_preds"].numpy(), "m_feature": so["feature"][:, ::FEATURE_STRIDE].numpy(),
                "m_teacher_cls": to["teacher_cls_preds"].numpy(), "m_teacher_reg": to["teacher_reg_preds"].numpy(),
                "m_teacher_dir": to["dir_preds"].numpy(),
                "m_teacher_feature": to["teacher_feature"][:, ::FEATURE_STRIDE].numpy()})
    # state_dict names and shapes for the YAML's own arguments (full range)
    full = hy["model"]["args"]
    keys = {"point_pillar_disconet": {k: list(v.shape) for k, v in
                                      student_mod.PointPillarDiscoNet(copy.deepcopy(full)).state_dict().items()},
            "point_pillar_disconet_teacher": {k: list(v.shape) for k, v in teacher_mod.PointPillarDiscoNetTeacher(
                copy.deepcopy(hy["kd_flag"]["teacher_model_config"])).state_dict().items()}}
    with open(os.path.join(OUT, "kd_state_dict_keys.json"), "w") as fh:
        json.dump(keys, fh, indent=0, sort_keys=True)


def gen_kd_small():
    out = {"feature_stride": np.array(FEATURE_STRIDE)}
    gen_loss_cases(out)
    gen_model_goldens(out)
    save("kd_small", **out)


if __name__ == "__main__":
    gen_kd_small()
