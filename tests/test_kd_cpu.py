"""DiscoNet distillation on the CPU (opv2v/LiDAROnly/lidar_disco.yaml): the student, the teacher and the loss construct by name;
their parameter layout equals the reference's (tests/golden/kd_state_dict_keys.json); the loss -- value, KD term and gradient --
and both models equal the reference's outputs (tests/golden/kd_small.npz, written by tests/golden/gen_golden_kd.py); the C ABI
declares and exports the fused KD kernel's entry points.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, configs
from tests.golden.detfill import fill_module
from tests.golden.disco_fill import fill_disco

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_YAML = "/root/reference/opencood/hypes_yaml/opv2v/LiDAROnly/lidar_disco.yaml"
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]          # the model case of kd_small.npz (a 32 x 32 map)
LOSS_CASES = {"c256_": (2, 256, 8, 8), "c64_": (1, 64, 13, 11), "c7_": (2, 7, 5, 3), "c2_": (1, 2, 1, 1), "gap_": (2, 64, 5, 7)}
TOL = 1e-3                                           # the project's tolerance against model goldens
NEW_SYMBOLS = ("heal_kd_kl_loss", "heal_kd_kl_loss_workspace")


def rel_err(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "kd_small.npz"))


def loss_case(g, prefix, device="cpu"):
    """(output_dict, target_dict) of a loss case; `feature` is a leaf that requires gradient."""
    f32 = lambda k: torch.from_numpy(g[f"{prefix}{k}"]).to(device)      # noqa: E731
    feature = torch.from_numpy(g[f"{prefix}s_code"].astype(np.float32) / np.float32(g[f"{prefix}s_scale"])).to(device)
    teacher = torch.from_numpy(g[f"{prefix}t_code"].astype(np.float32) / np.float32(g[f"{prefix}t_scale"])).to(device)
    out = {"cls_preds": f32("cls"), "reg_preds": f32("reg"), "dir_preds": f32("dir"), "feature": feature.requires_grad_(True),
           "teacher_feature": teacher, "teacher_cls_preds": f32("cls"), "teacher_reg_preds": f32("reg")}
    return out, {"pos_equal_one": f32("pos"), "neg_equal_one": f32("neg"), "targets": f32("tgt")}


def m_data(g, device="cpu"):
    def lidar(tag):
        return {"voxel_features": torch.from_numpy(g[f"m_{tag}_voxel_features"]).to(device),
                "voxel_coords": torch.from_numpy(g[f"m_{tag}_voxel_coords"]).to(torch.int32).to(device),
                "voxel_num_points": torch.from_numpy(g[f"m_{tag}_voxel_num_points"]).to(torch.int32).to(device)}
    return {"processed_lidar": lidar("s"), "teacher_processed_lidar": lidar("t"), "record_len": torch.tensor([3]),
            "pairwise_t_matrix": torch.from_numpy(g["m_pairwise"]).to(device)}


def m_models(device="cpu"):
    """(student, teacher) on the small range with the fixture's weights, eval mode, parameters trainable."""
    from heal_amd.opencood.tools.train_utils import create_model
    hy = configs.lidar_disco_kd(M_RANGE)
    student = fill_disco(create_model(hy)).to(device).eval()
    teacher = fill_module(create_model({"model": {"core_method": hy["kd_flag"]["teacher_model"],
                                                  "args": hy["kd_flag"]["teacher_model_config"]}})).to(device).eval()
    return student, teacher


def check_student(g, out):
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].detach().cpu().numpy(), g[f"m_{name}"])
        assert e <= TOL, (key, e)
    e = rel_err(out["feature"][:, ::int(g["feature_stride"])].detach().cpu().numpy(), g["m_feature"])
    assert e <= TOL, ("feature", e)


def check_teacher(g, out):
    assert sorted(out) == ["dir_preds", "teacher_cls_preds", "teacher_feature", "teacher_reg_preds"]
    for key, name in (("teacher_cls_preds", "teacher_cls"), ("teacher_reg_preds", "teacher_reg"), ("dir_preds", "teacher_dir")):
        e = rel_err(out[key].detach().cpu().numpy(), g[f"m_{name}"])
        assert e <= TOL, (key, e)
    e = rel_err(out["teacher_feature"][:, ::int(g["feature_stride"])].detach().cpu().numpy(), g["m_teacher_feature"])
    assert e <= TOL, ("teacher_feature", e)


def _build_all(hy):
    from heal_amd.opencood.loss.point_pillar_disconet_loss import PointPillarDiscoNetLoss
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import DiscoFusion
    from heal_amd.opencood.models.point_pillar_disconet import PointPillarDiscoNet
    from heal_amd.opencood.models.point_pillar_disconet_teacher import PointPillarDiscoNetTeacher
    from heal_amd.opencood.tools import train_utils as tu
    model, teacher, crit = tu.create_model(hy), tu.create_teacher(hy), tu.create_loss(hy)
    assert type(model) is PointPillarDiscoNet and isinstance(model.fusion_net, DiscoFusion)
    assert type(teacher) is PointPillarDiscoNetTeacher and not hasattr(teacher, "fusion_net")
    assert type(crit) is PointPillarDiscoNetLoss and crit.kd["weight"] == 10000
    return model, teacher, crit


def _keys():
    with open(os.path.join(GOLD, "kd_state_dict_keys.json")) as fh:
        return json.load(fh)


def test_config_builds_student_teacher_and_loss_with_the_reference_layout():
    hy = configs.lidar_disco_kd()
    assert hy["model"]["core_method"] == "point_pillar_disconet"
    assert hy["kd_flag"]["teacher_model"] == "point_pillar_disconet_teacher"
    assert hy["loss"]["core_method"] == "point_pillar_disconet_loss"
    model, teacher, _ = _build_all(hy)
    keys = _keys()
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == keys["point_pillar_disconet"]
    assert {k: list(v.shape) for k, v in teacher.state_dict().items()} == keys["point_pillar_disconet_teacher"]
    assert keys["point_pillar_disconet"]["fusion_net.pixel_weight_layer.conv1_1.weight"] == [128, 512, 1, 1]
    assert not any(k.startswith("fusion_net.") for k in keys["point_pillar_disconet_teacher"])


@pytest.mark.skipif(not os.path.isfile(REF_YAML), reason="reference tree not present")
def test_reference_yaml_builds_student_teacher_and_loss():
    from heal_amd.opencood.hypes_yaml.yaml_utils import load_yaml
    hy = load_yaml(REF_YAML)
    model, teacher, _ = _build_all(hy)        # the YAML's teacher_path does not exist here: initial weights
    keys = _keys()
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == keys["point_pillar_disconet"]
    assert {k: list(v.shape) for k, v in teacher.state_dict().items()} == keys["point_pillar_disconet_teacher"]
    mine = configs.lidar_disco_kd()
    assert mine["loss"] == hy["loss"] and mine["optimizer"] == hy["optimizer"] and mine["lr_scheduler"] == hy["lr_scheduler"]
    for k, v in hy["model"]["args"].items():
        if k != "point_pillar_scatter":
            assert mine["model"]["args"][k] == v, k
    assert hy["kd_flag"]["teacher_model_config"] is hy["model"]["args"]              # the YAML's alias
    assert mine["kd_flag"]["teacher_model_config"] is mine["model"]["args"]


def test_create_teacher_is_frozen_in_eval_mode_and_loads_a_checkpoint(tmp_path):
    from heal_amd.opencood.tools import train_utils as tu
    hy = configs.lidar_disco_kd(M_RANGE)
    src = fill_module(tu.create_teacher(hy))
    path = str(tmp_path / "net_epoch_bestval_at25.pth")
    state = {k: v.clone() for k, v in src.state_dict().items()}
    state["not_in_the_teacher.weight"] = torch.zeros(3)        # strict=False: an early-fusion checkpoint may carry more
    torch.save(state, path)
    hy["kd_flag"]["teacher_path"] = path
    teacher = tu.create_teacher(hy)
    assert not teacher.training and all(not m.training for m in teacher.modules())
    assert all(not p.requires_grad for p in teacher.parameters())
    assert all(torch.equal(v, state[k]) for k, v in teacher.state_dict().items())
    hy["kd_flag"]["teacher_model"] = "point_pillar_disconet_pupil"
    with pytest.raises(ImportError):
        tu.create_teacher(hy)


@pytest.mark.grad
@pytest.mark.parametrize("prefix", sorted(LOSS_CASES))
def test_loss_matches_reference_value_kd_term_and_gradient(g, prefix):
    """The CPU path is the reference's torch arithmetic in fp32: 1e-6 relative on the two values, 1e-6 of the gradient's maximum
    on the gradient."""
    from heal_amd.opencood.tools.train_utils import create_loss
    crit = create_loss(configs.lidar_disco_kd())
    out, tgt = loss_case(g, prefix)
    assert tuple(out["feature"].shape) == LOSS_CASES[prefix]
    total = crit(out, tgt)
    total.backward()
    for key in ("total_loss", "kd_loss"):
        got, want = crit.loss_dict[key], float(g[f"{prefix}{key}"])
        print(f"{prefix}{key}: {got!r} vs reference {want!r}")
        assert abs(got - want) <= 1e-6 * abs(want), (key, got, want)
    assert float(total.detach()) == crit.loss_dict["total_loss"]
    assert {"reg_loss", "cls_loss", "dir_loss"} <= set(crit.loss_dict)
    e = rel_err(out["feature"].grad.numpy(), g[f"{prefix}grad"])
    assert e <= 1e-6, e
    assert bool(torch.isfinite(out["feature"].grad).all())


def test_gap_case_underflows_teacher_probabilities(g):
    """The fixture's point: more than a fifth of the teacher's probabilities are exactly 0 in fp32, and the reference's values
    for it are finite."""
    t = torch.from_numpy(g["gap_t_code"].astype(np.float32) / np.float32(g["gap_t_scale"]))
    p = torch.softmax(t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]), dim=1)
    assert float((p == 0).float().mean()) > 0.2
    gap = t.max(dim=1)[0] - t.min(dim=1)[0]
    assert float(gap.max()) > 110
    assert np.isfinite(g["gap_total_loss"]) and np.isfinite(g["gap_grad"]).all()


def test_decoder_kd_is_refused():
    from heal_amd.opencood.tools.train_utils import create_loss
    hy = configs.lidar_disco_kd()
    hy["loss"]["args"]["kd"]["decoder_kd"] = True
    with pytest.raises(NotImplementedError, match="decoder_kd"):
        create_loss(hy)


def test_loss_logging_prints_the_kd_term(g, capsys):
    from heal_amd.opencood.tools.train_utils import create_loss
    crit = create_loss(configs.lidar_disco_kd())
    crit.loss_dict = {"total_loss": 3.0, "cls_loss": 1.0, "reg_loss": 0.5, "dir_loss": 0.25, "kd_loss": 1.25}
    tags = []

    class Writer:
        def add_scalar(self, tag, value, step):
            tags.append((tag, value, step))
    crit.logging(2, 4, 10, Writer())
    line = capsys.readouterr().out
    assert "[epoch 2][5/10]" in line and "KD Loss: 1.2500" in line and "Loss: 3.0000" in line
    assert ("Kd_loss", 1.25, 24) in tags and ("Regression_loss", 0.5, 24) in tags


def test_abi_declares_and_exports_the_kd_entry_points():
    declared = _capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/heal_amd.h"
        assert name in _capi.signatures(), f"{name} has no ctypes signature"
    assert _capi.abi_version_of_header() == 13          # (12 when these were added, additively; 13: heal_voxelize_layout)
    from heal_amd import build
    build.build()
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libheal_amd.so does not export {name}"
    header = open(_capi.HEADER).read()
    assert header.count("point_pillar_disconet_loss.py:35-46") >= 1 and "heal_kd_kl_loss_workspace(int n" in header
    # the workspace query is host arithmetic: one fp32 partial per 64-pixel tile of every image, rounded up to 256 B
    assert _capi.query("heal_kd_kl_loss_workspace", 2, 256, 256, 256) == 2 * 1024 * 4
    assert _capi.query("heal_kd_kl_loss_workspace", 1, 64, 13, 11) == 256
    assert _capi.query("heal_kd_kl_loss_workspace", 3, 7, 13, 11) == 256
    assert _capi.query("heal_kd_kl_loss_workspace", 0, 7, 13, 11) == 0
    assert _capi.query("heal_kd_kl_loss_workspace", 1, 0, 13, 11) == 0


def test_kd_ops_refuse_cpu_tensors_and_route_them_to_torch():
    from heal_amd import ops
    from heal_amd.opencood.loss.point_pillar_disconet_loss import PointPillarDiscoNetLoss
    s, t = torch.randn(1, 4, 3, 3), torch.randn(1, 4, 3, 3)
    assert not ops.kd_kl_supported(s, t)
    with pytest.raises(_capi.HealAmdError, match="CUDA"):
        ops.kd_kl_loss(s, t)
    want = torch.nn.functional.kl_div(torch.log_softmax(s.permute(0, 2, 3, 1).reshape(-1, 4), 1),
                                      torch.softmax(t.permute(0, 2, 3, 1).reshape(-1, 4), 1), reduction="sum") / s.numel()
    got = PointPillarDiscoNetLoss.kd_term(s, t)
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))


@pytest.mark.grad
def test_student_and_teacher_match_reference_on_cpu(g):
    student, teacher = m_models()
    data = m_data(g)
    out = student(data)
    check_student(g, out)
    t_out = teacher(data)
    check_teacher(g, t_out)
    # train_w_kd.py:144-146: the teacher's unprefixed dir_preds replaces the student's
    merged = dict(out)
    merged.update(t_out)
    assert merged["dir_preds"] is t_out["dir_preds"] and merged["cls_preds"] is out["cls_preds"]


def test_teacher_points_stack_every_agent_in_the_ego_frame():
    from heal_amd import synth
    poses = synth.agent_poses(7, 3, r_min=3.0, r_max=8.0)
    clouds = [np.array([[1.0, 2.0, -1.0, 0.5], [100.0, 0.0, -1.0, 0.1]], np.float32) for _ in poses]
    pts = synth.teacher_points(clouds, poses, M_RANGE)
    assert pts.dtype == np.float32 and pts.shape[1] == 4
    assert np.allclose(pts[0], clouds[0][0])                       # the ego's own point, unchanged; its far point is masked
    T = [synth.x_to_world(p) for p in poses]
    want = (np.linalg.solve(T[0], T[1]) @ np.array([1.0, 2.0, -1.0, 1.0]))[:3]
    assert any(np.allclose(p[:3], want, atol=1e-4) and p[3] == 0.5 for p in pts)
    assert np.all(np.abs(pts[:, :2]) < 12.8)
    calls = []

    def vox(p, b):
        calls.append((len(p), b))
        return np.zeros((2, 32, 4), np.float32), np.full((2, 4), b, np.int32), np.ones(2, np.int32)
    d = synth.teacher_processed_lidar([(clouds, poses), (clouds[:2], poses[:2])], M_RANGE, vox)
    assert [b for _, b in calls] == [0, 1] and d["voxel_coords"][:, 0].tolist() == [0, 0, 1, 1]     # one sample per scene
