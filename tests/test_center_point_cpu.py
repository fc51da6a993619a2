"""The anchor-free centre head without a GPU: the torch composition of CenterPointLoss against the reference's recordings
(tests/golden/center_small.npz), the config / factory / state_dict layout, the C header and the fixture's margins."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, configs
from heal_amd.opencood.loss import center_point_loss as L
from heal_amd.opencood.tools import train_utils
from tests.golden import center_margins as CM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5            # the bar of tests/test_gpu_det_loss.py
SYMBOLS = ("heal_center_loss_supported", "heal_center_loss_workspace", "heal_center_loss", "heal_center_boxes",
           "heal_center_decode_nms")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "center_small.npz"))


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize("prefix", CM.LOSS_CASES)
def test_composition_assigns_the_reference_targets(g, prefix):
    c = CM.loss_case(g, prefix)
    crit = L.CenterPointLoss(CM.loss_args(c))
    t = crit.assign_targets(torch.from_numpy(c["boxes"]), torch.from_numpy(c["mask"]))
    assert np.array_equal(t["inds"].numpy(), g[prefix + "inds"]) and t["inds"].dtype == torch.int64
    assert np.array_equal(t["masks"].numpy(), g[prefix + "masks"]) and t["masks"].dtype == torch.uint8
    heat, want = t["heatmaps"].numpy(), g[prefix + "heatmap"]
    assert heat.shape == want.shape
    assert np.array_equal(heat == 1, want == 1) and np.array_equal(heat == 0, want == 0)
    assert _rel(heat, want) <= TOL
    assert _rel(t["anno_boxes"].numpy(), g[prefix + "anno_boxes"]) <= TOL


@pytest.mark.grad
@pytest.mark.parametrize("prefix", CM.LOSS_CASES)
def test_composition_matches_reference_terms_and_gradients(g, prefix):
    c = CM.loss_case(g, prefix)
    crit = L.CenterPointLoss(CM.loss_args(c))
    cls = torch.from_numpy(c["cls"]).requires_grad_(True)
    bbox = torch.from_numpy(c["bbox"]).requires_grad_(True)
    total = crit({"cls_preds": cls, "bbox_preds": bbox},
                 {"object_bbx_center": torch.from_numpy(c["boxes"]), "object_bbx_mask": torch.from_numpy(c["mask"])})
    total.backward()
    for key in ("cls_loss", "reg_loss", "total_loss"):
        err = abs(crit.loss_dict[key] - float(g[prefix + key])) / abs(float(g[prefix + key]))
        print(prefix, key, crit.loss_dict[key], err)
        assert err <= TOL
    for name, grad in (("grad_cls", cls.grad), ("grad_bbox", bbox.grad)):
        err = _rel(grad.numpy(), g[prefix + name])
        print(prefix, name, err)
        assert err <= TOL


def test_single_suffix_keys_and_logging(g, capsys):
    c = CM.loss_case(g, "a_")
    crit = L.CenterPointLoss(CM.loss_args(c))
    total = crit({"cls_preds_single": torch.from_numpy(c["cls"]), "bbox_preds_single": torch.from_numpy(c["bbox"])},
                 {"object_bbx_center_single": torch.from_numpy(c["boxes"]),
                  "object_bbx_mask_single": torch.from_numpy(c["mask"])}, suffix="_single")
    assert abs(float(total) - float(g["a_total_loss"])) <= TOL * float(g["a_total_loss"])
    assert sorted(crit.loss_dict) == ["cls_loss", "reg_loss", "total_loss"]
    crit.logging(1, 2, 10, suffix="_single")
    line = capsys.readouterr().out
    assert "[epoch 1][3/10]_single" in line and "Conf Loss" in line and "Loc Loss" in line


def test_fixture_keeps_its_margins(g):
    for prefix in CM.LOSS_CASES:
        cell, rad, logit, finite = CM.loss_margins(CM.loss_case(g, prefix), L.gaussian_radius)
        assert cell >= CM.CELL_MARGIN and rad >= CM.CELL_MARGIN and logit >= CM.LOGIT_MARGIN and finite, (prefix, cell, rad, logit)
    assert np.abs(g["box_bbox"][:, 6]).min() >= 1e-3
    args = (float(g["dec_score_thr"]), float(g["dec_dir_offset"]), int(g["dec_num_bins"]), float(g["dec_nms_thr"]),
            g["dec_gt_range"].tolist())
    for tag, with_dir in (("d", True), ("n", False), ("m", True)):
        bad, info = CM.offenders(CM.case_cavs(g, tag), *args, with_dir)
        assert not bad and info["near_threshold"] == 0 and info["min_score_gap"] >= CM.SCORE_MARGIN, (tag, bad, info)
        assert info["pairs_above"] >= 1 and info["pairs_overlapping_below"] >= 1 and info["too_large"] >= 2, info
        assert info["bad_z"] >= 2 and info["out_of_range"] >= 1, info


def test_fixture_holds_the_cases_it_names(g):
    m, i, heat = g["c_masks"], g["c_inds"], g["c_heatmap"]
    assert m[0].sum() == 0 and g["c_mask"][1].sum() == 11 and m[1].tolist() == [1, 1, 1, 0, 1, 1, 0, 1]
    assert i[1, 1] == i[1, 2] and int((heat[1] == 1).sum()) == 5            # two objects in one cell: one positive cell
    assert i[1, 3] == 0 and i[1, 4] == 20 * 32 and i[1, 5] == 32 * 32 - 1   # out of range; centre in (-1, 0); last cell
    assert g["c_boxes"][1, 6, 3] == 0 and g["c_mask"][2].tolist()[:5] == [0, 1, 0, 1, 1] and m[2].tolist()[:4] == [1, 1, 1, 0]
    assert g["c_cls"][1, 0, 9, 8] == 12 and heat[1, 0, 9, 8] == 1 and g["c_grad_cls"][1, 0, 9, 8] == 0
    assert g["c_cls"][2, 0, 30, 2] == -12 and heat[2, 0, 30, 2] == 0 and g["c_grad_cls"][2, 0, 30, 2] == 0
    assert g["b_heatmap"].min() > 0 and int(g["b_min_radius"]) == 5 and g["a_cls"].shape[2:] == (13, 11)


@pytest.mark.parametrize("fusion,core", [("max", "center_point_baseline"), (None, "center_point")])
def test_factories_resolve_the_models_and_the_loss(fusion, core):
    hypes = configs.lidar_centerpoint(fusion, [-12.8, -12.8, -3, 12.8, 12.8, 1])
    assert hypes["model"]["core_method"] == core and hypes["loss"]["core_method"] == "center_point_loss"
    model = train_utils.create_model(hypes)
    assert type(model).__name__ == core.title().replace("_", "")
    assert tuple(model.reg_head.weight.shape) == (8, 256, 1, 1) and tuple(model.cls_head.weight.shape) == (1, 256, 1, 1)
    assert abs(float(model.cls_head.bias[0]) + np.log(99.0)) < 1e-6 and float(model.reg_head.weight.std()) < 2e-3
    crit = train_utils.create_loss(hypes)
    assert type(crit).__name__ == "CenterPointLoss" and crit.feature_map_size() == (32, 32)


def test_state_dict_names_and_shapes_match_the_reference():
    want = json.load(open(os.path.join(GOLDEN, "center_state_dict_keys.json")))
    built = {"center_point_baseline": configs.lidar_centerpoint("max"), "center_point": configs.lidar_centerpoint(None),
             "center_point_baseline_dir": configs.lidar_centerpoint("max", dir_head=True)}
    for name, hypes in built.items():
        got = {k: list(v.shape) for k, v in train_utils.create_model(hypes).state_dict().items()}
        assert got == want[name], (name, sorted(set(got) ^ set(want[name])))
    assert "dir_head.weight" in want["center_point_baseline_dir"] and "dir_head.weight" not in want["center_point"]


def test_backbone_fix_freezes_all_but_the_fusion_net_and_the_direction_head():
    """center_point_baseline.py:84-107 (max fusion has no parameters: the direction head is what stays trainable)."""
    hypes = configs.lidar_centerpoint("max", [-12.8, -12.8, -3, 12.8, 12.8, 1], dir_head=True)
    hypes["model"]["args"]["backbone_fix"] = True
    model = train_utils.create_model(hypes)
    free = {n.split(".")[0] for n, p in model.named_parameters() if p.requires_grad}
    assert free == {"dir_head"}


def test_header_parses_and_the_library_exports_every_symbol():
    sig = _capi.signatures_center()
    assert sorted(sig) == sorted(SYMBOLS)
    I, P, D, F, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_float, ctypes.c_size_t
    assert sig["heal_center_loss_workspace"] == (Z, [I, I, I, I])
    assert sig["heal_center_loss_supported"] == (I, [I, I, I, I, P, P, I, I])
    assert sig["heal_center_loss"] == (I, [P] * 4 + [I] * 4 + [P, P, I, I, I, D, P, D, D] + [P] * 8 + [Z, P])
    assert sig["heal_center_boxes"] == (I, [P, I, I, I, P, P, I, P, P])
    assert sig["heal_center_decode_nms"] == (I, [P, P, P, I, I, I, F, F, F, I, P, P, P, P, P, I, P, Z, P])
    assert not set(sig) & set(_capi.signatures())                    # outside the versioned table, whose version stays
    assert _capi.header_define("HEAL_CENTER_MAX_OBJS", _capi.HEADER_CENTER) >= 500
    from heal_amd import build
    build.build()
    lib = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libheal_amd.so does not export {name}"
    header = open(_capi.HEADER_CENTER).read()
    for cite in ("center_point_loss.py:205-242", ":385-470", ":526-555", "center_point_baseline.py:154-216",
                 "voxel_postprocessor.py:305-306"):
        assert cite in header, cite


def test_supported_and_workspace_are_host_arithmetic():
    rng = (ctypes.c_double * 6)(-12.8, -12.8, -3, 12.8, 12.8, 1)
    vox = (ctypes.c_double * 3)(0.4, 0.4, 4)
    q = lambda *a: _capi.query("heal_center_loss_supported", *a)        # noqa: E731
    assert q(3, 12, 32, 32, rng, vox, 2, 8) == 1 and q(3, 12, 32, 32, rng, vox, 2, 500) == 1
    assert q(3, 12, 32, 31, rng, vox, 2, 8) == 0 and q(3, 12, 16, 16, rng, vox, 2, 8) == 0      # not the range's feature map
    assert q(3, 12, 16, 16, rng, vox, 4, 8) == 1
    assert q(3, 12, 32, 32, rng, vox, 2, _capi.header_define("HEAL_CENTER_MAX_OBJS", _capi.HEADER_CENTER) + 1) == 0
    assert q(0, 12, 32, 32, rng, vox, 2, 8) == 0 and q(3, 0, 32, 32, rng, vox, 2, 8) == 0
    rect = (ctypes.c_double * 6)(-4.4, -5.2, -3, 4.4, 5.2, 1)
    assert q(2, 10, 13, 11, rect, vox, 2, 8) == 1 and q(2, 10, 11, 13, rect, vox, 2, 8) == 0    # W along x
    ws = lambda *a: _capi.query("heal_center_loss_workspace", *a)       # noqa: E731
    assert ws(2, 13, 11, 8) == 256 + 256 + 512 + 256 and ws(2, 13, 11, 0) == 0 and ws(0, 13, 11, 8) == 0


def test_ops_refuse_cpu_tensors_and_the_loss_takes_the_composition(g):
    from heal_amd import ops
    c = CM.loss_case(g, "b_")
    cfg = L.CenterPointLoss(CM.loss_args(c))._kernel_cfg()
    t = [torch.from_numpy(c[k]) for k in ("cls", "bbox", "boxes", "mask")]
    assert not ops.center_loss_supported(*t, cfg["cav_lidar_range"], cfg["voxel_size"], cfg["out_size_factor"], cfg["max_objs"])
    with pytest.raises(_capi.HealAmdError):
        ops.center_loss(*t, **cfg)
    with pytest.raises(_capi.HealAmdError):
        ops.center_boxes(t[1], cfg["cav_lidar_range"], cfg["voxel_size"], 2)
