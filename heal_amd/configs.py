"""Hypes dictionaries for the BASELINE configurations, built in code with the reference's key names
(what `yaml_utils.load_yaml` returns for opencood/hypes_yaml/opv2v/LiDAROnly/lidar_pyramid.yaml,
MoreModality/HEAL/stage2/m1_single_pyramid.yaml, Single/m1_pointpillar_pretrain.yaml and
MoreModality/HEAL/final_infer/m1m2m3m4.yaml, inference-relevant sections only).
`dump_yaml` writes them out as a config.yaml that both loaders parse.
"""
import copy

import yaml

from heal_amd.opencood.hypes_yaml.yaml_utils import load_general_params, load_point_pillar_params, load_second_params

FULL_RANGE = [-102.4, -102.4, -3, 102.4, 102.4, 1]
ANCHOR_YAW = [0, 90]
DIR_ARGS = {"dir_offset": 0.7853, "num_bins": 2, "anchor_yaw": ANCHOR_YAW}


def _pointpillar_modality(lidar_range, aligner="identity"):
    aligner_args = {"core_method": "identity"} if aligner == "identity" else {
        "core_method": "convnext", "spatial_align": False, "args": {"num_of_blocks": 3, "dim": 64}}
    return {
        "core_method": "point_pillar",
        "sensor_type": "lidar",
        "encoder_args": {
            "voxel_size": [0.4, 0.4, 4],
            "lidar_range": list(lidar_range),
            "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
            "point_pillar_scatter": {"num_features": 64},
        },
        "backbone_args": {"layer_nums": [3], "layer_strides": [2], "num_filters": [64]},
        "aligner_args": aligner_args,
    }


def _fusion_backbone():
    return {"resnext": True, "layer_nums": [3, 5, 8], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256],
            "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128], "anchor_number": 2}


def _shrink_header():
    return {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [256], "input_dim": 384}


def _common(lidar_range, max_cav):
    r = list(lidar_range)
    return {
        "yaml_parser": "load_general_params",
        "train_params": {"batch_size": 1, "max_cav": max_cav},
        "cav_lidar_range": r,
        "preprocess": {
            "core_method": "SpVoxelPreprocessor",
            "args": {"voxel_size": [0.4, 0.4, 4], "max_points_per_voxel": 32, "max_voxel_train": 32000,
                     "max_voxel_test": 70000},
            "cav_lidar_range": r,
        },
        "postprocess": {
            "core_method": "VoxelPostprocessor",
            "gt_range": r,
            "anchor_args": {"cav_lidar_range": r, "l": 3.9, "w": 1.6, "h": 1.56, "r": list(ANCHOR_YAW),
                            "feature_stride": 2, "num": 2},
            "target_args": {"pos_threshold": 0.6, "neg_threshold": 0.45, "score_threshold": 0.2},
            "order": "hwl",
            "max_num": 150,
            "nms_thresh": 0.15,
            "dir_args": copy.deepcopy(DIR_ARGS),
        },
        # the loss block of the reference's *_pyramid.yaml files (training side)
        "loss": {"core_method": "point_pillar_pyramid_loss", "args": {
            "pos_cls_weight": 2.0,
            "cls": {"type": "SigmoidFocalLoss", "alpha": 0.25, "gamma": 2.0, "weight": 1.0},
            "reg": {"type": "WeightedSmoothL1Loss", "sigma": 3.0, "codewise": True, "weight": 2.0},
            "dir": {"type": "WeightedSoftmaxClassificationLoss", "weight": 0.2, "args": copy.deepcopy(DIR_ARGS)},
            "depth": {"weight": 1.0},
            "pyramid": {"relative_downsample": [1, 2, 4], "weight": [0.4, 0.2, 0.1]}}},
    }


def lidar_pyramid(lidar_range=FULL_RANGE, max_cav=5):
    """PointPillars + PyramidFusion collaborative model (BASELINE configs 3 and the LiDAR part of 4)."""
    h = _common(lidar_range, max_cav)
    h["name"] = "heal_amd_opv2v_lidar_pyramid"
    h["model"] = {"core_method": "heter_pyramid_collab", "args": {
        "lidar_range": list(lidar_range), "supervise_single": True,
        "m1": _pointpillar_modality(lidar_range, "identity"),
        "fusion_backbone": _fusion_backbone(), "shrink_header": _shrink_header(),
        "in_head": 256, "anchor_number": 2, "dir_args": copy.deepcopy(DIR_ARGS)}}
    return load_general_params(h)


def m1_single_pyramid(lidar_range=FULL_RANGE):
    """Single-agent PointPillars through the pyramid backbone (BASELINE configs 1/2)."""
    h = _common(lidar_range, 1)
    h["name"] = "heal_amd_opv2v_m1_single_pyramid"
    h["model"] = {"core_method": "heter_pyramid_single", "args": {
        "ego_modality": "m1", "lidar_range": list(lidar_range), "fix_encoder": False,
        "m1": _pointpillar_modality(lidar_range, "convnext"),
        "fusion_backbone": _fusion_backbone(), "shrink_header": _shrink_header(),
        "in_head": 256, "anchor_number": 2, "dir_args": copy.deepcopy(DIR_ARGS)}}
    return load_general_params(h)


def m1_late(lidar_range=FULL_RANGE):
    """Single-agent PointPillars detector of the late-fusion / pre-training recipe (configs 1/2)."""
    h = _common(lidar_range, 1)
    h["name"] = "heal_amd_opv2v_m1_pointpillar_late"
    m1 = _pointpillar_modality(lidar_range, "identity")
    m1["layers_args"] = {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256],
                         "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]}
    m1["shrink_header"] = _shrink_header()
    m1["head_args"] = {"in_head": 256}
    h["model"] = {"core_method": "heter_model_late", "args": {
        "ego_modality": "m1", "lidar_range": list(lidar_range), "m1": m1, "anchor_number": 2,
        "dir_args": copy.deepcopy(DIR_ARGS)}}
    return load_general_params(h)


def _camera_modality(lidar_range, final_dim, encoder, cam_bound=51.2):
    grid_conf = {"xbound": [-cam_bound, cam_bound, 0.4], "ybound": [-cam_bound, cam_bound, 0.4], "zbound": [-10, 10, 20.0],
                 "ddiscr": [2, 50, 48], "mode": "LID"}
    data_aug_conf = {"resize_lim": [0.65, 0.7] if encoder == "EfficientNet" else [0.56, 0.61],
                     "final_dim": list(final_dim), "rot_lim": [-3.6, 3.6], "H": 600, "W": 800, "rand_flip": False,
                     "bot_pct_lim": [0.0, 0.05], "cams": ["camera0", "camera1", "camera2", "camera3"], "Ncams": 4}
    return {
        "core_method": "lift_splat_shoot",
        "sensor_type": "camera",
        "encoder_args": {"anchor_number": 2, "grid_conf": grid_conf, "data_aug_conf": data_aug_conf,
                         "img_downsample": 8, "img_features": 128, "use_depth_gt": False,
                         "depth_supervision": True, "camera_encoder": encoder},
        "camera_mask_args": {"cav_lidar_range": list(lidar_range), "grid_conf": copy.deepcopy(grid_conf)},
        "backbone_args": {"layer_nums": [3], "layer_strides": [2], "num_filters": [64], "inplanes": 128},
        "aligner_args": {"core_method": "convnext", "spatial_align": False,
                         "args": {"num_of_blocks": 3, "dim": 64}},
    }


def _second_modality(lidar_range):
    return {
        "core_method": "second",
        "sensor_type": "lidar",
        "encoder_args": {"voxel_size": [0.1, 0.1, 0.1], "lidar_range": list(lidar_range),
                         "mean_vfe": {"num_point_features": 4},
                         "spconv": {"num_features_in": 4, "num_features_out": 64},
                         "map2bev": {"feature_num": 128}},
        "backbone_args": {"layer_nums": [3], "layer_strides": [1], "num_filters": [64], "inplanes": 128},
        "aligner_args": {"core_method": "convnext", "spatial_align": False,
                         "args": {"num_of_blocks": 3, "dim": 64}},
    }


def heal_heter(modalities=("m1", "m2", "m3", "m4"), lidar_range=FULL_RANGE, max_cav=5, cam_bound=51.2, cam_dims=None):
    """HEAL final-infer collaborative model with several modalities (m1 PointPillars LiDAR,
    m2 Lift-Splat EfficientNet 384x512, m4 Lift-Splat Resnet101 336x448; m3 SECOND when built) --
    MoreModality/HEAL/final_infer/m1m2m3m4.yaml, BASELINE config 4.  `cam_bound` / `cam_dims` ({"m2": (H, W), ...})
    shrink the camera BEV grid and the image sizes for reduced-size parity tests."""
    cam_dims = dict({"m2": (384, 512), "m4": (336, 448)}, **(cam_dims or {}))
    h = _common(lidar_range, max_cav)
    h["name"] = "heal_amd_opv2v_" + "".join(modalities)
    args = {"ego_modality": "m1", "lidar_range": list(lidar_range), "supervise_single": True}
    for m in modalities:
        if m == "m1":
            args[m] = _pointpillar_modality(lidar_range, "identity")
        elif m == "m2":
            args[m] = _camera_modality(lidar_range, cam_dims["m2"], "EfficientNet", cam_bound)
        elif m == "m3":
            args[m] = _second_modality(lidar_range)
        elif m == "m4":
            args[m] = _camera_modality(lidar_range, cam_dims["m4"], "Resnet101", cam_bound)
        else:
            raise NotImplementedError(f"modality {m}")
    args.update({"fusion_backbone": _fusion_backbone(), "shrink_header": _shrink_header(), "in_head": 256,
                 "anchor_number": 2, "dir_args": copy.deepcopy(DIR_ARGS)})
    h["model"] = {"core_method": "heter_pyramid_collab", "args": args}
    return load_general_params(h)


def _v2xvit_args():
    return {"transformer": {"encoder": {
        "num_blocks": 1, "depth": 3, "use_roi_mask": True, "use_RTE": False, "RTE_ratio": 0,
        "cav_att_config": {"dim": 256, "use_hetero": True, "use_RTE": False, "RTE_ratio": 0, "heads": 8,
                           "dim_head": 32, "dropout": 0.3},
        "pwindow_att_config": {"dim": 256, "heads": [16, 8, 4], "dim_head": [16, 32, 64], "dropout": 0.3,
                               "window_size": [4, 8, 16], "relative_pos_embedding": True,
                               "fusion_method": "split_attn"},
        "feed_forward": {"mlp_dim": 256, "dropout": 0.3},
        "sttf": {"voxel_size": [0.4, 0.4, 4], "downsample_rate": 4}}}}


def _baseline_modality(base, strides, inplanes=None):
    m = {k: v for k, v in base.items() if k in ("core_method", "sensor_type", "encoder_args", "camera_mask_args")}
    m["backbone_args"] = {"layer_nums": [3, 5, 8], "layer_strides": list(strides), "num_filters": [64, 128, 256],
                          "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]}
    if inplanes:
        m["backbone_args"]["inplanes"] = inplanes
    m["shrink_header"] = {"kernal_size": [3], "stride": [2], "padding": [1], "dim": [256], "input_dim": 384}
    return m


def lidar_baseline(fusion_method="v2xvit", lidar_range=FULL_RANGE, max_cav=5, modality="m1"):
    """HeterModelBaseline (LiDAROnly/lidar_v2xvit.yaml; BASELINE config 5 with modality='m3'):
    encoder -> plain BEV backbone -> shrinker -> single-scale fusion (v2xvit | att | max | cobevt | v2vnet | disconet | where2comm | who2com) -> heads."""
    h = _common(lidar_range, max_cav)
    h["name"] = f"heal_amd_opv2v_{modality}_{fusion_method}"
    if modality == "m1":
        mod = _baseline_modality(_pointpillar_modality(lidar_range), (2, 2, 2))
    elif modality == "m3":
        mod = _baseline_modality(_second_modality(lidar_range), (1, 2, 2), inplanes=128)
    else:
        raise NotImplementedError(modality)
    args = {"ego_modality": modality, "lidar_range": list(lidar_range), modality: mod, "fusion_method": fusion_method,
            "in_head": 256, "anchor_number": 2, "dir_args": copy.deepcopy(DIR_ARGS)}
    if fusion_method == "v2xvit":
        args["v2xvit"] = _v2xvit_args()
    elif fusion_method == "att":
        args["att"] = {"feat_dim": 256}
    elif fusion_method == "cobevt":     # LiDAROnly/lidar_cobevt.yaml
        args["cobevt"] = {"input_dim": 256, "mlp_dim": 256, "agent_size": max_cav, "window_size": 4, "dim_head": 32,
                          "drop_out": 0.1, "depth": 3}
    elif fusion_method == "v2vnet":     # LiDAROnly/lidar_v2vnet.yaml; conv_gru.H / W: the fusion map (128 x 128 on the full range)
        H = int(round((lidar_range[4] - lidar_range[1]) / (0.4 * 4)))
        W = int(round((lidar_range[3] - lidar_range[0]) / (0.4 * 4)))
        args["v2vnet"] = {"num_iteration": 2, "in_channels": 256, "gru_flag": True, "agg_operator": "avg",
                          "conv_gru": {"H": H, "W": W, "num_layers": 1, "kernel_size": [[3, 3]]}}
    elif fusion_method == "disconet":   # LiDAROnly/lidar_disco.yaml
        args["disconet"] = {"feat_dim": 256}
    elif fusion_method in ("where2comm", "who2com"):    # heter_model_baseline.py:108-111: the entry is the feature width itself
        args[fusion_method] = 256
    h["model"] = {"core_method": "heter_model_baseline", "args": args}
    # encoder + backbone + stride-2 shrinker leave the map at 1/4 of the 0.4 m anchor grid (lidar_v2xvit.yaml: feature_stride 4)
    h["postprocess"]["anchor_args"]["feature_stride"] = 4
    return load_general_params(h)


def lidar_coalign(fusion_method="att", lidar_range=FULL_RANGE, max_cav=5):
    """HeterModelBaselineMs, the multiscale CoAlign baseline (LiDAROnly/lidar_coalign.yaml with its `att` block repaired,
    INTEGRATION.md): PointPillars -> one-level ResNet backbone -> identity aligner, then three fusion levels (64 / 128 / 256
    channels at 1, 1/2, 1/4 of the 0.8 m map), each fused over the agents (att | max), decoded and shrunk to 256 channels."""
    h = _common(lidar_range, max_cav)
    h["name"] = f"heal_amd_opv2v_lidar_coalign_{fusion_method}"
    args = {"ego_modality": "m1", "lidar_range": list(lidar_range), "supervise_single": False,
            "m1": _pointpillar_modality(lidar_range, "identity"), "fusion_method": fusion_method,
            "fusion_backbone": {"layer_nums": [3, 5, 8], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256],
                                "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]},
            "shrink_header": _shrink_header(), "in_head": 256, "anchor_number": 2, "dir_args": copy.deepcopy(DIR_ARGS)}
    if fusion_method == "att":
        args["att"] = {"feat_dim": [64, 128, 256]}
    elif fusion_method != "max":
        raise NotImplementedError(f"lidar_coalign: fusion_method '{fusion_method}' (max | att)")
    h["model"] = {"core_method": "heter_model_baseline_ms", "args": args}
    return load_general_params(h)      # feature_stride 2 (the _common default): the fused map is the backbone's stride-2 grid


def oldstyle_pointpillar(fusion_method=None, lidar_range=FULL_RANGE, max_cav=5, compression=0):
    """Old-style YAML (v2xsim2/visualization.yaml `model` block): core_method point_pillar, or
    point_pillar_baseline when a fusion_method (max | att | v2xvit) is given.  Uses the `processed_lidar` key."""
    h = _common(lidar_range, max_cav)
    args = {"voxel_size": [0.4, 0.4, 4], "lidar_range": list(lidar_range), "anchor_number": 2, "max_cav": max_cav,
            "backbone_fix": False,
            "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
            "point_pillar_scatter": {"num_features": 64},
            "base_bev_backbone": {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256],
                                  "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]},
            "shrink_header": {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [256], "input_dim": 384},
            "dir_args": copy.deepcopy(DIR_ARGS)}
    core = "point_pillar"
    if fusion_method is not None:
        core = "point_pillar_baseline"
        args["fusion_method"] = fusion_method
        if fusion_method == "att":
            args["att"] = {"feat_dim": 256}
        elif fusion_method == "v2xvit":
            args["v2xvit"] = _v2xvit_args()
        if compression:
            args["compression"] = compression
    h["name"] = f"heal_amd_{core}"
    h["model"] = {"core_method": core, "args": args}
    return load_general_params(h)


def lidar_centerpoint(fusion_method="max", lidar_range=FULL_RANGE, max_cav=5, dir_head=False):
    """Anchor-free centre head on the old-style PointPillars trunk: core_method center_point_baseline with a fusion_method
    (max | att | v2xvit), or the single-agent center_point with fusion_method=None; center_point_loss as the criterion.
    The reference ships no CenterPoint YAML: the KEY NAMES are the ones its code reads (center_point_baseline.py:22-77,
    center_point_loss.py:189-203, :385-396); the VALUES are this project's -- the stride-2 head map of the trunk
    (out_size_factor 2), CenterPoint's customary max_objs 500, min_radius 2 and gaussian_overlap 0.1, unit code weights."""
    h = _common(lidar_range, max_cav)
    voxel_size, factor = [0.4, 0.4, 4], 2
    args = {"voxel_size": list(voxel_size), "lidar_range": list(lidar_range), "anchor_number": 1, "max_cav": max_cav,
            "out_size_factor": factor, "backbone_fix": False,
            "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
            "point_pillar_scatter": {"num_features": 64},
            "base_bev_backbone": {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256],
                                  "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]},
            "shrink_header": {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [256], "input_dim": 384}}
    core = "center_point"
    if fusion_method is not None:
        core = "center_point_baseline"
        args["fusion_method"] = fusion_method
        if fusion_method == "att":
            args["att"] = {"feat_dim": 256}
        elif fusion_method == "v2xvit":
            args["v2xvit"] = _v2xvit_args()
        if dir_head:
            args["dir_args"] = copy.deepcopy(DIR_ARGS)
    h["name"] = f"heal_amd_{core}"
    h["model"] = {"core_method": core, "args": args}
    h["postprocess"]["anchor_args"].update({"r": [0], "num": 1})
    if not (dir_head and fusion_method is not None):
        h["postprocess"].pop("dir_args")
    h["loss"] = {"core_method": "center_point_loss", "args": {
        "cls_weight": 1.0, "loc_weight": 2.0, "code_weights": [1.0] * 8,
        "target_assigner_config": {"max_objs": 500, "min_radius": 2, "gaussian_overlap": 0.1, "out_size_factor": factor,
                                   "voxel_size": list(voxel_size), "cav_lidar_range": list(lidar_range)}}}
    return load_general_params(h)


def lidar_uncertainty(lidar_range=FULL_RANGE, dim=3, dir_head=True):
    """CoAlign's first stage: core_method point_pillar_uncertainty (the single-agent PointPillars detector with a per-box pose
    uncertainty head of `dim` components: 2 = x, y; 3 = x, y, yaw; 7 = every regression target), point_pillar_uncertainty_loss
    and the UncertaintyVoxelPostprocessor.  The reference ships no YAML for this model: the KEY NAMES are the ones its code
    reads (point_pillar_uncertainty.py:14-41, point_pillar_uncertainty_loss.py:16-22, :195-216); the VALUES of the
    `uncertainty` block are this project's test values, not recovered ones."""
    h = _common(lidar_range, 1)
    args = {"voxel_size": [0.4, 0.4, 4], "lidar_range": list(lidar_range), "anchor_num": 2, "uncertainty_dim": dim,
            "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
            "point_pillar_scatter": {"num_features": 64},
            "base_bev_backbone": {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256],
                                  "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]}}
    if dir_head:
        args["dir_args"] = copy.deepcopy(DIR_ARGS)
    h["name"] = "heal_amd_point_pillar_uncertainty"
    h["model"] = {"core_method": "point_pillar_uncertainty", "args": args}
    h["postprocess"]["core_method"] = "UncertaintyVoxelPostprocessor"
    if not dir_head:
        h["postprocess"].pop("dir_args")
    base = h["loss"]["args"]
    h["loss"] = {"core_method": "point_pillar_uncertainty_loss", "args": {
        "pos_cls_weight": base["pos_cls_weight"], "cls": base["cls"], "reg": base["reg"],
        "uncertainty": {"weight": 0.25, "dim": dim, "xy_loss_type": "l2", "angle_loss_type": "von-mise", "angle_weight": 0.5,
                        "lambda_V": 0.001, "s0": 1.0, "limit_period": True}}}
    if dir_head:
        h["loss"]["args"]["dir"] = base["dir"]
    return load_general_params(h)


SSFA_RANGE = [-140.8, -40, -3, 140.8, 40, 1]


def second_ssfa(lidar_range=SSFA_RANGE, uncertainty_dim=None, dir_head=True):
    """The SECOND + SSFA detectors.  uncertainty_dim None: core_method second_ssfa (second_ssfa.py:15-57) with CIA-SSD's `head` block
    (box, class, IoU and, with dir_head, direction maps) and the VoxelPostprocessor, whose post_process rescores with `iou_preds`.
    uncertainty_dim 2 | 3 | 7: core_method second_ssfa_uncertainty (second_ssfa_uncertainty.py:16-86), the SECOND flavour of
    CoAlign's first stage, with `anchor_num` / `uncertainty_dim` / `dir_args`, point_pillar_uncertainty_loss and the
    UncertaintyVoxelPostprocessor as in lidar_uncertainty.  0.1 m voxels, the BEV map at stride 8 (100 x 352 for the default
    +-140.8 m x +-40 m range).  The reference ships no YAML for either model: the KEY NAMES are the ones its code reads."""
    if uncertainty_dim is not None:
        h = lidar_uncertainty(lidar_range, uncertainty_dim, dir_head)
    else:
        h = _common(lidar_range, 1)
        if not dir_head:
            h["postprocess"].pop("dir_args")
    h["preprocess"]["args"] = {"voxel_size": [0.1, 0.1, 0.1], "max_points_per_voxel": 5, "max_voxel_train": 36000,
                               "max_voxel_test": 70000}
    h["postprocess"]["anchor_args"]["feature_stride"] = 8
    h["yaml_parser"] = "load_second_params"
    args = {"lidar_range": list(lidar_range), "voxel_size": [0.1, 0.1, 0.1], "mean_vfe": {"num_point_features": 4},
            "spconv": {"num_features_in": 4, "num_features_out": 64}, "map2bev": {"feature_num": 128},
            "ssfa": {"feature_num": 128}}
    if uncertainty_dim is not None:
        args.update({"anchor_num": 2, "uncertainty_dim": uncertainty_dim})
        if dir_head:
            args["dir_args"] = copy.deepcopy(DIR_ARGS)
        h["name"] = "heal_amd_second_ssfa_uncertainty"
        h["model"] = {"core_method": "second_ssfa_uncertainty", "args": args}
    else:
        args["head"] = {"num_input": 128, "num_pred": 14, "num_cls": 2, "num_iou": 2, "use_dir": bool(dir_head), "num_dir": 4}
        h["name"] = "heal_amd_second_ssfa"
        h["model"] = {"core_method": "second_ssfa", "args": args}
        h["loss"]["core_method"] = "point_pillar_loss"
        for k in ("depth", "pyramid"):
            h["loss"]["args"].pop(k)
        if not dir_head:
            h["loss"]["args"].pop("dir")
    return load_second_params(h)


def lidar_centerpoint_where2comm(agg="ATTEN", multi_scale=True, backbone="resnet", communication=True, lidar_range=FULL_RANGE,
                                 max_cav=5, thre=0.01, k_size=5, c_sigma=1.0):
    """core_method center_point_where2comm: lidar_centerpoint's trunk, heads and criterion with Where2comm's spatially masked
    fusion (`fusion_args`).  agg: ATTEN | MAX (agg_operator.mode); multi_scale: the fusion runs per backbone level on the canvas
    (downsample_rate 1: the affine matrix is normalised with the canvas size) or once on the stride-2 output map
    (downsample_rate 2); backbone: "resnet" (`base_bev_backbone.resnet`: every level from the unmasked input) | "plain" (the
    masked level feeds the next block); communication: False leaves the `communication` entry out (no mask, rate 0).
    The reference ships no YAML for this model: the KEY NAMES are the ones its code reads (center_point_where2comm.py:17-54,
    where2comm_attn.py:178-217, comm_modules/where2comm.py:13-21); the VALUES (thre 0.01, a 5 x 5 filter with sigma 1) are this project's
    defaults, to be replaced by a checkpoint's own."""
    if backbone not in ("resnet", "plain"):
        raise ValueError(f"backbone must be 'resnet' or 'plain', got {backbone!r}")
    h = lidar_centerpoint(None, lidar_range, max_cav)
    args = h["model"]["args"]
    bb = args["base_bev_backbone"]
    if backbone == "resnet":
        bb["resnet"] = True
    fusion = {"voxel_size": list(args["voxel_size"]), "downsample_rate": 1 if multi_scale else 2, "in_channels": 256,
              "multi_scale": bool(multi_scale), "layer_nums": list(bb["layer_nums"]), "num_filters": list(bb["num_filters"]),
              "agg_operator": {"mode": agg, "feature_dim": 256}}
    if communication:
        fusion["communication"] = {"thre": thre, "gaussian_smooth": {"k_size": k_size, "c_sigma": c_sigma}}
    args["fusion_args"] = fusion
    h["name"] = "heal_amd_center_point_where2comm"
    h["model"]["core_method"] = "center_point_where2comm"
    return h


def lidar_disco_kd(lidar_range=FULL_RANGE, max_cav=5):
    """DiscoNet with distillation (opv2v/LiDAROnly/lidar_disco.yaml): the student `point_pillar_disconet`, the early-fusion
    teacher of `kd_flag` (same architecture arguments, as the YAML's `*model_args` alias) and `point_pillar_disconet_loss` with
    its KD weight.  `kd_flag.teacher_path` is left empty: the YAML's points into its author's file system."""
    h = _common(lidar_range, max_cav)
    h["name"] = "heal_amd_opv2v_point_pillar_lidar_disconet"
    h["train_params"]["batch_size"] = 2
    args = {"voxel_size": [0.4, 0.4, 4], "lidar_range": list(lidar_range), "anchor_number": 2,
            "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
            "point_pillar_scatter": {"num_features": 64},
            "base_bev_backbone": {"layer_nums": [3, 5, 8], "layer_strides": [2, 2, 2], "num_filters": [64, 128, 256],
                                  "upsample_strides": [1, 2, 4], "num_upsample_filter": [128, 128, 128]},
            "shrink_header": {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [256], "input_dim": 384},
            "dir_args": copy.deepcopy(DIR_ARGS)}
    h["model"] = {"core_method": "point_pillar_disconet", "args": args}
    h["kd_flag"] = {"teacher_model": "point_pillar_disconet_teacher", "teacher_model_config": args,      # the YAML's alias: one dict
                    "teacher_path": ""}
    h["loss"] = {"core_method": "point_pillar_disconet_loss", "args": {
        "pos_cls_weight": 2.0,
        "cls": {"type": "SigmoidFocalLoss", "alpha": 0.25, "gamma": 2.0, "weight": 2.0},
        "reg": {"type": "WeightedSmoothL1Loss", "sigma": 3.0, "codewise": True, "weight": 2.0},
        "dir": {"type": "WeightedSoftmaxClassificationLoss", "weight": 0.2, "args": copy.deepcopy(DIR_ARGS)},
        "kd": {"weight": 10000}}}
    h["optimizer"] = {"core_method": "Adam", "lr": 0.002, "args": {"eps": 1e-10, "weight_decay": 1e-4}}
    h["lr_scheduler"] = {"core_method": "multistep", "gamma": 0.1, "step_size": [10, 15, 40]}
    h["yaml_parser"] = "load_point_pillar_params"
    return load_point_pillar_params(h)


def oldstyle_lss(encoder="EfficientNet", final_dim=(384, 512), lidar_range=FULL_RANGE, max_cav=5):
    """Old-style camera detector (opencood/models/lift_splat_shoot.py): core_method lift_splat_shoot, `image_inputs`
    key, resnet18-trunk BevEncode on the 256x256 pooled grid, stride-2 shrink header to the 128x128 anchor map."""
    h = _common(lidar_range, max_cav)
    enc = _camera_modality(lidar_range, final_dim, encoder)["encoder_args"]
    args = dict(enc, bevout_feature=128,
                shrink_header={"kernal_size": [3], "stride": [2], "padding": [1], "dim": [128], "input_dim": 128},
                dir_args=copy.deepcopy(DIR_ARGS))
    h["name"] = "heal_amd_lift_splat_shoot"
    h["model"] = {"core_method": "lift_splat_shoot", "args": args}
    return load_general_params(h)


def dump_yaml(hypes, path):
    def plain(o):
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        if hasattr(o, "tolist"):
            return o.tolist()
        return o
    with open(path, "w") as f:
        yaml.safe_dump(plain(hypes), f, sort_keys=False)
