"""HeterModelBaselineMs -- the multiscale "CoAlign" baseline (reference: opencood/models/heter_model_baseline_ms.py:26-220).
Per modality encoder -> ResNet BEV backbone -> aligner (-> camera crop); the agent stack is level 0, levels i >= 1 are
`backbone.get_layer_i_feature` of the UN-fused stack; every level is fused with the same normalised affine matrix (AttFusion or
MaxFusion per level: one heal_warp_att_fuse_levels launch per scene on the device, fusion_in_one.fuse_levels), then
`decode_multiscale_feature`, the shrink header and the heads.  The fusion backbone's layer0 is never run -- level 0 is the stack
itself -- but its parameters exist, as in the reference, so that a reference checkpoint loads strictly."""
from collections import Counter

import torch
import torch.nn as nn

from heal_amd.opencood.models._heter_common import (anchor_heads, crop_camera_feature, detection_heads, modality_stems,
                                                     wants_depth_items)
from heal_amd.opencood.models.fuse_modules.fusion_in_one import AttFusion, MaxFusion, fuse_levels
from heal_amd.opencood.models.sub_modules.bev_blocks import AlignNet, DownsampleConv, ResNetBEVBackbone
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm, pairwise_to_host


class HeterModelBaselineMs(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.ego_modality = args["ego_modality"]
        self.stage2_added_modality = args.get("stage2_added_modality", None)
        for m, setting in modality_stems(self, args, lambda st: ResNetBEVBackbone(st["backbone_args"])):
            setattr(self, f"aligner_{m}", AlignNet(setting["aligner_args"]))
            if setting["sensor_type"] == "camera":
                grid = setting["camera_mask_args"]["grid_conf"]
                setattr(self, f"xdist_{m}", grid["xbound"][1] - grid["xbound"][0])
                setattr(self, f"ydist_{m}", grid["ybound"][1] - grid["ybound"][0])
        self.H = self.cav_range[4] - self.cav_range[1]
        self.W = self.cav_range[3] - self.cav_range[0]
        self.fake_voxel_size = 1
        self.supervise_single = bool(args.get("supervise_single", False))
        if self.supervise_single:
            self.cls_head_single, self.reg_head_single, self.dir_head_single = anchor_heads(args["in_head_single"], args)
        self.backbone = ResNetBEVBackbone(args["fusion_backbone"])
        n_levels = len(args["fusion_backbone"]["layer_nums"])
        method = args["fusion_method"]
        if method == "att":
            feat_dim = args["att"]["feat_dim"]
            if not isinstance(feat_dim, (list, tuple)) or len(feat_dim) < n_levels:
                raise ValueError(f"att.feat_dim must list one dimension per fusion level ({n_levels}), got {feat_dim!r}")
            self.fusion_net = nn.ModuleList([AttFusion(feat_dim[i]) for i in range(n_levels)])
        elif method == "max":
            self.fusion_net = nn.ModuleList([MaxFusion() for _ in range(n_levels)])
        else:   # the reference appends nothing for another name and then fuses no level at all
            raise NotImplementedError(f"HeterModelBaselineMs: fusion_method '{method}' (the reference builds max | att)")
        self.shrink_flag = "shrink_header" in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args["shrink_header"])
        self.cls_head, self.reg_head, self.dir_head = anchor_heads(args["in_head"], args)

    def encode_modality(self, data_dict, m):
        """encoder -> backbone -> aligner (-> camera crop) for all agents of modality m (:142-168)."""
        f = getattr(self, f"encoder_{m}")(data_dict, m)
        f = getattr(self, f"backbone_{m}")({"spatial_features": f})["spatial_features_2d"]
        return crop_camera_feature(self, m, getattr(self, f"aligner_{m}")(f))

    def heads(self, fused):
        if self.shrink_flag:
            fused = self.shrink_conv(fused)
        return detection_heads(fused, self.cls_head, self.reg_head, self.dir_head)

    def forward(self, data_dict):
        output_dict = {}
        agent_modality_list = data_dict["agent_modality_list"]
        pairwise, _ = pairwise_to_host(data_dict["pairwise_t_matrix"])
        affine_matrix = normalize_pairwise_tfm(pairwise, self.H, self.W, self.fake_voxel_size)
        record_len = data_dict["record_len"]
        counts = Counter(agent_modality_list)
        feats = {}
        for m in self.modality_name_list:
            if m not in counts:
                continue
            feats[m] = self.encode_modality(data_dict, m)
            if wants_depth_items(self, m):
                output_dict[f"depth_items_{m}"] = getattr(self, f"encoder_{m}").depth_items
        if len(counts) == 1:      # one modality: the encoder's batch IS the agent stack (no copy)
            x = feats[agent_modality_list[0]]
        else:
            cursor = {m: 0 for m in self.modality_name_list}
            parts = []
            for m in agent_modality_list:
                parts.append(feats[m][cursor[m]])
                cursor[m] += 1
            x = torch.stack(parts)
        if self.supervise_single:
            output_dict.update({"cls_preds_single": self.cls_head_single(x), "reg_preds_single": self.reg_head_single(x),
                                "dir_preds_single": self.dir_head_single(x)})
        feature_list = [x]        # the fusion backbone's first layer is omitted (:196-202)
        for i in range(1, len(self.fusion_net)):
            x = self.backbone.get_layer_i_feature(x, layer_i=i)
            feature_list.append(x)
        fused = self.backbone.decode_multiscale_feature(fuse_levels(self.fusion_net, feature_list, record_len, affine_matrix))
        cls_preds, reg_preds, dir_preds = self.heads(fused)
        output_dict.update({"cls_preds": cls_preds, "reg_preds": reg_preds, "dir_preds": dir_preds})
        return output_dict
