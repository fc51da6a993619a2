"""SECOND trunk + SSFA neck + CIA-SSD's IoU-aware head: host mirror of opencood/models/second_ssfa.py:15-57 -- MeanVFE ->
VoxelBackBone8x (sparse conv, K3) -> HeightCompression -> SSFA (sub_modules/cia_ssd_utils.py: heal_deconv3x3_s2 + heal_ssfa_blend)
(-> DownsampleConv) -> Head; output keys `reg_preds`, `cls_preds`, `dir_preds`, `iou_preds`.

Same constructor `args` (`lidar_range`, `voxel_size`, `mean_vfe`, `spconv`, `map2bev`, `ssfa`, optional `shrink_header`, `head`) and
the reference's attribute names (`vfe`, `spconv_block`, `map_to_bev`, `ssfa`, `shrink_conv`, `head`), so its checkpoints load with
strict=True.  The gradient path is chosen as in models/second.py."""
import numpy as np
import torch
import torch.nn as nn

from heal_amd.opencood.models.sub_modules.cia_ssd_utils import SSFA, Head
from heal_amd.opencood.models.sub_modules.downsample_conv import DownsampleConv
from heal_amd.opencood.models.sub_modules.height_compression import HeightCompression
from heal_amd.opencood.models.sub_modules.mean_vfe import MeanVFE
from heal_amd.opencood.models.sub_modules.sparse_backbone_3d import VoxelBackBone8x


class _SecondSSFATrunk(nn.Module):
    """What second_ssfa.py:16-34 and second_ssfa_uncertainty.py:17-38 construct alike, and the walk up to the heads."""

    def __init__(self, args):
        super().__init__()
        lidar_range = np.array(args['lidar_range'])
        grid_size = np.round((lidar_range[3:6] - lidar_range[:3]) / np.array(args['voxel_size'])).astype(np.int64)
        self.vfe = MeanVFE(args['mean_vfe'], args['mean_vfe']['num_point_features'])
        self.spconv_block = VoxelBackBone8x(args['spconv'], input_channels=args['spconv']['num_features_in'],
                                            grid_size=grid_size)
        self.map_to_bev = HeightCompression(args['map2bev'])
        self.ssfa = SSFA(args['ssfa'])
        self.out_channel = args['ssfa']['feature_num']
        self.shrink_flag = 'shrink_header' in args
        if self.shrink_flag:
            self.shrink_conv = DownsampleConv(args['shrink_header'])
            self.out_channel = args['shrink_header']['dim'][-1]

    def bev_features(self, data_dict):
        lidar = data_dict['processed_lidar']
        coords = lidar['voxel_coords']
        batch_dict = {'voxel_features': lidar['voxel_features'], 'voxel_coords': coords,
                      'voxel_num_points': lidar['voxel_num_points'],
                      'batch_size': int(coords[:, 0].max().item()) + 1}    # the batch index is padded into column 0
        batch_dict = self.vfe(batch_dict)
        if self.training and torch.is_grad_enabled():   # gradient path (sparse_backbone_3d.py: sparse on the device)
            batch_dict = self.spconv_block.forward_autograd(batch_dict)
        else:
            batch_dict = self.spconv_block(batch_dict)
        batch_dict = self.map_to_bev(batch_dict)
        out = self.ssfa(batch_dict['spatial_features'])
        return self.shrink_conv(out) if self.shrink_flag else out


class SecondSSFA(_SecondSSFATrunk):
    def __init__(self, args):
        super().__init__(args)
        self.head = Head(**args['head'])

    def forward(self, data_dict):
        return self.head(self.bev_features(data_dict))
