"""Single-agent CenterPoint detector: host mirror of opencood/models/center_point.py:12-145.

The PointPillars trunk of point_pillar.py (`pillar_vfe`, `scatter`, `backbone`, optional `shrink_conv`; K2 + the BEV kernels)
with the anchor-free centre heads: `cls_head` (one score per cell) and an 8-channel `reg_head`
(dx, dy, z, h, w, l, sin, cos in feature-map units).  Outputs `cls_preds`, `bbox_preds` (the raw head, what the criterion reads)
and `reg_preds` [N, H*W, 7] in metres from the streaming kernel heal_center_boxes (ops.center_boxes), which replaces the ~25
launches of generate_predicted_boxes (:83-145).  No gradient flows through `reg_preds`.  Same state_dict names and shapes."""
import numpy as np
import torch.nn as nn

from heal_amd import ops
from heal_amd.opencood.models.point_pillar import _PillarDetector, head


class _CenterDetector(_PillarDetector):
    """_PillarDetector with the centre heads; `head_channels(args)` is the heads' input width."""

    def __init__(self, args):
        super().__init__(args)
        cin = self.head_channels(args)
        self.cls_head = nn.Conv2d(cin, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(cin, 8 * args["anchor_number"], kernel_size=1)
        self.out_size_factor = args["out_size_factor"]
        self.cav_lidar_range = args["lidar_range"]

    def head_channels(self, args):
        return self.out_channel

    def init_weight(self):
        """center_point.py:43-46: the focal-loss prior on the score bias, a small normal on the box weights."""
        pi = 0.01
        nn.init.constant_(self.cls_head.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.reg_head.weight, mean=0, std=0.001)

    def generate_predicted_boxes(self, cls_preds, box_preds, dir_cls_preds=None):
        """center_point.py:83-145 on heal_center_boxes: box_preds [N, 8, H, W] -> (cls_preds, boxes [N, H*W, 7])."""
        return cls_preds, ops.center_boxes(box_preds, self.cav_lidar_range, self.voxel_size, self.out_size_factor)

    def predictions(self, x):
        cls, bbox = head(self.cls_head, x), head(self.reg_head, x)
        out = {"cls_preds": cls, "reg_preds": self.generate_predicted_boxes(cls, bbox)[1], "bbox_preds": bbox}
        if self.use_dir:
            out["dir_preds"] = head(self.dir_head, x)
        return out


class CenterPoint(_CenterDetector):
    def __init__(self, args):
        super().__init__({k: v for k, v in args.items() if k != "dir_args"})      # :12-41 builds no direction head
        self.init_weight()

    def head_channels(self, args):
        return 128 * 2 if self.shrink_flag else 128 * 3                           # :32, whatever the backbone says

    def forward(self, data_dict):
        return self.predictions(self.bev_features(data_dict)[1])
