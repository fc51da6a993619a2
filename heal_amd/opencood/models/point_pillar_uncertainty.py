"""Single-agent PointPillars detector with a per-box pose uncertainty head -- CoAlign's first stage, whose boxes and
uncertainties the pose-graph alignment consumes: host mirror of opencood/models/point_pillar_uncertainty.py:14-76.

Same constructor `args` (`pillar_vfe`, `point_pillar_scatter`, `base_bev_backbone`, `uncertainty_dim`, `anchor_num` -- not the
`anchor_number` of the other PointPillar mirrors -- and an optional `dir_args`), `forward(data_dict)` reading
`data_dict['processed_lidar']`, same state_dict names (`pillar_vfe.*`, `backbone.*`, `cls_head/reg_head/unc_head/dir_head.*`):
a CoAlign stage-1 checkpoint loads with strict=True.  No shrink header: the heads sit on the 384-channel backbone output.
`unc_preds` is [N, uncertainty_dim * A, H, W], the channel of anchor a, component d being a * dim + d (the log-variance `s` of
opencood/loss/point_pillar_uncertainty_loss.py).  Stem through K2 and heads through conv_bias_act / grad_conv as in
models/point_pillar.py."""
import torch.nn as nn

from heal_amd.opencood.models.point_pillar import _PillarDetector, head


class PointPillarUncertainty(_PillarDetector):
    def __init__(self, args):
        if "shrink_header" in args:
            raise ValueError("point_pillar_uncertainty has no shrink header (point_pillar_uncertainty.py:27-38)")
        super().__init__({**args, "anchor_number": args["anchor_num"]})
        self.uncertainty_dim = args["uncertainty_dim"]      # 3: x, y, yaw;  2: x, y;  7: every regression target
        self.unc_head = nn.Conv2d(self.out_channel, self.uncertainty_dim * args["anchor_num"], kernel_size=1)
        if self.use_dir:                                    # the reference registers dir_head after unc_head
            self.dir_head = self._modules.pop("dir_head")

    def forward(self, data_dict):
        x = self.bev_features(data_dict)[1]
        out = self.predictions(x)
        out["unc_preds"] = head(self.unc_head, x)
        return out
