"""SECOND trunk + SSFA neck with a per-box pose uncertainty head -- the SECOND flavour of CoAlign's first stage: host mirror of
opencood/models/second_ssfa_uncertainty.py:16-86.

Same constructor `args` as models/second_ssfa.py plus `anchor_num`, `uncertainty_dim` and an optional `dir_args`; the reference's
attribute names (`vfe`, `spconv_block`, `map_to_bev`, `ssfa`, `shrink_conv`, `cls_head`, `reg_head`, `unc_head`, `dir_head`) and
output keys (`cls_preds`, `reg_preds`, `unc_preds`, `dir_preds`).  `unc_preds` is [N, uncertainty_dim * A, H, W] as in
models/point_pillar_uncertainty.py.  The reference's `weight_init` only changes the initial values."""
import torch.nn as nn

from heal_amd.opencood.models.point_pillar import head
from heal_amd.opencood.models.second_ssfa import _SecondSSFATrunk


class SecondSSFAUncertainty(_SecondSSFATrunk):
    def __init__(self, args):
        super().__init__(args)
        self.cls_head = nn.Conv2d(self.out_channel, args['anchor_num'], kernel_size=1)
        self.reg_head = nn.Conv2d(self.out_channel, 7 * args['anchor_num'], kernel_size=1)
        self.unc_head = nn.Conv2d(self.out_channel, args['uncertainty_dim'] * args['anchor_num'], kernel_size=1)
        self.use_dir = 'dir_args' in args
        if self.use_dir:
            self.dir_head = nn.Conv2d(self.out_channel, args['dir_args']['num_bins'] * args['anchor_num'], kernel_size=1)

    def forward(self, data_dict):
        out = self.bev_features(data_dict)
        output_dict = {'cls_preds': head(self.cls_head, out), 'reg_preds': head(self.reg_head, out),
                       'unc_preds': head(self.unc_head, out)}
        if self.use_dir:
            output_dict['dir_preds'] = head(self.dir_head, out)
        return output_dict
