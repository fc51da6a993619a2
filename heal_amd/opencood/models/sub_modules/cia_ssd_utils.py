"""SSFA, get_conv_layers and Head: host mirror of opencood/models/sub_modules/cia_ssd_utils.py:6-101 (CIA-SSD's
spatial-semantic feature aggregation neck and its IoU-aware head).

Parameter names, shapes and registration order follow the reference, so that its checkpoints load with strict=True and
`state_dict()` lists its keys in its order.

SSFA follows ConvNeXtBlock.forward's rule.  On a device tensor outside the gradient path (`grad_path` false) and with HEAL_SSFA_FUSED
on it runs every Conv + BatchNorm (eps 1e-3) folded (heal_amd.derived) on this library's operators:
  * the 3x3 layers on heal_conv3x3 (`ZeroPad2d(1)` + a padding-0 convolution is a padding-1 convolution; bottom_up_block_1 opens with
    a stride-2 layer), trans_0 / trans_1 on heal_conv1x1, each with its ReLU in the epilogue;
  * deconv_block_0 and deconv_block_1 as ONE heal_deconv3x3_s2 launch: the two folded weights concatenated along Cout (256 -> 256),
    one read of x_trans_1, ReLU fused, x_trans_0 added after the ReLU to the first 128 channels;
  * conv_0 / conv_1 on the two channel halves of that map;
  * w_0 / w_1, the softmax over the two weights and the weighted sum as ONE heal_ssfa_blend pass.
On CPU tensors, under autograd, with BatchNorm in training mode, for a shape the transposed convolution refuses or with
HEAL_SSFA_FUSED=0 it runs the reference's composition line by line on the same parameters.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from heal_amd.derived import derived
from heal_amd.opencood.models.sub_modules.bev_blocks import conv_bias_act, fold_bn, grad_path


def get_conv_layers(conv_name, in_channels, out_channels, n_layers, kernel_size, stride, padding, relu_last=True,
                    sequential=True, **kwargs):
    """cia_ssd_utils.py:58-74: n_layers x (conv without bias, BatchNorm2d(eps 1e-3, momentum 0.01), ReLU); the last ReLU only with
    relu_last.  kernel_size, stride, padding and every keyword are lists with one entry per layer."""
    seq = []
    for i in range(n_layers):
        seq.append(getattr(nn, conv_name)(in_channels, out_channels, kernel_size[i], stride=stride[i], padding=padding[i],
                                          bias=False, **{k: v[i] for k, v in kwargs.items()}))
        seq.append(nn.BatchNorm2d(out_channels, eps=1e-3, momentum=0.01))
        if i < n_layers - 1 or relu_last:
            seq.append(nn.ReLU())
        in_channels = out_channels
    return nn.Sequential(*seq) if sequential else seq


def _folded_stack(seq, x):
    """A Sequential of get_conv_layers (Conv2d only, optionally behind a ZeroPad2d(1)) with every BatchNorm folded and every ReLU in
    its convolution's epilogue."""
    from heal_amd import ops
    mods, i, pad = list(seq), 0, None
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ZeroPad2d):
            pad, i = tuple(m.padding), i + 1
            continue
        conv, bn = m, mods[i + 1]
        relu = i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
        padding = conv.padding
        if pad is not None:                          # ZeroPad2d(p) + padding 0 == padding p
            if len(set(pad)) != 1 or conv.padding != (0, 0):
                raise NotImplementedError("SSFA: a ZeroPad2d in front of a padded convolution")
            padding, pad = (pad[0], pad[0]), None
        w, b = fold_bn(conv, bn)
        if conv.kernel_size == (1, 1) and not ops.conv1x1_supported(conv.in_channels, conv.out_channels,
                                                                    int(x.shape[2] * x.shape[3])):
            x = F.conv2d(x, w, b)                    # a map too small for heal_conv1x1 (rows that are no 16-byte pieces)
            x = F.relu(x) if relu else x
        else:
            x = conv_bias_act(x, w, b, conv.stride, padding, conv.dilation, conv.groups, relu)
        i += 3 if relu else 2
    return x


class SSFA(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._num_input_features = args['feature_num']  # 128
        seq = [nn.ZeroPad2d(1)]
        seq += get_conv_layers('Conv2d', 128, 128, n_layers=3, kernel_size=[3, 3, 3], stride=[1, 1, 1], padding=[0, 1, 1],
                               sequential=False)
        self.bottom_up_block_0 = nn.Sequential(*seq)
        self.bottom_up_block_1 = get_conv_layers('Conv2d', 128, 256, n_layers=3, kernel_size=[3, 3, 3], stride=[2, 1, 1],
                                                 padding=[1, 1, 1])
        self.trans_0 = get_conv_layers('Conv2d', 128, 128, n_layers=1, kernel_size=[1], stride=[1], padding=[0])
        self.trans_1 = get_conv_layers('Conv2d', 256, 256, n_layers=1, kernel_size=[1], stride=[1], padding=[0])
        self.deconv_block_0 = get_conv_layers('ConvTranspose2d', 256, 128, n_layers=1, kernel_size=[3], stride=[2], padding=[1],
                                              output_padding=[1])
        self.deconv_block_1 = get_conv_layers('ConvTranspose2d', 256, 128, n_layers=1, kernel_size=[3], stride=[2], padding=[1],
                                              output_padding=[1])
        self.conv_0 = get_conv_layers('Conv2d', 128, 128, n_layers=1, kernel_size=[3], stride=[1], padding=[1])
        self.conv_1 = get_conv_layers('Conv2d', 128, 128, n_layers=1, kernel_size=[3], stride=[1], padding=[1])
        self.w_0 = get_conv_layers('Conv2d', 128, 1, n_layers=1, kernel_size=[1], stride=[1], padding=[0], relu_last=False)
        self.w_1 = get_conv_layers('Conv2d', 128, 1, n_layers=1, kernel_size=[1], stride=[1], padding=[0], relu_last=False)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight, gain=1)
                if hasattr(m, "bias") and m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _deconv_pair(self):
        """(fragments, bias) of deconv_block_0 and deconv_block_1 as one 256 -> 256 transposed convolution, BatchNorm folded."""
        from heal_amd import ops
        (c0, n0), (c1, n1) = self.deconv_block_0[:2], self.deconv_block_1[:2]
        sources = [t for c, n in ((c0, n0), (c1, n1)) for t in (c.weight, n.weight, n.bias, n.running_mean, n.running_var)]

        def build():
            (w0, b0), (w1, b1) = fold_bn(c0, n0, transposed=True), fold_bn(c1, n1, transposed=True)
            return ops._deconv3x3_s2_pack(torch.cat([w0, w1], dim=1)), torch.cat([b0, b1]).contiguous()
        return derived("ssfa_deconv_pair", sources, build)

    def _fused_ok(self, x):
        from heal_amd import ops
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4) or grad_path(x, self):
            return False
        H, W = int(x.shape[2]), int(x.shape[3])          # x_1 is (H + 1) // 2: the deblocks give back H x W only for even sizes
        return (H % 2 == 0 and W % 2 == 0 and ops.ssfa_fused_enabled()
                and ops.deconv3x3_s2_supported(256, 256, H // 2, W // 2))

    def forward(self, x):
        if self._fused_ok(x):
            return self._forward_fused(x)
        x_0 = self.bottom_up_block_0(x)
        x_1 = self.bottom_up_block_1(x_0)
        x_trans_0 = self.trans_0(x_0)
        x_trans_1 = self.trans_1(x_1)
        x_middle_0 = self.deconv_block_0(x_trans_1) + x_trans_0
        x_middle_1 = self.deconv_block_1(x_trans_1)
        x_output_0 = self.conv_0(x_middle_0)
        x_output_1 = self.conv_1(x_middle_1)
        x_weight_0 = self.w_0(x_output_0)
        x_weight_1 = self.w_1(x_output_1)
        x_weight = torch.softmax(torch.cat([x_weight_0, x_weight_1], dim=1), dim=1)
        x_output = x_output_0 * x_weight[:, 0:1, :, :] + x_output_1 * x_weight[:, 1:, :, :]
        return x_output.contiguous()

    def _forward_fused(self, x):
        from heal_amd import ops
        x_0 = _folded_stack(self.bottom_up_block_0, x)
        x_1 = _folded_stack(self.bottom_up_block_1, x_0)
        x_trans_0 = _folded_stack(self.trans_0, x_0)
        x_trans_1 = _folded_stack(self.trans_1, x_1)
        frag, bias = self._deconv_pair()
        x_middle = ops.deconv3x3_s2(x_trans_1, frag, bias, relu=True, residual=x_trans_0)     # [x_middle_0 | x_middle_1]
        x_output_0 = _folded_stack(self.conv_0, x_middle[:, :128])
        x_output_1 = _folded_stack(self.conv_1, x_middle[:, 128:])
        (wa, ba), (wb, bb) = fold_bn(*self.w_0[:2]), fold_bn(*self.w_1[:2])
        if ops.ssfa_blend_supported(128, int(x_output_0.shape[2] * x_output_0.shape[3])):
            return ops.ssfa_blend(x_output_0, x_output_1, wa, ba, wb, bb)
        sa = (x_output_0 * wa.view(1, -1, 1, 1)).sum(1, keepdim=True) + ba      # a map whose rows are not 16-byte pieces
        pa = torch.sigmoid(sa - ((x_output_1 * wb.view(1, -1, 1, 1)).sum(1, keepdim=True) + bb))
        return x_output_0 * pa + x_output_1 * (1 - pa)


class Head(nn.Module):
    """cia_ssd_utils.py:77-101: 1x1 box, class and IoU heads (and a direction head with use_dir).  Without use_dir `dir_preds` is
    the reference's zero tensor [N, 1, 2]."""

    def __init__(self, num_input, num_pred, num_cls, num_iou=2, use_dir=False, num_dir=1):
        super().__init__()
        self.use_dir = use_dir
        self.conv_box = nn.Conv2d(num_input, num_pred, 1)   # 14 of 128
        self.conv_cls = nn.Conv2d(num_input, num_cls, 1)    # 2 of 128
        self.conv_iou = nn.Conv2d(num_input, num_iou, 1, bias=False)
        if self.use_dir:
            self.conv_dir = nn.Conv2d(num_input, num_dir, 1)  # 4 of 128

    def forward(self, x):
        from heal_amd.opencood.models.point_pillar import head
        box_preds = head(self.conv_box, x)
        ret_dict = {"reg_preds": box_preds, "cls_preds": head(self.conv_cls, x)}
        if self.use_dir:
            ret_dict["dir_preds"] = head(self.conv_dir, x)
        else:
            ret_dict["dir_preds"] = torch.zeros((len(box_preds), 1, 2), device=box_preds.device)
        ret_dict["iou_preds"] = head(self.conv_iou, x)
        return ret_dict
