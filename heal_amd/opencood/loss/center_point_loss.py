"""Criterion of the anchor-free centre head (reference: opencood/loss/center_point_loss.py:188-470, with gaussian_radius
:526-555, draw_heatmap_gaussian :493-522, gaussian_focal_loss :662-684 and l1_loss :686-701).

The reference copies the boxes to the host, assigns the targets object by object in a Python loop (a numpy Gaussian per object,
copied to the device), and composes the Gaussian focal term and the L1 term from separate operators.  Here, for CUDA fp32 maps
whose size is the feature map of the target assigner's range (ops.center_loss_supported; HEAL_LOSS_FUSED=0 turns it off), one
call of heal_center_loss assigns the targets and writes both terms and their gradients; `loss_dict` is
filled from one device-to-host copy.  Otherwise the torch composition below runs: the same arithmetic, operation by operation,
vectorised over the objects instead of looped (assign_targets), on whatever device the maps live.
Same constructor `args`, `forward(output_dict, target_dict, suffix="")` (the `_single` keys included), `loss_dict` keys and
`logging`.  The unused FastFocalLoss / RegLoss of the reference file are not mirrored."""
import numpy as np
import torch
import torch.nn as nn

from heal_amd import ops


def clip_sigmoid(x, eps=1e-4):
    """center_point_loss.py:100-113."""
    return torch.clamp(torch.sigmoid(x), min=eps, max=1 - eps)


def gaussian_focal_loss(pred, gaussian_target, alpha=2.0, gamma=4.0):
    """center_point_loss.py:662-684, element-wise (the reduction is the caller's)."""
    eps = 1e-12
    pos_weights = gaussian_target.eq(1)
    neg_weights = (1 - gaussian_target).pow(gamma)
    pos_loss = -(pred + eps).log() * (1 - pred).pow(alpha) * pos_weights
    neg_loss = -(1 - pred + eps).log() * pred.pow(alpha) * neg_weights
    return pos_loss + neg_loss


def gaussian_radius(det_size, min_overlap=0.5):
    """center_point_loss.py:526-555 on tensors of any shape."""
    height, width = det_size
    a1 = 1
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    sq1 = torch.sqrt(b1 ** 2 - 4 * a1 * c1)
    r1 = (b1 + sq1) / (2 * a1)
    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    sq2 = torch.sqrt(b2 ** 2 - 4 * a2 * c2)
    r2 = (b2 + sq2) / (2 * a2)
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    sq3 = torch.sqrt(b3 ** 2 - 4 * a3 * c3)
    r3 = (b3 + sq3) / (2 * a3)
    return torch.minimum(torch.minimum(r1, r2), r3)


class CenterPointLoss(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.cls_weight = args['cls_weight']
        self.loc_weight = args['loc_weight']
        self.code_weights = args['code_weights']
        self.target_cfg = args['target_assigner_config']
        self.lidar_range = self.target_cfg['cav_lidar_range']
        self.voxel_size = self.target_cfg['voxel_size']
        self.loss_dict = {}

    def feature_map_size(self):
        """(W, H) as get_targets_single derives it (:393-396)."""
        grid = (np.array(self.lidar_range[3:6]) - np.array(self.lidar_range[0:3])) / np.array(self.voxel_size)
        grid = np.round(grid).astype(np.int64)
        fm = grid[:2] // self.target_cfg['out_size_factor']
        return int(fm[0]), int(fm[1])

    def _kernel_cfg(self):
        return dict(cav_lidar_range=self.lidar_range, voxel_size=self.voxel_size,
                    out_size_factor=self.target_cfg['out_size_factor'], max_objs=self.target_cfg['max_objs'],
                    min_radius=self.target_cfg['min_radius'], gaussian_overlap=self.target_cfg['gaussian_overlap'],
                    code_weights=self.code_weights, cls_weight=self.cls_weight, loc_weight=self.loc_weight)

    def forward(self, output_dict, target_dict, suffix=""):
        bbox_preds = output_dict['bbox_preds{}'.format(suffix)]
        cls_preds = output_dict['cls_preds{}'.format(suffix)]
        boxes = target_dict['object_bbx_center{}'.format(suffix)]
        mask = target_dict['object_bbx_mask{}'.format(suffix)]
        if ops.center_loss_supported(cls_preds, bbox_preds, boxes, mask, self.lidar_range, self.voxel_size,
                                     self.target_cfg['out_size_factor'], self.target_cfg['max_objs']):
            terms = ops.center_loss_terms(cls_preds, bbox_preds, boxes, mask, **self._kernel_cfg())
            cls_loss, box_loss = terms[0], terms[1]
            host = np.asarray(terms.detach().tolist(), dtype=np.float32)        # ONE device-to-host copy
            self.loss_dict.update({'total_loss': float(host[0] + host[1]), 'reg_loss': float(host[1]),
                                   'cls_loss': float(host[0])})
            return cls_loss + box_loss
        targets = self.assign_targets(boxes.to(cls_preds.device), mask.to(cls_preds.device))
        cls_loss = self.get_cls_layer_loss(clip_sigmoid(cls_preds), targets['heatmaps'])
        box_loss = self.get_box_reg_layer_loss(bbox_preds.permute(0, 2, 3, 1).contiguous(),
                                               (targets['anno_boxes'], targets['inds'], targets['masks']))
        rpn_loss = cls_loss + box_loss
        self.loss_dict.update({'total_loss': rpn_loss.item(), 'reg_loss': box_loss.item(), 'cls_loss': cls_loss.item()})
        return rpn_loss

    def get_cls_layer_loss(self, pred_heatmaps, gt_heatmaps):
        """:275-284; the number of positive cells stays on the device (the reference reads it with .item())."""
        num_pos = gt_heatmaps.eq(1).float().sum()
        loss = gaussian_focal_loss(pred_heatmaps, gt_heatmaps).sum() / torch.clamp(num_pos, min=1)
        return loss * self.cls_weight

    def get_box_reg_layer_loss(self, bbox_preds, bbox_gt):
        """:314-332 with l1_loss / weight_reduce_loss (:584-613, :686-701).  bbox_preds [B, H, W, 8]."""
        target_box, inds, masks = bbox_gt
        num = masks.float().sum()
        pred = bbox_preds.view(bbox_preds.size(0), -1, bbox_preds.size(3))
        pred = pred.gather(1, inds.unsqueeze(2).expand(inds.size(0), inds.size(1), pred.size(2)))
        mask = masks.unsqueeze(2).expand_as(target_box).float()
        mask = mask * (~torch.isnan(target_box)).float()
        bbox_weights = mask * mask.new_tensor(self.code_weights)
        loc_loss = (torch.abs(pred - target_box) * bbox_weights).sum() / (num + 1e-4)
        return loc_loss * self.loc_weight

    def assign_targets(self, object_bbx_center, object_bbx_mask):
        """forward :217-225 + get_targets_single :385-470 without the host round trip and the per-object loop: the same fp32
        chain per object, as tensor operations over [B, K] (K = the slots in use, at most max_objs), and the heat map as the
        maximum over chunks of objects of the fp64 Gaussian rounded to fp32.
        -> {'heatmaps' [B, 1, H, W], 'anno_boxes' [B, max_objs, 8], 'inds' [B, max_objs] int64, 'masks' [B, max_objs] uint8}."""
        cfg = self.target_cfg
        max_objs, factor = int(cfg['max_objs']), cfg['out_size_factor']
        pc_range, voxel_size = self.lidar_range, self.voxel_size
        W, H = self.feature_map_size()
        boxes = object_bbx_center.to(torch.float32)            # the reference copies into a float32 array (:222)
        dev = boxes.device
        B, Mmax = int(boxes.shape[0]), int(boxes.shape[1])
        n_b = object_bbx_mask.sum(dim=1).to(torch.int64)       # int(bbox_mask[k].sum()): the FIRST n_b rows are used
        K = min(Mmax, max_objs)
        t = boxes[:, :K]
        used = torch.arange(K, device=dev)[None, :] < n_b[:, None]
        coor_x = (t[..., 0] - pc_range[0]) / voxel_size[0] / factor
        coor_y = (t[..., 1] - pc_range[1]) / voxel_size[1] / factor
        coor_z = (t[..., 2] - pc_range[2]) / voxel_size[2] / factor
        h = t[..., 3] / voxel_size[0] / factor
        w = t[..., 4] / voxel_size[1] / factor
        l = t[..., 5] / voxel_size[2] / factor
        rot = t[..., 6]
        sized = used & (h > 0) & (w > 0)
        one = torch.ones_like(h)
        radius = gaussian_radius((torch.where(sized, h, one), torch.where(sized, w, one)), min_overlap=cfg['gaussian_overlap'])
        radius = torch.clamp(torch.trunc(radius), min=cfg['min_radius']).to(torch.int64)         # max(min_radius, int(radius))
        cx_f, cy_f = torch.trunc(coor_x), torch.trunc(coor_y)                                    # .to(torch.int32): toward zero
        kept = sized & (cx_f >= 0) & (cx_f < W) & (cy_f >= 0) & (cy_f < H)
        cx = torch.where(kept, cx_f, torch.zeros_like(cx_f)).to(torch.int64)
        cy = torch.where(kept, cy_f, torch.zeros_like(cy_f)).to(torch.int64)
        anno = torch.stack([coor_x - cx.to(torch.float32), coor_y - cy.to(torch.float32), coor_z, h, w, l,
                            torch.sin(rot), torch.cos(rot)], dim=-1)
        anno = torch.where(kept[..., None], anno, torch.zeros_like(anno))
        anno_boxes = torch.zeros((B, max_objs, 8), dtype=torch.float32, device=dev)
        inds = torch.zeros((B, max_objs), dtype=torch.int64, device=dev)
        masks = torch.zeros((B, max_objs), dtype=torch.uint8, device=dev)
        anno_boxes[:, :K] = anno
        inds[:, :K] = torch.where(kept, cy * W + cx, torch.zeros_like(cx))
        masks[:, :K] = kept.to(torch.uint8)
        # draw_heatmap_gaussian: the window |dx|, |dy| <= radius clipped to the map, values of gaussian_2d in float64 rounded
        # to float32, combined by maximum.  (gaussian_2d's eps * max cut never triggers: a window's corner is >= exp(-9).)
        heat = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
        xs = torch.arange(W, device=dev, dtype=torch.int64)
        ys = torch.arange(H, device=dev, dtype=torch.int64)
        live = int(kept.any(dim=0).nonzero().max().item()) + 1 if bool(kept.any()) else 0
        for k0 in range(0, live, 32):
            sl = slice(k0, min(k0 + 32, live))
            r = radius[:, sl, None]
            dx = xs[None, None, :] - cx[:, sl, None]                                            # [B, k, W]
            dy = ys[None, None, :] - cy[:, sl, None]                                            # [B, k, H]
            in_x = (dx.abs() <= r) & kept[:, sl, None]
            in_y = dy.abs() <= r
            sigma = (2 * r + 1).to(torch.float64) / 6
            d2 = (dx * dx)[:, :, None, :] + (dy * dy)[:, :, :, None]                            # [B, k, H, W]
            g = torch.exp(-d2.to(torch.float64) / (2 * sigma * sigma)[..., None]).to(torch.float32)
            g = torch.where(in_x[:, :, None, :] & in_y[:, :, :, None], g, torch.zeros_like(g))
            heat = torch.maximum(heat, g.max(dim=1)[0])
        return {'heatmaps': heat[:, None], 'anno_boxes': anno_boxes, 'inds': inds, 'masks': masks}

    def logging(self, epoch, batch_id, batch_len, writer=None, suffix=""):
        """center_point_loss.py:244-272."""
        total_loss = self.loss_dict.get('total_loss', 0)
        reg_loss = self.loss_dict.get('reg_loss', 0)
        cls_loss = self.loss_dict.get('cls_loss', 0)
        print("[epoch %d][%d/%d]%s, || Loss: %.4f || Conf Loss: %.4f"
              " || Loc Loss: %.4f" % (epoch, batch_id + 1, batch_len, suffix, total_loss, cls_loss, reg_loss))
        if writer is not None:
            writer.add_scalar('Regression_loss', reg_loss, epoch * batch_len + batch_id)
            writer.add_scalar('Confidence_loss', cls_loss, epoch * batch_len + batch_id)
