"""UncertaintyVoxelPostprocessor (reference: opencood/data_utils/post_processor/uncertainty_voxel_postprocessor.py:26-249):
the post-processor of CoAlign's first stage.  post_process (:116-249) returns the kept boxes' uncertainty next to boxes and
scores -- on the pooled decode + NMS kernel with its gather (ops.decode_nms_agents_unc) for CUDA fp32 maps, as tensor ops
otherwise; post_process_stage1 (:30-113) decodes every sample of a batch in its own frame for the offline box alignment."""
import numpy as np
import torch

from heal_amd import ops, switches
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
from heal_amd.opencood.utils import box_utils
from heal_amd.opencood.utils.common_utils import limit_period


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))


class UncertaintyVoxelPostprocessor(VoxelPostprocessor):
    def _correct_direction(self, boxes3d, dir_preds, mask):
        """:56-71 / :163-179 -- the direction classifier's bin put back into the yaw of the selected boxes, in place."""
        dir_args = self.params['dir_args']
        num_bins, dir_offset = dir_args['num_bins'], dir_args['dir_offset']
        labels = torch.max(dir_preds.permute(0, 2, 3, 1).contiguous().reshape(-1, num_bins)[mask], dim=-1)[1]
        period = 2 * np.pi / num_bins
        rot = limit_period(boxes3d[..., 6] - dir_offset, 0, period)
        boxes3d[..., 6] = rot + dir_offset + period * labels.to(dir_preds.dtype)
        boxes3d[..., 6] = limit_period(boxes3d[..., 6], 0.5, 2 * np.pi)

    def post_process_stage1(self, stage1_output_dict, anchor_box):
        """:30-113.  Every sample of the batch decoded in ITS OWN frame (no projection), a rotated NMS per sample, no size, z or
        range filter.  -> (corners [[n_b, 8, 3]], boxes [[n_b, 7]], uncertainty [[n_b, dim]]), one entry per sample, or three
        Nones when nothing in the batch passes the score threshold.  Runs offline (pose_graph_pre_calc.py): tensor ops and
        box_utils.nms_rotated."""
        cls_preds, reg_preds = stage1_output_dict['cls_preds'], stage1_output_dict['reg_preds']
        unc_preds = stage1_output_dict['unc_preds']
        dim = unc_preds.shape[1] // cls_preds.shape[1]
        prob = torch.sigmoid(cls_preds.permute(0, 2, 3, 1).contiguous())
        unc = unc_preds.permute(0, 2, 3, 1).contiguous().view(-1, dim)
        boxes = self.delta_to_boxes3d(reg_preds, _tensor(anchor_box)).view(-1, 7)
        mask = torch.gt(prob, self.params['target_args']['score_threshold'])
        counts = [int(m.sum()) for m in mask]
        mask = mask.view(-1)
        boxes3d, uncertainty, scores = boxes[mask], unc[mask], prob.view(-1)[mask]
        if len(boxes3d) == 0:
            return None, None, None
        if 'dir_preds' in stage1_output_dict:
            self._correct_direction(boxes3d, stage1_output_dict['dir_preds'], mask)
        boxes3d = boxes3d.detach()
        corners = box_utils.boxes_to_corners_3d(boxes3d, order=self.params['order'])
        out_corners, out_boxes, out_unc, at = [], [], [], 0
        for n in counts:
            keep = torch.from_numpy(box_utils.nms_rotated(corners[at:at + n], scores[at:at + n],
                                                          self.params['nms_thresh']).astype(np.int64)).to(corners.device)
            out_corners.append(corners[at:at + n][keep])
            out_boxes.append(boxes3d[at:at + n][keep])
            out_unc.append(uncertainty[at:at + n][keep])
            at += n
        return out_corners, out_boxes, out_unc

    def _unc_fused_ok(self, outs):
        """The kernel path: 1..8 cavs whose four (three) maps are CUDA fp32 with batch size 1 on ONE device, all with or all
        without a direction map, one uncertainty width -- and a gt_range whose z interval contains [-3, 1]: the reference masks
        x and y only (get_mask_for_boxes_within_range_torch), the kernel all three axes, which after the z filter of
        remove_bbx_abnormal_z is the same set exactly then.  HEAL_LATE_FUSED=0 keeps the tensor path."""
        r = self.params['gt_range']
        if not switches.on("HEAL_LATE_FUSED") or not 1 <= len(outs) <= ops.DECODE_MAX_AGENTS or r[2] > -3 or r[5] < 1:
            return False
        device, with_dir, dims = None, {o.get('dir_preds') is not None for o in outs}, set()
        if len(with_dir) != 1:
            return False
        for o in outs:
            if 'iou_preds' in o:
                return False
            for t in (o['cls_preds'], o['reg_preds'], o['unc_preds'], o.get('dir_preds')):
                if t is None:
                    continue
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == 1):
                    return False
                device = t.device if device is None else device
                if t.device != device:
                    return False
            dims.add(o['unc_preds'].shape[1] // o['cls_preds'].shape[1])
        return len(dims) == 1

    def post_process(self, data_dict, output_dict, return_uncertainty=False):
        """:116-249.  The cavs of data_dict that are in output_dict, in data_dict's order, each decoded and projected with its own
        transformation_matrix, pooled, filtered (size, z), ONE rotated NMS, range mask; the uncertainty of a box follows it
        through every step.  -> (pred_box3d [K,8,3], scores [K]) or, with return_uncertainty, (.., uncertainty [K,dim]); Nones
        when nothing survives."""
        if self.params['order'] != 'hwl':
            raise NotImplementedError("the decode kernel implements order 'hwl' (PointPillars / HEAL configs)")
        cavs = [(data_dict[cav_id], output_dict[cav_id]) for cav_id in data_dict if cav_id in output_dict]
        empty = (None, None, None) if return_uncertainty else (None, None)
        if not cavs:
            return empty
        outs = []
        for _, out in cavs:
            cls, reg, dirp = self._heads(out)
            o = {'cls_preds': cls, 'reg_preds': reg, 'unc_preds': out['unc_preds'] if 'unc_preds' in out else out['sm']}
            if dirp is not None:
                o['dir_preds'] = dirp
            outs.append(o)
        if self._unc_fused_ok(outs):
            pred, scores, unc = self._post_process_unc_agents([c for c, _ in cavs], outs)
        else:
            pred, scores, unc = self._post_process_unc_tensors([c for c, _ in cavs], outs)
        if pred is None:
            return empty
        return (pred, scores, unc) if return_uncertainty else (pred, scores)

    def _post_process_unc_agents(self, cavs, outs):
        """The cavs, in order, through ONE heal_decode_nms_agents_unc call."""
        dev = outs[0]['cls_preds'].device
        anchors = [self._anchors_f32(c['anchor_box'], dev, keep=ops.DECODE_MAX_AGENTS) for c in cavs]
        tfms = [c['transformation_matrix'] for c in cavs]
        on_dev = [isinstance(t, torch.Tensor) and t.is_cuda for t in tfms]
        if all(on_dev):
            tfms = torch.stack([t.to(torch.float32) for t in tfms])
        elif any(on_dev):
            tfms = [t.cpu() if d else t for t, d in zip(tfms, on_dev)]
        dir_args = self.params.get('dir_args', {'dir_offset': 0.7853, 'num_bins': 2})
        dirs = [o['dir_preds'] for o in outs] if 'dir_preds' in outs[0] else None
        return ops.decode_nms_agents_unc([o['cls_preds'] for o in outs], [o['reg_preds'] for o in outs], dirs, anchors,
                                         [o['unc_preds'] for o in outs], tfms, self.params['target_args']['score_threshold'],
                                         dir_args['dir_offset'], dir_args['num_bins'], self.params['nms_thresh'],
                                         self.params['gt_range'])

    def _post_process_unc_tensors(self, cavs, outs):
        """The reference's steps in its order, as tensor ops on the maps' device + box_utils.nms_rotated."""
        thr = self.params['target_args']['score_threshold']
        boxes3d_list, scores_list, unc_list = [], [], []
        for cav, out in zip(cavs, outs):
            dim = out['unc_preds'].shape[1] // out['cls_preds'].shape[1]
            prob = torch.sigmoid(out['cls_preds'].permute(0, 2, 3, 1)).reshape(1, -1)
            unc = out['unc_preds'].permute(0, 2, 3, 1).contiguous().view(out['unc_preds'].shape[0], -1, dim)
            box3d = self.delta_to_boxes3d(out['reg_preds'], _tensor(cav['anchor_box']))
            assert box3d.shape[0] == 1                      # batch size 1 at validation / test time (:155)
            mask = torch.gt(prob, thr).view(-1)
            boxes3d, scores, uncertainty = box3d[0][mask], prob[0][mask], unc[0][mask]
            if len(boxes3d) == 0:
                continue
            if 'dir_preds' in out:
                self._correct_direction(boxes3d, out['dir_preds'], mask)
            corners = box_utils.boxes_to_corners_3d(boxes3d, order=self.params['order'])
            tfm = _tensor(cav['transformation_matrix'])
            boxes3d_list.append(box_utils.project_box3d(corners, tfm.to(corners.device).float()))
            scores_list.append(scores)
            unc_list.append(uncertainty)
        if not boxes3d_list:
            return None, None, None
        pred, scores, unc = torch.vstack(boxes3d_list), torch.cat(scores_list), torch.vstack(unc_list)
        keep = torch.logical_and(box_utils.remove_large_pred_bbx(pred), box_utils.remove_bbx_abnormal_z(pred))
        pred, scores, unc = pred[keep], scores[keep], unc[keep]
        keep = torch.from_numpy(box_utils.nms_rotated(pred, scores, self.params['nms_thresh']).astype(np.int64)).to(pred.device)
        pred, scores, unc = pred[keep], scores[keep], unc[keep]
        mask = box_utils.get_mask_for_boxes_within_range_torch(pred, self.params['gt_range'])
        pred, scores, unc = pred[mask], scores[mask], unc[mask]
        if pred.shape[0] == 0:
            return None, None, None
        return pred, scores, unc
