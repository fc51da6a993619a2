"""AP evaluation (reference: opencood/utils/eval_utils.py -- :14-37 voc_ap, :40-91 caluclate_tp_fp, :95-137 calculate_ap,
:140-164 eval_final_results): the reference's names, signatures and result_stat dictionary, so that tools/inference*.py scores a
run unchanged.  The per-frame step -- pairwise IoU and the greedy TP / FP match -- runs on the device (heal_eval_match: the IoU
arithmetic of the NMS that produced the boxes); no polygons, no shapely.

  caluclate_tp_fp         the reference's entry: one threshold, one launch, one host read
  caluclate_tp_fp_multi   every threshold of a frame in one launch, one host read
  DeviceResultStat        accumulates a whole run on the device: .add() never reads on the host (legal inside a graph capture),
                          .result_stat() reads once and returns the reference's dictionary

HEAL_EVAL_FUSED=0, or a frame beyond the kernel's limits (1024 detections, 256 ground-truth boxes, 8 thresholds), takes the
fallback: one heal_quad_iou launch for the whole matrix, then the reference's loop restated in numpy (_greedy_match).  Both paths
give the same bits.  Equal scores go by ascending detection index (np.argsort's order on ties is implementation-defined in the
reference); a NaN IoU (zero-area pair) counts as 0."""
import os

import numpy as np
import torch

from heal_amd import ops, switches
from heal_amd.opencood.hypes_yaml import yaml_utils

DEFAULT_THRESHOLDS = (0.3, 0.5, 0.7)


def voc_ap(rec, prec):
    """eval_utils.py:14-37: VOC 2010 average precision; rec / prec are lists and are extended in place like the reference's."""
    rec.insert(0, 0.0)
    rec.append(1.0)
    mrec = rec[:]
    prec.insert(0, 0.0)
    prec.append(0.0)
    mpre = prec[:]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap, mrec, mpre


def _greedy_match(iou, thresholds, score=None):
    """The reference loop (eval_utils.py:67-87) on a precomputed IoU matrix iou [n,m] (rows in detection order), for every
    threshold: -> (order [n], tp [T,n] uint8, gt_index [T,n] int32), rows of tp / gt_index in descending-score order (equal
    scores by ascending index; score None: the rows are already in that order).  A detection is FP when no ground-truth box is
    left or the maximum IoU over the boxes still unmatched is < float32(threshold); otherwise TP, and the first maximum in
    original ground-truth order is removed.  NaN counts as 0."""
    iou = np.asarray(iou, np.float32)
    n, m = iou.shape
    iou = np.where(np.isnan(iou), np.float32(0), iou)
    order = np.arange(n) if score is None else np.argsort(-np.asarray(score, np.float32), kind="stable")
    tp = np.zeros((len(thresholds), n), np.uint8)
    gi = np.full((len(thresholds), n), -1, np.int32)
    for t, thr in enumerate(thresholds):
        thr = np.float32(thr)
        left = list(range(m))                                  # original indices of the boxes still unmatched
        for r, i in enumerate(order):
            if not left:
                break
            ious = iou[i, left]
            if ious.max() < thr:
                continue
            tp[t, r] = 1
            gi[t, r] = left.pop(int(np.argmax(ious)))
    return order.astype(np.int32), tp, gi


def fused_enabled():
    return switches.on("HEAL_EVAL_FUSED")


def _on_device(t, dtype=torch.float32):
    """Host tensors / arrays are copied to the current device: the library has no CPU arithmetic."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    t = t.detach()
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.to(dtype)


def _footprints(boxes):
    return boxes[:, :4, :2].contiguous()


def _match_frame(det_boxes, det_score, gt_boxes, thresholds):
    """-> (score_sorted list, tp [T,n] numpy uint8) of one frame, by the fused kernel or the fallback."""
    det, score, gt = _on_device(det_boxes), _on_device(det_score).reshape(-1), _on_device(gt_boxes)
    n, m, T = int(det.shape[0]), int(gt.shape[0]), len(thresholds)
    if n == 0:
        return [], np.zeros((T, 0), np.uint8)
    if fused_enabled() and ops.eval_match_supported(n, m, T):
        _, tp, sorted_score = ops.eval_match(det, score, gt, thresholds)
        packed = torch.cat([sorted_score.view(torch.uint8), tp.reshape(-1)]).cpu().numpy()      # the one host read
        return packed[:4 * n].view(np.float32).tolist(), packed[4 * n:].reshape(T, n)
    if m == 0:
        iou, s = np.zeros((n, 0), np.float32), score.cpu().numpy()
    else:
        iou_dev = ops.quad_iou(_footprints(det), _footprints(gt))
        packed = torch.cat([score, iou_dev.reshape(-1)]).cpu().numpy()
        s, iou = packed[:n], packed[n:].reshape(n, m)
    order, tp, _ = _greedy_match(iou, thresholds, s)
    return s[order].tolist(), tp


def _append(result_stat, key, score, tp, gt):
    stat = result_stat[key]
    if score is not None:
        stat['score'] += score
        stat['fp'] += (1 - tp.astype(np.int64)).tolist()
        stat['tp'] += tp.astype(np.int64).tolist()
    stat['gt'] += gt


def caluclate_tp_fp(det_boxes, det_score, gt_boxes, result_stat, iou_thresh):
    """eval_utils.py:40-91 (the reference's spelling): add the frame's fp / tp / score lists, in descending-score order, and its
    ground-truth count to result_stat[iou_thresh].  det_boxes None: only gt is added."""
    gt = int(gt_boxes.shape[0])
    if det_boxes is None:
        return _append(result_stat, iou_thresh, None, None, gt)
    score, tp = _match_frame(det_boxes, det_score, gt_boxes, [iou_thresh])
    _append(result_stat, iou_thresh, score, tp[0], gt)


def caluclate_tp_fp_multi(det_boxes, det_score, gt_boxes, result_stat, iou_threshs=DEFAULT_THRESHOLDS):
    """caluclate_tp_fp for every threshold of `iou_threshs` (keys of result_stat) in one launch and one host read."""
    gt = int(gt_boxes.shape[0])
    if det_boxes is None:
        for thr in iou_threshs:
            _append(result_stat, thr, None, None, gt)
        return
    score, tp = _match_frame(det_boxes, det_score, gt_boxes, list(iou_threshs))
    for t, thr in enumerate(iou_threshs):
        _append(result_stat, thr, list(score), tp[t], gt)


def new_result_stat(thresholds=DEFAULT_THRESHOLDS):
    """The dictionary tools/inference.py:110-112 starts from."""
    return {thr: {'tp': [], 'fp': [], 'gt': 0, 'score': []} for thr in thresholds}


class DeviceResultStat:
    """result_stat of a whole run kept on the device: tp [T,capacity] u8, score [capacity] f32 (and the detection order), the
    row cursor, the ground-truth total and a sticky overflow word.  add() appends a frame with no host read -- it may be
    captured in a HIP graph, with n_dev / m_dev naming the live counts of the frame that is loaded at replay.  capacity is the
    number of detections of the whole run (frames x nms_top bounds it)."""

    def __init__(self, thresholds=DEFAULT_THRESHOLDS, capacity=1 << 16, device=None, want_gt_index=False):
        self.thresholds = tuple(thresholds)
        T = len(self.thresholds)
        if not 1 <= T <= ops.EVAL_MAX_THR:
            raise ValueError(f"DeviceResultStat: 1..{ops.EVAL_MAX_THR} thresholds, got {T}")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity = int(capacity)
        words = torch.zeros((3,), dtype=torch.int32, device=dev)
        self.buffers = {"order": torch.zeros((self.capacity,), dtype=torch.int32, device=dev),
                        "tp": torch.zeros((T, self.capacity), dtype=torch.uint8, device=dev),
                        "score": torch.zeros((self.capacity,), dtype=torch.float32, device=dev),
                        "cursor": words[0:1], "gt_total": words[1:2], "overflow": words[2:3]}
        if want_gt_index:
            self.buffers["gt_index"] = torch.full((T, self.capacity), -1, dtype=torch.int32, device=dev)
        self._words = words

    def add(self, det, score, gt, n_dev=None, m_dev=None):
        """Append one frame (device tensors; limits of heal_eval_match).  No host read, no synchronisation."""
        ops.eval_match(det, score.reshape(-1), gt, self.thresholds, n_dev=n_dev, m_dev=m_dev, sync=False, out=self.buffers)

    def result_stat(self):
        """One host read -> the reference's dictionary {thr: {'tp', 'fp', 'gt', 'score'}}, ready for eval_final_results.
        Raises if a frame did not fit (its rows were dropped)."""
        b = self.buffers
        packed = torch.cat([self._words.view(torch.uint8), b["score"].view(torch.uint8), b["tp"].reshape(-1)]).cpu().numpy()
        cursor, gt_total, overflow = (int(v) for v in packed[:12].view(np.int32))
        if overflow:
            raise RuntimeError(f"DeviceResultStat: a frame did not fit into the capacity of {self.capacity} detections "
                               f"({cursor} rows were stored); its results were dropped -- use a larger capacity")
        cap = self.capacity
        score = packed[12:12 + 4 * cap].view(np.float32)[:cursor]
        tp = packed[12 + 4 * cap:].reshape(len(self.thresholds), cap)[:, :cursor]
        stat = new_result_stat(self.thresholds)
        for t, thr in enumerate(self.thresholds):
            _append(stat, thr, score.tolist(), tp[t], gt_total)
        return stat


def calculate_ap(result_stat, iou):
    """eval_utils.py:95-137: cumulative tp / fp over all detections of the run in descending score -> (ap, mrec, mpre)."""
    stat = result_stat[iou]
    fp = np.array(stat['fp'])
    tp = np.array(stat['tp'])
    score = np.array(stat['score'])
    assert len(fp) == len(tp) and len(tp) == len(score)
    sorted_index = np.argsort(-score)
    fp = np.cumsum(fp[sorted_index]).tolist() if len(fp) else []
    tp = np.cumsum(tp[sorted_index]).tolist() if len(tp) else []
    gt_total = stat['gt']
    rec = [float(v) / gt_total for v in tp]
    prec = [float(t) / (f + t) for t, f in zip(tp, fp)]
    return voc_ap(rec[:], prec[:])


def eval_final_results(result_stat, save_path, infer_info=None):
    """eval_utils.py:140-164: AP at 0.3 / 0.5 / 0.7, written to eval.yaml (eval_<infer_info>.yaml) with the reference's keys."""
    ap_30, mrec_30, mpre_30 = calculate_ap(result_stat, 0.30)
    ap_50, mrec_50, mpre_50 = calculate_ap(result_stat, 0.50)
    ap_70, mrec_70, mpre_70 = calculate_ap(result_stat, 0.70)
    dump_dict = {'ap30': ap_30, 'ap_50': ap_50, 'ap_70': ap_70,
                 'mpre_50': mpre_50, 'mrec_50': mrec_50, 'mpre_70': mpre_70, 'mrec_70': mrec_70}
    name = 'eval.yaml' if infer_info is None else f'eval_{infer_info}.yaml'
    yaml_utils.save_yaml(dump_dict, os.path.join(save_path, name))
    print('The Average Precision at IOU 0.3 is %.2f, '
          'The Average Precision at IOU 0.5 is %.2f, '
          'The Average Precision at IOU 0.7 is %.2f' % (ap_30, ap_50, ap_70))
    return ap_30, ap_50, ap_70
