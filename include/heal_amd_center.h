/* heal_amd_center.h -- the anchor-free centre head (CenterPoint): criterion with target assignment, box map and decode + NMS.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  Same conventions as include/heal_amd.h: fp32 NCHW device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no floating-point atomics, workspaces that need not be initialised, *_workspace / *_supported are host
 * arithmetic and return 0 for a shape out of range.  The library is built with -ffp-contract=off: the fp32 chains below are the
 * reference's, operation by operation.
 *
 * heal_center_loss = CenterPointLoss.forward (opencood/loss/center_point_loss.py:205-242), target assignment included:
 *   targets   get_targets_single :385-470, gaussian_radius :526-555, draw_heatmap_gaussian :493-522, gaussian_2d :473-489
 *   cls term  clip_sigmoid :100-113, gaussian_focal_loss :662-684, get_cls_layer_loss :275-284
 *   reg term  get_box_reg_layer_loss :314-332, l1_loss :686-701, weight_reduce_loss :584-613
 * Target assignment, per sample b (map [H, W], W along x):
 *   n_b = int(sum(mask[b])); the rows k < min(n_b, max_objs) are used -- the FIRST n_b rows, wherever the ones of the mask are
 *   (:221-224).  A row with h <= 0 or w <= 0 is skipped (:427; that is also the zero padding up to the batch's max_gt).
 *   fp32, in this order:  coor = ((v - range) / voxel) / out_size_factor for x, y, z;  h = (b3 / vx) / f, w = (b4 / vy) / f,
 *   l = (b5 / vz) / f  (:419-424: l and coor_z are divided by voxel_size[2]);
 *   radius = max(min_radius, int(min(r1, r2, r3))) with the three roots of :538-554 exactly as written;
 *   (x, y) = coor_x, coor_y truncated toward zero (:436): a centre in (-1, 0) lands in cell 0 and is kept; an object outside
 *   [0, W) x [0, H) is skipped and its slot k stays zero (:440-442);
 *   inds[k] = y * W + x, masks[k] = 1 at slot k (not compacted);
 *   anno_boxes[k] = (coor_x - x, coor_y - y, coor_z, h, w, l, sin(rot), cos(rot)).
 *   heatmap[pixel] = max over the kept objects with |dx|, |dy| <= radius of float32(exp(-(dx^2 + dy^2) / (2 sigma^2))), evaluated
 *   in fp64 with sigma = (2 radius + 1) / 6.  (gaussian_2d's `h < eps * h.max()` cut never triggers: the smallest value of a
 *   window is exp(-2 r^2 / (2 sigma^2)) >= exp(-9), far above 2.2e-16; it is not implemented.)
 * Classification term: p = clamp(sigmoid(x), 1e-4, 1 - 1e-4) in fp32, pos = (heat == 1), neg_w = (1 - heat)^4,
 *   sum(-log(p) (1 - p)^2 pos - log(1 - p) p^2 neg_w) / max(number of positive CELLS of the batch, 1) * cls_weight: two objects in
 *   one cell count once.  (The reference's `+ 1e-12` is absorbed in fp32: p and 1 - p are >= 1e-4.)  Gradient: exactly zero
 *   where the clamp is active, the analytic derivative (through 1 - p as the fp32 number the forward used) elsewhere.
 * Regression term: sum_k |pred[b, :, inds[k]] - anno_boxes[k]| masks[k] code_weights / (sum(masks) + 1e-4) * loc_weight.
 *   grad_bbox is zero off the kept inds; where several kept slots share one pixel it is the sum of their contributions in slot
 *   order.  The pixel pass finds the slots of a pixel itself, so no scatter and no atomic is needed.
 *   NaN ground-truth boxes are out of scope (the reference itself returns NaN for them).
 * Reduction: per-pixel values in fp64 -> fixed xor tree over the 64 lanes of a tile -> one fp64 partial per tile and term -> one
 * block adds the partials in a fixed order in fp64.  Two launches on the same values are bit-equal.
 * Three launches: (1) one block per sample: n_b, per-object geometry, inds / masks / anno_boxes, the number of distinct positive
 * cells; (2) the pixel pass over 64-pixel tiles, every lane walking the sample's object table (in LDS) behind a tile-level
 * bounding-box cull: heat value, both terms, grad_cls, grad_bbox; (3) one block: the sums and the two normalisers.
 *
 * heal_center_boxes = generate_predicted_boxes (opencood/models/center_point_baseline.py:154-216, center_point.py:83-145).
 * heal_center_decode_nms = VoxelPostprocessor.post_process with 3-D reg_preds (voxel_postprocessor.py:305-306 and :308-405):
 * an anchor-free front end before the tail of heal_decode_nms (rank, re-decode of the top candidates, rotated NMS, range mask).
 */
#ifndef HEAL_AMD_CENTER_H
#define HEAL_AMD_CENTER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_CENTER_MAX_OBJS 512      /* largest max_objs of heal_center_loss (the object table of a sample lives in LDS)        */
#define HEAL_CENTER_MAX_BATCH 65535   /* largest B of heal_center_loss and heal_center_boxes (one grid row per sample)           */

/* heal_center_loss_supported (host only): 1 if heal_center_loss takes this problem, else 0 --
 *   1 <= B <= HEAL_CENTER_MAX_BATCH, 1 <= Mmax, 1 <= max_objs <= HEAL_CENTER_MAX_OBJS, out_size_factor >= 1, positive voxel sizes,
 *   H * W <= 2^31 - 64 and B * ceil(H * W / 64) < 2^31, and (H, W) equal to the reference's feature_map_size:
 *   grid = round((range[3:6] - range[0:3]) / voxel_size) (half to even, as numpy), W = grid[0] // factor, H = grid[1] // factor.  */
int heal_center_loss_supported(int B, int Mmax, int H, int W, const double* cav_lidar_range, const double* voxel_size,
                               int out_size_factor, int max_objs);

/* bytes of workspace of heal_center_loss; 0 for a shape out of range */
size_t heal_center_loss_workspace(int B, int H, int W, int max_objs);

/* heal_center_loss: both terms and their gradients in one call.
 *   cls_preds [B, 1, H, W], bbox_preds [B, 8, H, W] fp32; object_bbx_center [B, Mmax, 7] fp32 and object_bbx_mask [B, Mmax] int32,
 *   both on the device.  Host scalars: cav_lidar_range[6], voxel_size[3], code_weights[8] (doubles, rounded to fp32 where the
 *   reference's tensor arithmetic does), out_size_factor, max_objs, min_radius, gaussian_overlap, cls_weight, loc_weight.
 *   terms[2] <- (cls, reg).  grad_cls [B, 1, H, W], grad_bbox [B, 8, H, W] <- d (term) / d (map), every element written; either
 *   may be NULL.  Optional outputs for inspection (NULL on the training path; the heat values then never reach memory):
 *   heatmap [B, 1, H, W] fp32, anno_boxes [B, max_objs, 8] fp32, inds [B, max_objs] int64, masks [B, max_objs] uint8.
 *   ws: heal_center_loss_workspace bytes, 256-B aligned, need not be initialised.  Fails where heal_center_loss_supported is 0. */
int heal_center_loss(const float* cls_preds, const float* bbox_preds, const float* object_bbx_center,
                     const int32_t* object_bbx_mask, int B, int Mmax, int H, int W, const double* cav_lidar_range,
                     const double* voxel_size, int out_size_factor, int max_objs, int min_radius, double gaussian_overlap,
                     const double* code_weights, double cls_weight, double loc_weight, float* terms, float* grad_cls,
                     float* grad_bbox, float* heatmap, float* anno_boxes, int64_t* inds, uint8_t* masks, void* ws,
                     size_t ws_bytes, void* stream);

/* heal_center_boxes: bbox_preds [B, 8, H, W] -> reg_preds [B, H * W, 7] = (x, y, z, h, w, l, atan2(sin, cos)), one streaming
 *   launch, in the reference's fp32 order: x = ((col + c0) * factor) * vx + range[0], y = ((row + c1) * factor) * vy + range[1],
 *   z = (c2 * factor) * vz + range[2], h = (c3 * factor) * vx, w = (c4 * factor) * vy, l = (c5 * factor) * vz, yaw = atan2(c6, c7).
 *   No gradient flows through it: the criterion reads bbox_preds, reg_preds feeds the post-processor only.
 *   1 <= B <= HEAL_CENTER_MAX_BATCH, H * W <= 2^31 - 256 and B * H * W * 8 < 2^63.                                              */
int heal_center_boxes(const float* bbox_preds, int B, int H, int W, const double* cav_lidar_range, const double* voxel_size,
                      int out_size_factor, float* reg_preds, void* stream);

/* heal_center_decode_nms: cls [1, 1, H, W] scores and boxes [H * W, 7] (the 3-D reg_preds, used as they are: no anchor table, no
 *   delta decode) -> score threshold, optional direction correction from dir [1, num_bins, H, W] (NULL: none), 'hwl' corners,
 *   projection by tfm_host (4 x 4, row-major), size / z filters, top-nms_top rotated NMS, range mask; outputs and limits as
 *   heal_decode_nms.  One box per cell (the reference's own reshape only lines up for anchor_number 1).
 *   ws: heal_decode_nms_workspace(H * W, nms_top) bytes.                                                                       */
int heal_center_decode_nms(const float* cls, const float* boxes, const float* dir, int H, int W, int num_bins, float score_thr,
                           float dir_offset, float nms_thr, int nms_top, const float* tfm_host, const float* gt_range_host,
                           float* out_corners, float* out_scores, int32_t* out_count, int max_out, void* ws, size_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
