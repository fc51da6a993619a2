/* heal_amd_unc.h -- CoAlign's first stage, the single-agent detector with a per-box pose uncertainty: the criterion with its KL
 * term in one pass, and the pooled decode + NMS that also returns the uncertainty of the kept boxes.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  Same conventions as include/heal_amd.h: fp32 NCHW device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no floating-point atomics, workspaces that need not be initialised, *_workspace / *_supported are host
 * arithmetic and return 0 for a shape out of range.  The library is built with -ffp-contract=off.
 *
 * heal_unc_loss = PointPillarUncertaintyLoss.forward (opencood/loss/point_pillar_uncertainty_loss.py:24-124) without the IoU
 * branch, gamma = 2, two direction bins: the four terms (cls, reg, unc, dir) and the gradients of the four head maps in one
 * streaming pass, laid out as heal_det_loss (a wave owns 64 consecutive pixels of one image, every channel row of a tile is one
 * 256-B access, the labels [N, H, W, A] and [N, H, W, 7A] are read in place, integer positive counts first, one partial per tile
 * and term, a one-block fp64 finish in a fixed order; repeated launches are bit-equal).
 *   cls, reg, dir  exactly heal_det_loss's arithmetic: on the same inputs terms[cls], terms[reg], terms[dir], grad_cls and
 *                  grad_dir are bit-equal to its results.  (The reference's reg term takes [..., :7] of the 8-wide tensors of
 *                  add_sin_difference_and_angle: the base criterion's seven encoded components.)
 *   unc            KLLoss.forward :262-293.  Per anchor the weight is w = (pos > 0) / max(#positives of the sample, 1) and s are
 *                  the anchor's `dim` channels of unc_preds (channel a * dim + d).
 *                    dim 2   xy_loss(x - x_t, s0) + xy_loss(y - y_t, s1)
 *                    dim 3   the same + angle_weight * angle_loss(yaw - yaw_t, s2), on the RAW yaw residuals (index 7 of the
 *                            8-wide tensors), not on the sin-difference encoding
 *                    dim 7   xy_loss on the components 0..5 and on the raw yaw difference, s of width 7
 *                  xy_loss     HEAL_UNC_L2: 0.5 (exp(-s) d^2 + s);  HEAL_UNC_L1: 0.5 exp(-s) |d| + s (the reference's kl_loss_l1
 *                              as written: s is outside the 0.5)
 *                  angle_loss  HEAL_UNC_L2, or HEAL_UNC_VON_MISES: log I0(k) - k c + lambda_V elu(s - s0), k = exp(-s),
 *                              c = |cos d| without a gradient to d under limit_period (the reference detaches it), else cos d.
 *                              d / ds = k (c - i1e(k) / i0e(k)) + lambda_V elu'(s - s0).
 *                  i0e, i1e are the Cephes Chebyshev expansions (two intervals split at 8) evaluated in fp32 with the
 *                  coefficients that reach fp32 (the float tables of ATen/native/Math.h for i1e, the same cut for i0e).
 *   grad_reg       the reg term's gradient plus the unc term's (through the x, y, ... differences and through the raw yaw, except
 *                  for von Mises under limit_period), in one store.
 * Deviations from the reference, all in the unc term:
 *   * log I0(k) is evaluated as log(i0e(k)) + k, the whole angular value as log(i0e(k)) + k (1 - c).  The reference's
 *     log(i0e(k) exp(k)) overflows to inf above k ~ 88 (s < -4.48); this form is finite up to k ~ 3e38 and equal to rounding
 *     wherever the reference's is finite.
 *   * An anchor with w == 0 contributes exactly 0 to every term and gets exactly 0 gradients whatever its s (heal_det_loss's
 *     convention; the composition gives inf * 0 = NaN for an extreme s there).
 *   * A NaN target counts as "equal to the input" in the unc term only (KLLoss.forward :266).  The reference's own reg term is
 *     NaN for such a target, and so is this one's: the case is documented, not supported.
 *
 * heal_decode_nms_agents_unc = UncertaintyVoxelPostprocessor.post_process (uncertainty_voxel_postprocessor.py:116-249):
 * heal_decode_nms_agents with the pooled anchor index of every kept box and the uncertainty channels gathered at it.
 */
#ifndef HEAL_AMD_UNC_H
#define HEAL_AMD_UNC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_UNC_L2 0          /* xy_loss_type / angle_loss_type "l2"   */
#define HEAL_UNC_L1 1          /* xy_loss_type "l1"                     */
#define HEAL_UNC_VON_MISES 1   /* angle_loss_type "von-mise"            */

/* heal_unc_loss_supported (host only): 1 if heal_unc_loss takes this configuration, else 0 -- dim in {2, 3, 7},
 *   1 <= anchors <= HEAL_LOSS_MAX_ANCHORS, xy_type in {L2, L1}, angle_type in {L2, VON_MISES}, and anchors == 2 with a direction
 *   map (the composition's own direction term is only defined there).                                                          */
int heal_unc_loss_supported(int anchors, int dim, int xy_type, int angle_type, int with_dir);

/* bytes of workspace of heal_unc_loss; 0 for a shape out of range (the limits of heal_det_loss_workspace) */
size_t heal_unc_loss_workspace(int n, int anchors, int H, int W);

/* heal_unc_loss: cls_preds [N, A, H, W], reg_preds [N, 7A, H, W], unc_preds [N, dim * A, H, W], dir_preds [N, 2A, H, W] or NULL,
 *   fp32; pos_equal_one, neg_equal_one [N, H, W, A] and targets [N, H, W, 7A], float32 or float64 (labels_f64).
 *   terms[4] <- (cls, reg, unc, dir), each x its weight / N (dir: 0 without a direction map).  grad_cls, grad_reg, grad_unc,
 *   grad_dir <- d (sum of the terms) / d (map), every element written; any of them may be NULL, and with all four NULL the
 *   kernels only read.  anchor_yaw[anchors] in radians (needed with dir_preds).  angle_weight, lambda_V, s0 and limit_period are
 *   read where the configuration uses them.  ws: heal_unc_loss_workspace bytes, 256-B aligned, need not be initialised.        */
int heal_unc_loss(const float* cls_preds, const float* reg_preds, const float* unc_preds, const float* dir_preds,
                  const void* pos_equal_one, const void* neg_equal_one, const void* targets, int labels_f64, int n, int anchors,
                  int H, int W, int dim, float pos_cls_weight, float alpha, float sigma, float cls_weight, float reg_weight,
                  float unc_weight, float dir_weight, int xy_type, int angle_type, float angle_weight, float lambda_V, float s0,
                  int limit_period, const double* anchor_yaw, double dir_offset, float* terms, float* grad_cls, float* grad_reg,
                  float* grad_unc, float* grad_dir, void* ws, size_t ws_bytes, void* stream);

/* bytes of workspace of heal_decode_nms_agents_unc */
size_t heal_decode_nms_agents_unc_workspace(int anchors_total, int nms_top);

/* heal_decode_nms_agents_unc: the arguments, limits and results of heal_decode_nms_agents (include/heal_amd.h) -- corners, scores
 *   and count are bit-equal to its on the same inputs -- plus
 *     unc_host   host array of n_agents device pointers to the [unc_dim * A, H_k, W_k] uncertainty maps, 1 <= unc_dim <= 16
 *     out_unc    [max_out, unc_dim]: row i = the unc_dim channels of the anchor that kept box i was decoded from
 *     out_index  [max_out] int32 or NULL: that anchor's pooled index (agent k's anchors start at sum_{u<k} H_u W_u A; inside an
 *                agent (row * W + col) * A + anchor)
 *   Front end, rank / re-decode, mask and reduce are heal_decode_nms_agents's kernels; the pooled index travels in the place of
 *   the source agent and one short kernel gathers the rows afterwards.                                                         */
int heal_decode_nms_agents_unc(int n_agents, const float* const* cls_host, const float* const* reg_host,
                               const float* const* dir_host, const float* const* anchors_host, const float* const* unc_host,
                               const int32_t* h_host, const int32_t* w_host, int anchor_num, int num_bins, int unc_dim,
                               float score_thr, float dir_offset, float nms_thr, int nms_top, const float* tfm_host,
                               const float* tfm_dev, const float* gt_range_host, float* out_corners, float* out_scores,
                               float* out_unc, int32_t* out_agent, int32_t* out_index, int32_t* out_count, int max_out, void* ws,
                               size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
