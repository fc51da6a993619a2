/* heal_amd_train_warp.h -- warp_affine_simple as a stand-alone differentiable operator: forward and backward kernels.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  They serve the warp of every agent's map into the ego frame that all baseline fusions and
 * every CoAlign level start with (heal_amd.ops.warp_affine / ops.WarpAffine, ops.warp_grad("kernel"), fusion_in_one.py).
 * Same conventions as include/heal_amd.h: fp32 NCHW device pointers, a hipStream_t as void*, non-zero return + heal_last_error()
 * on failure, no host synchronisation (safe under graph capture).  Includes heal_amd.h for HEAL_WARP_MAX_AGENTS.
 *
 * Arithmetic (torch_transformation_utils.py:323-332: F.affine_grid(M, size, align_corners=False).to(src) + F.grid_sample(bilinear,
 * zeros padding, align_corners=False)), for agent a with row m = (m00 m01 m02 m10 m11 m12) and destination pixel d = (w, h):
 *   xs = base(w, W), ys = base(h, H),  base(j, n) = element j of linspace(-1, 1, n) * (n - 1) / n      (in T)
 *   gx = (float)((m00 xs + m01 ys) + m02),  gy = (float)((m10 xs + m11 ys) + m12)                      (in T, rounded once to fp32)
 *   ix = ((gx + 1) W - 1) / 2,  iy = ((gy + 1) H - 1) / 2,  x0 = floor(ix), y0 = floor(iy)             (fp32)
 *   taps nw (x0, y0), ne (x0+1, y0), sw (x0, y0+1), se (x0+1, y0+1) with weights (x1-ix)(y1-iy), (ix-x0)(y1-iy), (x1-ix)(iy-y0),
 *   (ix-x0)(iy-y0): products of fp32 differences; a tap outside the map contributes exactly zero
 *   out[a, c, d] = ((src[nw] w_nw + src[ne] w_ne) + src[sw] w_sw) + src[se] w_se                       (fp32, the taps inside only)
 * T = double when grid_f64 != 0 (the affine matrix came as float64: pairwise_t_matrix from numpy), else float (the row is rounded
 * to fp32 first).  This is csrc/warp_taps.h, the code every warp kernel of the library shares: the forward here is bit-equal to
 * heal_warp_agent agent by agent.
 *
 * Backward: the adjoint in GATHER form.  grad_src[a, c, s] = sum over the destination pixels d that have s among their four taps
 * of w(d, s) * grad_out[a, c, d].  In pixel units a row maps d to p(d) = A d + b with A = [[m00, m01 W/H], [m10 H/W, m11]];
 * s is a tap of d only if |p(d) - s|_inf < 1, so d lies within r_x = |Ainv_00| + |Ainv_01| (r_y = |Ainv_10| + |Ainv_11|) of
 * Ainv (s - b).  One thread owns one source pixel of one agent for HEAL_WARP_BWD_CHANNELS channels, walks that box of candidates
 * in destination row-major order, re-runs the forward's sampling arithmetic on each and, where one of the four taps (order nw, ne,
 * sw, se) is s, does acc[c] = acc[c] + w * G[c, d] (one fp32 multiply, one fp32 add).  Membership and weights are the forward's
 * own; the box only has to be a superset, which the margin HEAL_WARP_BWD_MARGIN(H, W) = 0.01 + 2^-20 max(H, W) added to both
 * reaches secures against the fp32 rounding of gx, gy, ix, iy.  No atomics, no zeroed destination: every element of grad_src is
 * written (zeros included), and repeated launches are bit-equal.  A rigid row (rotation + shift, what normalize_pairwise_tfm
 * produces for a square-celled map) has r <= sqrt(2): at most 4 x 4 candidates and at most 5 contributors per source pixel.
 */
#ifndef HEAL_AMD_TRAIN_WARP_H
#define HEAL_AMD_TRAIN_WARP_H
#include <stddef.h>
#include <stdint.h>
#include "heal_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_WARP_BWD_MAX_REACH 4.0   /* largest r_x, r_y (before the margin) the backward takes: at most 10 candidates per axis */
#define HEAL_WARP_BWD_CHANNELS 32     /* channels per thread of the backward kernel (blockIdx.z = agent x channel chunk)        */

/* heal_warp_affine_forward: out[a] = warp_affine_simple(src[a], row a) for the n agents of a scene in one launch, NCHW in and out.
 *   1 <= n <= HEAL_WARP_MAX_AGENTS; any C, H, W >= 1 with H * W <= 2^30 and n * ceil(C / 16) <= 65535.
 *   affine_host | affine_dev: n x (2,3) fp64 rows, by value from the host or read from device memory at run time (affine_dev wins
 *   when both are given), as heal_warp_fuse.  src and out must not overlap.                                                     */
int heal_warp_affine_forward(const float* src, int n, int C, int H, int W, const double* affine_host, const double* affine_dev,
                             int grid_f64, float* out, void* stream);

/* heal_warp_affine_backward_supported (host only): 1 if the backward takes these rows on an H x W map --
 *   every entry finite, |det A| >= 1e-9, r_x, r_y <= HEAL_WARP_BWD_MAX_REACH, 1 <= n <= HEAL_WARP_MAX_AGENTS, H, W >= 1 and
 *   H * W <= 2^30 -- else 0.  affine_host: n x 6 doubles (may be null only to ask about a shape that is refused anyway).        */
int heal_warp_affine_backward_supported(const double* affine_host, int n, int H, int W);

/* heal_warp_affine_window (host only): the per-agent parameters a backward launch passes for one row (6 doubles) on an H x W map:
 *   out[0..3] = Ainv (row-major), out[4..5] = b, out[6] = r_x + margin, out[7] = r_y + margin.  The candidates of source pixel
 *   s = (sx, sy) are the integer d = (w, h) with |w - cx| <= out[6], |h - cy| <= out[7], (cx, cy) = Ainv (s - b), clipped to the
 *   map.  Returns 0, or non-zero (+ heal_last_error) for a row that heal_warp_affine_backward_supported refuses.               */
int heal_warp_affine_window(const double* row, int H, int W, double* out);

/* heal_warp_affine_backward: grad_src [n, C, H, W] <- adjoint of heal_warp_affine_forward applied to grad_out [n, C, H, W].
 *   Rows from the host only (the support rule above is a host decision; a call it refuses fails and launches nothing).
 *   Also needs n * ceil(C / HEAL_WARP_BWD_CHANNELS) <= 65535.  grad_src need not be initialised and must not overlap grad_out.  */
int heal_warp_affine_backward(const float* grad_out, int n, int C, int H, int W, const double* affine_host, int grid_f64,
                              float* grad_src, void* stream);

#ifdef __cplusplus
}
#endif
#endif
