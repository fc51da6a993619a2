/* heal_amd_roi.h -- per-image REGION-OF-INTEREST launches of the pointwise and the small-group 3x3 convolution.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the entry points declared here are shipped in the same
 * library (every build exports them), bound next to it by heal_amd/_capi.py (signatures_roi), and use its limits
 * (HEAL_WARP_MAX_AGENTS).  Purely additive: heal_conv1x1 and heal_grouped_small_conv3x3 keep their signatures and their results
 * bit for bit (they run the same kernels with an empty table).
 * Same conventions as include/heal_amd.h: device pointers unless the name ends in _host, fp32 NCHW, a hipStream_t as void*,
 * non-zero return + heal_last_error() on failure, no host synchronisation (safe under graph capture).
 *
 * What a ROI is.  roi_host: HOST array of n x 4 int32, one box (y0, y1, x0, x1) per image in OUTPUT pixels, 0 <= y <= Ho,
 * 0 <= x <= Wo; y1 <= y0 or x1 <= x0 is an empty box.  n <= HEAL_WARP_MAX_AGENTS.  The table travels BY VALUE in the kernel's
 * arguments -- no device memory -- so a captured HIP graph holds the boxes as constants: they are configuration (which agents are
 * camera agents, how large their crop window is), never data of a frame.
 * A workgroup whose output tile holds no pixel of its image's box returns before its first load and writes NOTHING: the output
 * outside the kept tiles keeps whatever the buffer held.  Inside a kept tile every pixel is computed (also those outside the box)
 * by the instructions of the plain launch on the same values: bit-identical to heal_conv1x1 / heal_grouped_small_conv3x3 there.
 * Reference: the convolutions are those of the ResNeXt bottleneck (opencood/models/sub_modules/resblock.py:67-122); the reference
 * evaluates them on the whole map of every agent although its fusion (pyramid_fuse.py:139-162) multiplies a camera agent's map by a
 * score of exactly zero outside the crop window.
 */
#ifndef HEAL_AMD_ROI_H
#define HEAL_AMD_ROI_H
#include "heal_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* heal_conv1x1_roi: heal_conv1x1 (stride 1 | 2, bias, residual, in_scale, act 0..3 as there) with a ROI.  out_pixel_major must be 0:
 *   the pixel-major, split-K and depth-to-space forms take no ROI (an error, nothing is launched).
 *   Tiles: 64 consecutive pixels of the flattened Ho x Wo output image (x all 64-channel chunks of Cout).  Wo % 64 == 0: a tile is a
 *   row segment (Wo == 64: one row) and is skipped when its row or its columns miss the box -- exact.  A tile that spans several rows
 *   is kept when any row it touches lies in [y0, y1) (its columns are not looked at) -- conservative, never wrong.              */
int heal_conv1x1_roi(const float* x, const float* weight_frag, const float* bias, const float* residual,
                     const float* in_scale, int n, int cin, int cout, int H, int W, int stride, int act,
                     int out_pixel_major, const int32_t* roi_host, float* y, void* stream);

/* heal_conv1x1_box_roi: the same convolution (NCHW output) with the BOX rule: the launch's 64-pixel tiles enumerate each image's
 *   ALIGNED box instead of the image.  For the box (y0, y1, x0, x1): xa = x0 rounded down to 4, xb = x1 rounded up to 4 (inside the
 *   map, as Wo % 4 == 0), bw = xb - xa, bh = y1 - y0.  Tile t of the image covers the box-relative pixels q in [64 t, 64 t + 64),
 *   pixel q being row y0 + q / bw, column xa + q % bw; the ceil(bw bh / 64) tiles with 64 t < bw bh run, the others leave as above.
 *   Exactly the pixels of the aligned box are computed and written -- bit-identical to heal_conv1x1 -- and NOTHING outside it: a
 *   narrow box costs its own pixels, not the rows it touches.  The full box is the plain launch (same addresses); an empty box skips
 *   the image.  An output width that is no multiple of 4 (stride 1 only) keeps heal_conv1x1_roi's tile rule.                      */
int heal_conv1x1_box_roi(const float* x, const float* weight_frag, const float* bias, const float* residual,
                         const float* in_scale, int n, int cin, int cout, int H, int W, int stride, int act,
                         const int32_t* roi_host, float* y, void* stream);

/* heal_grouped_small_conv3x3_roi: heal_grouped_small_conv3x3 (4, 8 or 16 channels per group, stride 1 | 2) with a ROI.
 *   Tiles: TH x TW output pixels (x one 16-channel super-group), TH x TW = 16 x 32 (4 channels per group, stride 1), 8 x 32 (8 or 16
 *   per group, stride 1) or 8 x 16 (stride 2), clipped to the map; a tile is skipped when it holds no pixel of the box -- exact.    */
int heal_grouped_small_conv3x3_roi(const float* x, const float* weight_q, const float* bias, int n, int channels,
                                   int group_channels, int H, int W, int stride, int relu, const int32_t* roi_host,
                                   float* y, void* stream);

/* heal_roi_enabled: 0 when the environment says HEAL_PYRAMID_ROI=0, else 1 (read at every call).  The fusion pyramid's lean walk asks
 *   before it plans a stage by ROI; 0 restores the walk without ROIs (A/B, and the reference side of the equality tests).  The two
 *   entry points above do not look at it.                                                                                       */
int heal_roi_enabled(void);

#ifdef __cplusplus
}
#endif
#endif
