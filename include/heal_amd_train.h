/* heal_amd_train.h -- entry points of the TRAINING side of the dense BEV convolutions.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) is what a reference maintainer binds and stays as it is; the
 * kernels declared here are shipped in the same library (every build exports them) and serve the opt-in kernel-backed backward
 * of the dense convolutions (heal_amd.ops.ConvGrad, HEAL_CONV_GRAD=kernel).
 * Same conventions as include/heal_amd.h: device pointers, fp32 NCHW, a hipStream_t as void*, non-zero return +
 * heal_last_error() on failure, no host synchronisation (safe under graph capture), workspaces supplied by the caller.
 */
#ifndef HEAL_AMD_TRAIN_H
#define HEAL_AMD_TRAIN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* heal_conv_wgrad: the weight gradient of a dense convolution (what torch.nn.grad.conv2d_weight computes, and what autograd runs on
 *   the library for every conv3x3 / conv1x1 of opencood/models/sub_modules/resblock.py:18-122 during a training step):
 *     dW[co][ci][ky][kx] = sum over n, oy, ox of  g[n][co][oy][ox] * x[n][ci][oy*s + ky - p][ox*s + kx - p]
 *   with reads outside the map taken as zero; k = 1 | 3, p = k / 2, s = stride = 1 | 2.
 *   x [n, cin, H, W], g [n, cout, Ho, Wo] with Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1, dw [cout, cin, k, k]; fp32, any sizes >= 1
 *   (no alignment requirement: heal_conv_wgrad_supported only bounds the index ranges).
 *   A GEMM with M = cout, N = cin per tap and the PIXELS as the reduction, on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate).  A
 *   block owns 64 x 32 (cout x cin) of all k*k taps; it walks pixel tiles of R output rows x 32 output columns (R = 4 for stride 1,
 *   2 for stride 2), staging the tile of g and the matching halo tile of x in LDS once and serving every tap from it by shifted LDS
 *   reads; image borders and tile tails are zeros in LDS.
 *   The list of n * ceil(Ho / R) * ceil(Wo / 32) pixel tiles is cut into heal_conv_wgrad_splits(...) contiguous parts (a pure function
 *   of the shape: enough parts to fill the chip when cout x cin is small, never an empty one; tiles % splits leading parts hold one
 *   tile more than the rest).  With more than one part each writes its partial [split][cout][cin][k*k] to ws and a second launch adds
 *   the partials in split order: no floating-point atomics, repeated launches are bit-equal.
 *   ws: heal_conv_wgrad_workspace(...) bytes (0 for one split or an unsupported shape), need not be initialised.                    */
int heal_conv_wgrad_supported(int n, int cin, int cout, int H, int W, int k, int stride);
int heal_conv_wgrad_splits(int n, int cin, int cout, int H, int W, int k, int stride);
size_t heal_conv_wgrad_workspace(int n, int cin, int cout, int H, int W, int k, int stride);
int heal_conv_wgrad(const float* x, const float* g, int n, int cin, int cout, int H, int W, int k, int stride, float* dw, void* ws,
                    size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
