/* heal_amd_align.h -- the aligners of AlignNet beyond ConvNeXt: cross-covariance attention (XCA, the attention of EdgeNeXt's SDTA
 * encoder; opencood/models/sub_modules/feature_alignnet_modules.py:33-67) reduced to one per-image pointwise weight.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  Same conventions as include/heal_amd.h: fp32 NCHW device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no floating-point atomics, workspaces that need not be initialised, *_workspace / *_supported / *_parts
 * are host arithmetic and return 0 for a shape out of range.  The library is built with -ffp-contract=off.
 *
 * XCA on a qkv map [B, 3C, N] (N = H W pixels, channel s C + h d + i = row i of head h of q / k / v for s = 0 / 1 / 2, d = C / heads):
 *     G_b,h[i,j] = sum_n q[b,h,i,n] k[b,h,j,n]        nq[i] = max(||q_i||_2, 1e-12), nk[j] likewise (F.normalize's eps)
 *     A_b,h      = softmax_j( G[i,j] / (nq[i] nk[j]) * temperature[h] )
 *     W_b        = proj_w_scaled * blockdiag_h(A_b,h)                                       [C, C]
 * XCA is linear in v once A is known, so with proj_w_scaled = gamma_xca (.) W_proj the layer's result
 *     x + gamma_xca * xca(norm_xca(x))  =  x + W_b v_b + gamma_xca (.) b_proj
 * is ONE pointwise convolution of the v rows per image (heal_conv1x1 with a bias and a residual); attn @ v is never written.
 *
 * heal_xca_weights is two launches:
 *   Gram pass   grid (parts, heads, B), 256 threads.  A block owns a contiguous range of `range` = heal_xca_range pixels (a multiple
 *               of the 256-pixel block step; the last part may be shorter) and accumulates the d x d Gram tile on
 *               v_mfma_f32_16x16x4_f32 with the PIXEL as the reduction index: lane l loads a float4 of row l & 15 of q and of k at the
 *               same four pixels and feeds four MFMAs from it (any pixel order is valid as long as A and B agree); wave w of a step
 *               takes pixels 64 w .. 64 w + 63, lane group l >> 4 sixteen consecutive ones of them, so a lane's four loads of a step
 *               are consecutive 16-byte pieces of its row.  d = 16 is one accumulator tile, d = 32 two by two.  The squared norms are
 *               the lanes' own sums of the loaded values, reduced over the four lanes of a row.  Pixels past the end of the range
 *               are zeros.  The four waves combine through LDS in wave order and the block writes its d d + 2 d partial sums.
 *   finalise    grid (heads, B).  Sums the partials in part order (bit-equal across launches), forms the logits, subtracts the row
 *               maximum before expf, normalises, and multiplies the head's C x d slice of proj_w_scaled by A.
 */
#ifndef HEAL_AMD_ALIGN_H
#define HEAL_AMD_ALIGN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* heal_align_fused_enabled (host only): HEAL_ALIGN_FUSED as the library reads it, at every call -- 1 when the variable is unset, empty
 *   or "1" (the aligners beyond ConvNeXt run on this library's operators), 0 for "0" (the reference's torch composition on the
 *   device), -1 for any other text.                                                                                          */
int heal_align_fused_enabled(void);

/* heal_xca_supported (host only): 1 if heal_xca_weights takes the shape -- C % heads == 0, d = C / heads in {16, 32}, N % 4 == 0
 *   (16-byte pixel rows, heal_conv1x1's rule), 64 <= N < 2^30 -- else 0.                                                        */
int heal_xca_supported(int C, int heads, int N);

/* heal_xca_parts (host only): the number of pixel ranges the Gram pass splits an image into (grid x): enough blocks to fill the
 *   chip on small batches, every range but the last the same multiple of the 256-pixel step.  0 for a shape out of range.
 * heal_xca_range (host only): the pixels of one part (the last one holds N - (parts - 1) range).                               */
int heal_xca_parts(int B, int heads, int N);
int heal_xca_range(int B, int heads, int N);

/* bytes of workspace of heal_xca_weights (B heads parts (d d + 2 d) floats); 0 for a shape out of range */
size_t heal_xca_workspace(int B, int C, int heads, int N);

/* heal_xca_weights: qkv [B, 3C, N] f32, 16-byte aligned; temperature [heads]; proj_w_scaled [C, C] row-major (row = output channel).
 *   W_out     [B, C, C]                 row-major per image: y_b = W_out[b] v_b
 *   A_out     [B, heads, d, d] or NULL  the attention matrices
 *   stats_out [B, heads, d d + 2 d] or NULL: G (row i, column j at i d + j), then the SQUARED norms of the d q rows, then of the d
 *             k rows, as summed (before the clamp)
 *   ws: heal_xca_workspace bytes, 256-B aligned, need not be initialised.                                                      */
int heal_xca_weights(const float* qkv, const float* temperature, const float* proj_w_scaled, int B, int C, int heads, int N,
                     void* ws, size_t ws_bytes, float* W_out, float* A_out, float* stats_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
