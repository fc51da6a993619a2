/* heal_amd_train_bn.h -- entry points of the fused BatchNorm (+ residual) (+ ReLU) of the GRADIENT path.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them) and serve the opt-in kernel-backed BatchNorm of the training step
 * (heal_amd.ops.BatchNormAct, ops.bn_grad("kernel"), bev_blocks.grad_bn_act).
 * Same conventions as include/heal_amd.h: fp32 NCHW device pointers, a hipStream_t as void*, non-zero return + heal_last_error()
 * on failure, no host synchronisation (safe under graph capture), workspaces supplied by the caller (need not be initialised).
 *
 * x, y, dy, dx, residual, dresidual are [n, C, H*W] maps (HW = H * W); mean, rstd, gamma, beta, dgamma, dbeta, running_* hold C
 * values; M = n * HW is the number of elements of a channel.  No alignment or divisibility requirement: 16-byte accesses are used
 * when HW % 4 == 0 and every map pointer of the call is 16-byte aligned, dword accesses otherwise.
 *
 * Reductions: a SEGMENT is a contiguous run of at most HEAL_BN_SEGMENT elements of one (sample, channel) plane.  A 256-thread
 * block takes whole segments in a grid-stride loop and writes one pair of fp64 partial sums per segment, indexed by the segment
 * (not by the block); a second kernel (one block per channel) adds a channel's partials in segment order.  No floating-point
 * atomics: repeated launches are bit-equal and no result depends on the number of blocks.
 */
#ifndef HEAL_AMD_TRAIN_BN_H
#define HEAL_AMD_TRAIN_BN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_BN_SEGMENT 4096

/* heal_bn_train_supported: 1 if n, C, HW >= 1, HW <= 2^30 and n * C * ceil(HW / HEAL_BN_SEGMENT) <= 2^30 (index ranges only).
 * heal_bn_train_workspace: bytes of workspace any of the calls below needs for that shape (0 for an unsupported one).        */
int heal_bn_train_supported(int n, int C, int HW);
size_t heal_bn_train_workspace(int n, int C, int HW);

/* heal_bn_train_max_blocks: testing hook.  Caps the grid of the segment kernels at `blocks` (>= 1; 0 restores the default of 2048)
 *   for the calls that follow in this process and returns the previous cap.  Results must not depend on it.                    */
int heal_bn_train_max_blocks(int blocks);

/* heal_bn_stats: per channel the mean and the biased variance over the M elements, rstd = 1 / sqrt(var + eps).
 *   Accumulated in fp64 as sums of (x - K_c) and (x - K_c)^2 with K_c = x[0, c, 0] (the product of two fp32 values is exact in
 *   fp64; the shift removes the E[x^2] - mean^2 cancellation); mean = K_c + S1 / M, var = S2 / M - (S1 / M)^2 in fp64, each
 *   rounded once to fp32.  running_mean / running_var (both or neither): r <- (1 - momentum) r + momentum * stat in fp64, rounded
 *   once; running_var takes the unbiased variance var * M / (M - 1), which needs M >= 2.                                        */
int heal_bn_stats(const float* x, int n, int C, int HW, double eps, double momentum, float* save_mean, float* save_rstd,
                  float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);

/* heal_bn_act_forward: xh = (x - mean[c]) * rstd[c];  z = xh * gamma[c] + beta[c] (+ residual);  y = relu ? max(z, 0) : z
 *   (each operation rounded to fp32, in this order).  mean / rstd: heal_bn_stats' or, for a frozen BatchNorm, the running mean and
 *   1 / sqrt(running_var + eps) formed by the caller.  residual may be null.                                */
int heal_bn_act_forward(const float* x, const float* residual, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int n, int C, int HW, int relu, float* y, void* stream);

/* heal_bn_act_backward: dz = relu ? (y > 0 ? dy : 0) : dy  (y: the forward's result, required exactly when relu);
 *   xh = (x - mean[c]) * rstd[c];  dbeta[c] = sum dz,  dgamma[c] = sum dz * xh  (fp64 partials per segment, added in segment order);
 *   batch_stats = 1:  dx = gamma rstd ((dz - dbeta / M) - xh * (dgamma / M));   batch_stats = 0 (frozen statistics): dx = gamma rstd dz;
 *   dresidual = dz.  dx, dresidual, dgamma, dbeta may each be null: what is not asked for is not written, and the reduction is
 *   skipped when batch_stats = 0 and neither dgamma nor dbeta is wanted.                                                      */
int heal_bn_act_backward(const float* dy, const float* x, const float* y, const float* mean, const float* rstd, const float* gamma,
                         int n, int C, int HW, int relu, int batch_stats, float* dx, float* dresidual, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
