/* heal_amd_comm.h -- Where2comm's spatial communication: the confidence-map mask of every pyramid level, and the multiscale
 * warp + attention / max fusion reading masked maps.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  Same conventions as include/heal_amd.h: fp32 NCHW device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no floating-point atomics, workspaces that need not be initialised, *_workspace / *_supported are host
 * arithmetic and return 0 for a shape out of range.
 *
 * heal_comm_mask = Communication.forward (opencood/models/comm_modules/where2comm.py:34-78) for all scenes of a batch, plus the
 * F.max_pool2d(mask, 2) per further pyramid level of Where2comm.forward (fuse_modules/where2comm_attn.py:264-275).  Per agent:
 *   c = max_a sigmoid(psm[a])                                            (:52; evaluated as the sigmoid of the largest logit)
 *   s = bias + w[0] c[tap 0] + w[1] c[tap 1] + ...                       (:55; the k x k taps in row-major order, added one by one
 *       to an fp32 accumulator that starts at the bias; c is zero outside the map: Conv2d's padding of (k - 1) / 2)
 *       weight NULL: s = c                                               (:57, a config without `gaussian_smooth`)
 *   m = s > thre ? 1 : 0                                                 (:61)
 *   count[scene] = number of ones of the scene's FIRST agent             (:63, before the override)
 *   m = 1 where the agent's index within its scene is even               (:69-71: `communication_mask_nodiag[::2] = 1` forces the
 *       masks of agents 0, 2, 4, ... of a scene, not only the ego's)
 *   level l: the maximum of m over the 2^l x 2^l square, [H >> l, W >> l] (floor-mode pooling nests, so this is the l-fold
 *       max_pool2d(., 2); no level is read back to form the next)
 *   rate = (float(count_0) / float(H W) + float(count_1) / float(H W) + ...) / float(B), added in scene order in fp32 (:63, :76)
 * Two launches: (1) one block of 256 threads per 32 x 32 tile of one agent (the tile and its halo of c are staged in LDS once;
 * every level's cells of the tile are written from there; an ego's tile leaves its number of ones in the workspace); (2) one block
 * adds the tiles' integers in a fixed order.  Integer counting only; two launches on the same values are bit-equal.
 *
 * heal_warp_att_fuse_levels_masked = heal_warp_att_fuse_levels (include/heal_amd.h) with a mask per (level, agent): every bilinear
 * tap of agent j is multiplied by the mask value at that tap before it is weighted, so the result equals the unmasked entry on
 * maps premultiplied by their masks -- which are never written.  The kernel is the unmasked entry's, instantiated with a flag.
 */
#ifndef HEAL_AMD_COMM_H
#define HEAL_AMD_COMM_H
#include <stddef.h>
#include <stdint.h>
#include "heal_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_COMM_MAX_K 9            /* largest (odd) filter size of heal_comm_mask                                              */
#define HEAL_COMM_MAX_AGENTS 512     /* largest n_total of heal_comm_mask (the agents' scene table travels with the launch)      */

/* heal_comm_fused_enabled (host only): the HEAL_COMM_FUSED environment switch, read when called: 1 when it is unset, empty or "1"
 *   (Where2comm runs on the two kernels below), 0 when it is "0" (the module runs the reference's torch composition on the device:
 *   the A/B switch of scripts/w2c_comm_bench.py), -1 for any other text.                                                          */
int heal_comm_fused_enabled(void);

/* heal_comm_mask_supported (host only): 1 if heal_comm_mask takes this problem, else 0 --
 *   1 <= B <= n_total <= HEAL_COMM_MAX_AGENTS, A >= 1, H >= 1, W >= 1, H * W < 2^31, n_total * A * H * W < 2^62,
 *   k odd with 1 <= k <= HEAL_COMM_MAX_K, 1 <= n_levels <= HEAL_WARP_MAX_LEVELS.                                                */
int heal_comm_mask_supported(int n_total, int B, int A, int H, int W, int k, int n_levels);

/* bytes of workspace of heal_comm_mask; 0 for a shape out of range */
size_t heal_comm_mask_workspace(int B, int H, int W);

/* heal_comm_mask: psm [n_total, A, H, W] fp32; record_len_host [B] (host, every entry >= 1, their sum n_total);
 *   weight [k, k] and bias [1] fp32 ON THE DEVICE (the module's parameters, read at run time); weight NULL: no smoothing, bias and
 *   k are then not read.  mask_host [n_levels] (host) of device pointers: mask_host[l] <- [n_total, 1, H >> l, W >> l] fp32 zeros
 *   and ones; a level with H >> l == 0 or W >> l == 0 has no element and its pointer is not read.  count [B] int32, rate [1] fp32.
 *   ws: heal_comm_mask_workspace bytes, 256-B aligned, need not be initialised.  Fails where heal_comm_mask_supported is 0.      */
int heal_comm_mask(const float* psm, int n_total, int A, int H, int W, const int32_t* record_len_host, int B, const float* weight,
                   const float* bias, int k, float thre, int n_levels, float* const* mask_host, int32_t* count, float* rate,
                   void* ws, size_t ws_bytes, void* stream);

/* heal_warp_att_fuse_levels_masked: the arguments of heal_warp_att_fuse_levels, and mask_host [n_levels] (host) of device
 *   pointers to [n_agents, 1, H_l, W_l] fp32 (any values; Where2comm's are zeros and ones).                                      */
int heal_warp_att_fuse_levels_masked(int n_levels, const float* const* feats_host, const float* const* mask_host, int n_agents,
                                     const int32_t* channels_host, const int32_t* h_host, const int32_t* w_host,
                                     const float* sqrt_dim_host, const double* affine_host, const double* affine_dev, int grid_f64,
                                     int mode, float* const* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
