/* heal_amd_ext.h -- additive INFERENCE entry points outside the versioned table.
 *
 * include/heal_amd.h (HEAL_AMD_ABI_VERSION) is the table a reference maintainer binds; it stays as it is.  Entry points added after
 * it was closed are declared here: they are shipped in the same library (every build exports them), bound next to it by
 * heal_amd/_capi.py, and use its limits (HEAL_WARP_MAX_AGENTS).
 * Same conventions as include/heal_amd.h: device pointers, fp32 NCHW, a hipStream_t as void*, non-zero return +
 * heal_last_error() on failure, no host synchronisation (safe under graph capture).
 */
#ifndef HEAL_AMD_EXT_H
#define HEAL_AMD_EXT_H
#include "heal_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* heal_warp_mha_fuse: Where2comm's fusion of one scene between its projections and its out-projection (reference:
 *   opencood/models/fuse_modules/fusion_in_one.py:431-484 with where2comm_attn.py:64-103): per ego pixel the PROJECTED maps of
 *   every agent are sampled in the ego frame (the sampling arithmetic of heal_warp_fuse; agent 0 goes through the sampler too, with
 *   row 0), the projection biases are added after sampling, and the ego attends over the agents head by head:
 *     q = S_0(q_map) + bq,  k_j = S_j(kv_map[j, :C]) + bk,  v_j = S_j(kv_map[j, C:]) + bv
 *     per head h (d = channels / heads):  p_j = softmax_j((q_h * scale) . k_jh),  ctx_h = sum_j p_j v_jh
 *     ego_warped = S_0(x_ego)
 *   The softmax runs over ALL n agents: one whose footprint misses the pixel has k_j = bk, v_j = bv (no key mask).
 *   q_map [C,H,W] = Wq x_0 and kv_map [n,2C,H,W] = [Wk; Wv] x_j are projections of the UNWARPED maps WITHOUT bias (W warp(x) =
 *   warp(W x); the bias does not commute with the zero padding); x_ego [C,H,W] is the ego's unwarped map; bq, bk, bv [C].
 *   1 <= n_agents <= HEAL_WARP_MAX_AGENTS, channels % heads == 0, any H, W; affine_host | affine_dev: n_agents x (2,3) fp64 rows
 *   as heal_warp_fuse.  ctx, ego_warped [C,H,W]; logits: NULL, or [n,heads,H,W] receiving the scaled logits (a testing hook: the
 *   other outputs are bit-identical with and without it).  One wave per (16 x 4 ego tile, head); no atomics: launches are
 *   bit-equal.                                                                                                                  */
int heal_warp_mha_fuse(const float* q_map, const float* kv_map, const float* x_ego, const float* bq, const float* bk,
                       const float* bv, int n_agents, int channels, int heads, int H, int W, float scale,
                       const double* affine_host, const double* affine_dev, int grid_f64, float* ctx, float* ego_warped,
                       float* logits, void* stream);

/* heal_scan_exclusive, heal_radix_sort_pairs: the two index-building primitives of csrc/prims.hip (the rulebook sort, candidate
 *   compaction and granule scan of the sparse convolution; the cell sort of heal_bev_pool) as entry points of their own -- TEST
 *   SURFACES: the model path reaches the primitives through their clients only.  Thin wrappers, no kernels of their own.
 *   heal_scan_exclusive: out[i] = in[0] + ... + in[i-1] in int32 (wrapping like the additions it stands for); *total (device word,
 *     may be NULL) = the sum of all n.  in == out is allowed.  n == 0 writes *total = 0 when total is given and launches nothing
 *     else.  ws: heal_scan_exclusive_workspace(n) bytes, 4-byte aligned.
 *   heal_radix_sort_pairs: STABLE ascending sort of n (key, value) pairs by the low 9 * ceil(key_bits / 9) bits of the keys (all
 *     32 when that reaches 32: the last 9-bit digit is a full digit); the other key bits and the values are carried along.  keys0 /
 *     vals0 hold the input, keys1 / vals1 are the second halves of the ping-pong ([n] words each, all four distinct);
 *     *result_buf_host (HOST int, written before the function returns: it depends on key_bits alone) = 0 | 1 = the pair that holds
 *     the result, ceil(key_bits / 9) % 2 for n > 1 and 0 for n <= 1 (nothing is launched); the other pair is left holding the input or an
 *     intermediate pass.  1 <= key_bits <= 32.  ws: heal_radix_sort_pairs_workspace(n) bytes, 4-byte aligned.
 *   Both refuse a negative n, null pointers (operands: when n > 0) and a workspace smaller than the query before any launch.   */
size_t heal_scan_exclusive_workspace(int n);
int heal_scan_exclusive(const int32_t* in, int32_t* out, int n, int32_t* total, void* ws, size_t ws_bytes, void* stream);
size_t heal_radix_sort_pairs_workspace(int n);
int heal_radix_sort_pairs(uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1, int n, int key_bits,
                          int* result_buf_host, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
