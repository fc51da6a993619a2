// Where2comm fusion, the part between the projections and the out-projection: warp the projected maps of every agent into the ego
// frame, add the projection biases, multi-head attention of the ego pixel over the agents -- one launch per scene.
//
// Reference arithmetic (one scene of n agents, C channels, `heads` heads of d = C / heads channels):
//   opencood/models/fuse_modules/fusion_in_one.py:431-484   Where2commFusion.forward
//       x_j = warp_affine_simple(feats, t[0, :n])[j]                            (torch_transformation_utils.py:323-332)
//       EncodeLayer(x_0, x, x) per pixel                                         (where2comm_attn.py:64-103)
//   nn.MultiheadAttention over a "batch" of H W pixels with sequence length n:
//       q = Wq x_0 + bq,  k_j = Wk x_j + bk,  v_j = Wv x_j + bv
//       per head h:  p_j = softmax_j((q_h * scale) . k_jh),  ctx_h = sum_j p_j v_jh        (scale = 1 / sqrt(d), applied to q)
// The torch composition writes the warped stack and three permuted copies of it; here none of them exists.
//
// Identity (Where2comm): the warp is linear per channel and the projection linear per pixel, so W warp(x) = warp(W x).
// The caller projects the UNWARPED maps without bias (heal_conv1x1: q_map = Wq x_0, kv_map[j] = [Wk; Wv] x_j) and this kernel
// samples them; the bias is added AFTER sampling (zero padding gives partial tap weights at the border, so warp(W x + b) is not
// warp(W x) + b there).  An agent whose footprint misses the pixel has k_j = bk, v_j = bv and keeps its share of the softmax: there
// is no key mask.  The ego goes through the sampler too (row t[0, 0]); `ego_warped` = S_0(x_ego) is the residual of the caller's
// out-projection.
//
// Heads are independent, so -- unlike k_warp_att_fuse, whose one head needs every channel of a pixel -- no partial sums meet in LDS:
// a block is ONE wave, lane = pixel of a 16 x 4 ego tile, blockIdx.z = head.  The thread
//   1. computes, once, its taps per agent (make_taps: the sampling arithmetic of K5 and heal_disco_fuse, in the same order);
//   2. sweeps the d channels of its head of Q and K: n dot products, each K channel read once (and its d channels of x_ego);
//   3. softmax over ALL n agents (max, exp, sum, divide -- torch's order);
//   4. sweeps the d channels of V: ctx[c] = sum_j p_j v_j[c] in agent order, each V channel read once.
// One head per thread gives tiles x heads waves: 2048 at 128 x 128 with 8 heads (8 per CU), 512 at 64 x 64.  The taps are gathered
// directly from global memory, as k_warp_att_fuse does (see the gather notes in k_warp_fuse_lds's header: the LDS staging pays when
// one staged footprint serves many channels of ONE block; here a wave touches d channels of 2 n + 2 maps).
// Registers: n x (4 weights + 4 offsets) + n logits.  fp32 throughout; no atomics, no LDS, no barrier: two launches are bit-equal,
// and the `logits` hook only adds stores.
#include "common.h"
#include "warp_taps.h"
#include "../../include/heal_amd_ext.h"

namespace heal {

constexpr int WM_TW = 16, WM_TH = 4;      // ego pixel tile of a wave

struct WarpMhaParams {
    const float* q_map;     // [C, H, W]
    const float* kv_map;    // [n, 2C, H, W]
    const float* x_ego;     // [C, H, W]
    const float *bq, *bk, *bv;
    float* ctx;             // [C, H, W]
    float* ego_warped;      // [C, H, W]
    float* logits;          // [n, heads, H, W] or null
    AffineRows rows;
    int C, heads, H, W;
    float scale;
};

template <int NA>
__global__ __launch_bounds__(HEAL_WAVE) void k_warp_mha_fuse(const WarpMhaParams P) {
    const Block3 bk = xcd_block();      // x, y: tile, z: head -- neighbouring tiles of one head share rotated footprints
    const int l = threadIdx.x;
    const int w = bk.x * WM_TW + (l & (WM_TW - 1)), h = bk.y * WM_TH + (l / WM_TW);
    const int head = bk.z;
    const bool live = w < P.W && h < P.H;
    const int C = P.C, HW = P.H * P.W, d = C / P.heads;
    const int pix = live ? h * P.W + w : 0;
    int off[NA][4];
    float wt[NA][4];
    unsigned reach = 0;      // bit a: some lane of this wave samples agent a inside its map
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        pixel_taps(P.rows, a, h, w, P.H, P.W, live, off[a], wt[a]);
        const bool any = (wt[a][0] != 0.f) | (wt[a][1] != 0.f) | (wt[a][2] != 0.f) | (wt[a][3] != 0.f);
        reach |= __ballot(any) ? (1u << a) : 0u;
    }
    const int c_lo = head * d, c_hi = c_lo + d;
    const bool ego_in = reach & 1u;
    // a map out of reach of the whole wave is a zero operand (its loads are skipped, never its term of the softmax)
    auto sample_k = [&](int a, int c) -> float {
        return ((reach >> a) & 1u) ? tap4(P.kv_map + ((size_t)a * 2 * C + c) * HW, off[a], wt[a]) : 0.f;
    };

    // ---- sweep 1: Q and K of this head, the ego's own map --------------------------------------------------------------------
    float prob[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) prob[a] = 0.f;
#pragma unroll 2
    for (int c = c_lo; c < c_hi; ++c) {
        const float xe = ego_in ? tap4(P.x_ego + (size_t)c * HW, off[0], wt[0]) : 0.f;
        if (live) P.ego_warped[(size_t)c * HW + pix] = xe;
        if (NA > 1 || P.logits != nullptr) {
            float q = ego_in ? tap4(P.q_map + (size_t)c * HW, off[0], wt[0]) : 0.f;
            q = (q + P.bq[c]) * P.scale;      // F.multi_head_attention_forward scales q before the product
            const float bkc = P.bk[c];
#pragma unroll
            for (int a = 0; a < NA; ++a) prob[a] += q * (sample_k(a, c) + bkc);
        }
    }
    if (P.logits != nullptr && live) {
#pragma unroll
        for (int a = 0; a < NA; ++a) P.logits[((size_t)a * P.heads + head) * HW + pix] = prob[a];
    }

    // ---- softmax over the agents ---------------------------------------------------------------------------------------------
    if (NA == 1) {
        prob[0] = 1.f;      // the softmax of one logit: expf(0) / 1
    } else {
        softmax_agents(prob);
    }

    // ---- sweep 2: V of this head ---------------------------------------------------------------------------------------------
#pragma unroll 2
    for (int c = c_lo; c < c_hi; ++c) {
        const float bvc = P.bv[c];
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < NA; ++a) acc += prob[a] * (sample_k(a, C + c) + bvc);
        if (live) P.ctx[(size_t)c * HW + pix] = acc;
    }
}

}  // namespace heal

using namespace heal;

extern "C" int heal_warp_mha_fuse(const float* q_map, const float* kv_map, const float* x_ego, const float* bq, const float* bk,
                                  const float* bv, int n_agents, int channels, int heads, int H, int W, float scale,
                                  const double* affine_host, const double* affine_dev, int grid_f64, float* ctx, float* ego_warped,
                                  float* logits, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && n_agents <= WF_MAXA, "warp_mha_fuse: n_agents must be in [1,%d] (got %d)", WF_MAXA, n_agents);
    HEAL_REQUIRE(channels >= 1 && heads >= 1 && heads <= 65535 && channels % heads == 0,
                 "warp_mha_fuse: channels (%d) must be a positive multiple of heads (%d)", channels, heads);
    HEAL_REQUIRE(H >= 1 && W >= 1, "warp_mha_fuse: bad shape");
    HEAL_REQUIRE(2ll * n_agents * channels * H * W < (1ll << 31), "warp_mha_fuse: more than 2^31 elements");
    HEAL_REQUIRE(ceil_div(H, WM_TH) <= 65535, "warp_mha_fuse: H too large");
    HEAL_REQUIRE(q_map && kv_map && x_ego && bq && bk && bv && ctx && ego_warped, "warp_mha_fuse: null operand");
    WarpMhaParams P;
    if (fill_affine_rows(P.rows, "warp_mha_fuse", affine_host, affine_dev, n_agents, grid_f64)) return 1;
    P.q_map = q_map; P.kv_map = kv_map; P.x_ego = x_ego; P.bq = bq; P.bk = bk; P.bv = bv;
    P.ctx = ctx; P.ego_warped = ego_warped; P.logits = logits;
    P.C = channels; P.heads = heads; P.H = H; P.W = W; P.scale = scale;
    const dim3 grid(ceil_div(W, WM_TW), ceil_div(H, WM_TH), heads);
    hipStream_t st = (hipStream_t)stream;
    HEAL_FOR_AGENTS(n_agents, "warp_mha_fuse", HEAL_LAUNCH_EV(k_warp_mha_fuse<NA>, grid, dim3(HEAL_WAVE), 0, st, P));
    HEAL_LAUNCH_CHECK();
    return 0;
}
