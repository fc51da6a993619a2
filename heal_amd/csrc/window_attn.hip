// Fused window attention of the V2X-ViT pyramid (opencood/models/sub_modules/mswin.py:46-80,
// BaseWindowAttention): for every (agent, ws x ws window, head)
//     O = softmax(scale * Q K^T + pos_bias) V,      Q, K, V [T = ws*ws, d]
// straight from the packed to_qkv output [L,H,W,3*m*d] to [L,H,W,m*d].  The library path materialises the window
// re-layout of q/k/v, the [B,T,T] score tensor (0.5 GB at ws = 16), its softmax and the re-layout of the result:
// ~2.5 GB of HBM traffic per attention against 0.54 GB compulsory.
//
// One block per (window, head, agent), up to 4 waves (8 for the 256-token window); a wave owns 16-query slabs.  The transposed
// MFMA scheme (operand layouts, the softmax in one lane column, the probabilities as the B operand) and its blocks are in
// attn_tiles.h; the kernels here are the slab loops around them.
#include "attn_tiles.h"
#include "../../include/heal_amd.h"

namespace heal {

// waves per block: one per 16-query slab up to 4; the 256-token window runs 8 waves (K and V of the window in LDS: 139 KB, one
// block per CU, two waves per SIMD)
template <int WS>
constexpr int wattn_waves() { return WS * WS == 256 ? 8 : ((WS * WS / 16) < 4 ? (WS * WS / 16) : 4); }

template <int WS, int D>
__global__ __launch_bounds__(64 * wattn_waves<WS>()) void k_window_attn(
    const float* __restrict__ qkv /*[L,H,W,3,m,D]*/, const float* __restrict__ bias /*[T,T] or null*/, int H, int W,
    int m, float scale, float* __restrict__ out /*[L,H,W,m*D]*/) {
    constexpr int T = WS * WS, NCB = T / 16, NB = D / 16, NW = wattn_waves<WS>();
    constexpr int STR = D + 4;                           // row stride (words) of the LDS tiles (attn_tiles.h)
    __shared__ __attribute__((aligned(16))) float sK[T * STR];
    __shared__ __attribute__((aligned(16))) float sV[T * STR];
    const int nww = W / WS;
    const int ih = blockIdx.x / nww, iw = blockIdx.x - ih * nww, h = blockIdx.y, l = blockIdx.z;
    const WindowTokens<WS> tok{ih, iw, W};
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const float* base = qkv + ((size_t)l * H * W) * C3 + (size_t)h * D;      // q of this agent and head; k at + MD, v at + 2 MD
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    // Q rows of the first slab: requested together with K / V (one exposed round trip)
    float4 qf[NB];
    load_frag<D>(base + tok(min(wave, T / 16 - 1) * 16 + ln) * C3, lk, qf);
    stage_rows<D, 64 * NW>(tok, T, base + MD, C3, base + 2 * MD, C3, sK, sV);
    __syncthreads();
    for (int slab = wave; slab < T / 16; slab += NW) {
        const size_t qpix = tok(slab * 16 + ln);
        if (slab != wave) load_frag<D>(base + qpix * C3, lk, qf);
        f32x4 s[NCB];
        float mx, inv;
        query_scores<NCB, D>(sK, qf, bias ? bias + (size_t)(slab * 16 + ln) * T + lk * 4 : nullptr, scale, NCB, lk, ln, s, mx, inv);
        // ---- O^T = V^T P^T: B = the (unnormalised) probabilities as they lie -------------------------------------------------------
        f32x4 o[NB];
        zero_tiles(o);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) col_accumulate<D>(sV, cb, r, lk, ln, s[cb][r], o);
            if constexpr (NCB >= 16) __builtin_amdgcn_sched_barrier(0);
        }
        store_tiles(out + ((size_t)l * H * W + qpix) * MD + (size_t)h * D + lk * 4, o, inv);
    }
}

// ---- backward (training; OPT-IN until measured: HEAL_WATTN_GRAD=kernel) -----------------------------------------------------------
// What autograd derives from mswin.py:64-78 (scores + bias -> softmax -> weighted sum), as two passes over the same blocks:
//   pass A (keys / values of the window in LDS, a wave owns 16-QUERY slabs: the forward's loop) recomputes P, then per key tile
//       dP^T = V dO^T,  dS^T = P^T o (dP^T - D),  D_q = dO_q . O_q (from the saved output: no second sweep),
//       dQ^T += K^T dS^T  (the forward's O^T pattern with K for V and dS for P), grad_bias += dS (atomics), and leaves
//       (max, 1 / sum, D) per query in `stats`;
//   pass B (QUERIES and dO of the window in LDS, a wave owns 16-KEY slabs) rebuilds one score tile at a time from the stats,
//       dV^T += dO^T P,  dK^T += Q^T dS  (key_owned_pass of attn_tiles.h).
// Every GEMM is one of the forward's two MFMA patterns, so no operand changes layout here either.
template <int WS, int D>
__global__ __launch_bounds__(64 * wattn_waves<WS>()) void k_window_attn_bwd_q(
    const float* __restrict__ qkv, const float* __restrict__ bias, const float* __restrict__ outp /*[L,H,W,m*D]*/,
    const float* __restrict__ gout /*[L,H,W,m*D]*/, int H, int W, int m, float scale, float* __restrict__ gqkv,
    float* __restrict__ gbias /*[T,T] or null*/, float4* __restrict__ stats /*[L][windows][m][T]*/) {
    constexpr int T = WS * WS, NCB = T / 16, NB = D / 16, NW = wattn_waves<WS>();
    constexpr int STR = D + 4;
    __shared__ __attribute__((aligned(16))) float sK[T * STR];
    __shared__ __attribute__((aligned(16))) float sV[T * STR];
    const int nww = W / WS;
    const int ih = blockIdx.x / nww, iw = blockIdx.x - ih * nww, h = blockIdx.y, l = blockIdx.z;
    const WindowTokens<WS> tok{ih, iw, W};
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const float* base = qkv + ((size_t)l * H * W) * C3 + (size_t)h * D;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    stage_rows<D, 64 * NW>(tok, T, base + MD, C3, base + 2 * MD, C3, sK, sV);
    __syncthreads();
    float4* st = stats + (((size_t)l * gridDim.x + blockIdx.x) * m + h) * T;
    for (int slab = wave; slab < T / 16; slab += NW) {
        const size_t qpix = (size_t)l * H * W + tok(slab * 16 + ln);
        float4 qf[NB], gf[NB], of[NB];
        load_frag<D>(qkv + qpix * C3 + (size_t)h * D, lk, qf);
        load_frag<D>(gout + qpix * MD + (size_t)h * D, lk, gf);
        load_frag<D>(outp + qpix * MD + (size_t)h * D, lk, of);
        float dsum = 0.f;
#pragma unroll
        for (int i = 0; i < NB; ++i) dsum += (gf[i].x * of[i].x + gf[i].y * of[i].y) + (gf[i].z * of[i].z + gf[i].w * of[i].w);
        dsum = lk_sum(dsum);                   // the four lane groups hold the four quarters of the channels of query ln
        f32x4 s[NCB];
        float mx, inv;
        query_scores<NCB, D>(sK, qf, bias ? bias + (size_t)(slab * 16 + ln) * T + lk * 4 : nullptr, scale, NCB, lk, ln, s, mx, inv);
        if (lk == 0) st[slab * 16 + ln] = make_float4(mx, inv, dsum, 0.f);
        // ---- per key tile: dP^T = V dO^T, dS^T = P^T o (dP^T - D), dQ^T += K^T dS^T ----------------------------------------------
        f32x4 dq[NB];
        zero_tiles(dq);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const f32x4 dp = row_tile<D>(sV, cb, lk, ln, gf);
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[r] = s[cb][r] * inv * (dp[r] - dsum);
            if (gbias) {
                float* gb = gbias + (size_t)(slab * 16 + ln) * T + cb * 16 + lk * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) atomicAdd(gb + r, ds[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) col_accumulate<D>(sK, cb, r, lk, ln, ds[r], dq);
            if constexpr (NCB >= 16) __builtin_amdgcn_sched_barrier(0);
        }
        store_tiles(gqkv + qpix * C3 + (size_t)h * D + lk * 4, dq, scale);
    }
}

template <int WS, int D>
__global__ __launch_bounds__(64 * wattn_waves<WS>()) void k_window_attn_bwd_kv(
    const float* __restrict__ qkv, const float* __restrict__ bias, const float* __restrict__ gout, int H, int W, int m,
    float scale, const float4* __restrict__ stats, float* __restrict__ gqkv) {
    constexpr int T = WS * WS, NCB = T / 16, NB = D / 16, NW = wattn_waves<WS>();
    constexpr int STR = D + 4;
    __shared__ __attribute__((aligned(16))) float sQ[T * STR];
    __shared__ __attribute__((aligned(16))) float sG[T * STR];
    __shared__ float4 sSt[T];
    const int nww = W / WS;
    const int ih = blockIdx.x / nww, iw = blockIdx.x - ih * nww, h = blockIdx.y, l = blockIdx.z;
    const WindowTokens<WS> tok{ih, iw, W};
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const size_t apix = (size_t)l * H * W;               // first pixel of this agent's map
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    stage_rows<D, 64 * NW>(tok, T, qkv + apix * C3 + (size_t)h * D, C3, gout + apix * MD + (size_t)h * D, MD, sQ, sG);
    {
        const float4* st = stats + (((size_t)l * gridDim.x + blockIdx.x) * m + h) * T;
        for (int t = threadIdx.x; t < T; t += 64 * NW) sSt[t] = st[t];
    }
    __syncthreads();
    for (int slab = wave; slab < T / 16; slab += NW) {
        const size_t krow = (apix + tok(slab * 16 + ln)) * C3 + MD + (size_t)h * D;      // this lane's KEY; its value at + MD
        float4 kf[NB], vf[NB];
        load_frag<D>(qkv + krow, lk, kf);
        load_frag<D>(qkv + krow + MD, lk, vf);
        f32x4 dk[NB], dv[NB];
        zero_tiles(dk);
        zero_tiles(dv);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const f32x4 sc = row_tile<D>(sQ, cb, lk, ln, kf), dp = row_tile<D>(sG, cb, lk, ln, vf);
            f32x4 pr, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = cb * 16 + lk * 4 + r;
                const float4 stq = sSt[q];                               // (max, 1 / sum, D) of query q
                const float bv = bias ? bias[slab * 16 + ln + (size_t)q * T] : 0.f;
                pr[r] = expf(sc[r] * scale + bv - stq.x) * stq.y;
                ds[r] = pr[r] * (dp[r] - stq.z);
            }
            key_tile_accumulate<D, true>(sQ, sG, cb, lk, ln, pr, ds, dk, dv);
            if constexpr (NCB >= 16) __builtin_amdgcn_sched_barrier(0);
        }
        store_tiles(gqkv + krow + lk * 4, dk, scale);
        store_tiles(gqkv + krow + MD + lk * 4, dv, 1.f);
    }
}

}  // namespace heal

using namespace heal;

// the (window, dim_head) instantiations
#define HEAL_WATTN_SHAPES(X) X(4, 16) X(8, 32) X(16, 64) X(4, 32) X(8, 16) X(8, 64) X(4, 64)

extern "C" int heal_window_attention(const float* qkv, const float* pos_bias, int n_agents, int H, int W, int heads,
                                     int dim_head, int window, float scale, float* out, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && heads >= 1 && H >= 1 && W >= 1, "window_attention: bad shape");
    HEAL_REQUIRE(H % window == 0 && W % window == 0, "window_attention: H, W must be multiples of the window size");
    HEAL_REQUIRE(heads <= 65535 && n_agents <= 65535, "window_attention: too many heads / agents for the grid");
    HEAL_REQUIRE(qkv && out, "window_attention: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((H / window) * (W / window), heads, n_agents);
#define HEAL_WA(WS_, D_)                                                                                        \
    if (window == WS_ && dim_head == D_) {                                                                      \
        constexpr int NW_ = wattn_waves<WS_>();                                                                  \
        k_window_attn<WS_, D_><<<grid, 64 * NW_, 0, s>>>(qkv, pos_bias, H, W, heads, scale, out);               \
        HEAL_LAUNCH_CHECK();                                                                                    \
        return 0;                                                                                               \
    }
    HEAL_WATTN_SHAPES(HEAL_WA)
#undef HEAL_WA
    return set_error("window_attention: window %d with dim_head %d is not instantiated", window, dim_head);
}

extern "C" size_t heal_window_attention_backward_workspace(int n_agents, int H, int W, int heads) {
    return (size_t)n_agents * H * W * heads * sizeof(float4) + 256;
}

extern "C" int heal_window_attention_backward(const float* qkv, const float* pos_bias, const float* out, const float* grad_out,
                                              int n_agents, int H, int W, int heads, int dim_head, int window, float scale,
                                              float* grad_qkv, float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && heads >= 1 && H >= 1 && W >= 1, "window_attention_backward: bad shape");
    HEAL_REQUIRE(H % window == 0 && W % window == 0, "window_attention_backward: H, W must be multiples of the window size");
    HEAL_REQUIRE(heads <= 65535 && n_agents <= 65535, "window_attention_backward: too many heads / agents for the grid");
    HEAL_REQUIRE(qkv && out && grad_out && grad_qkv, "window_attention_backward: null pointer");
    HEAL_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= heal_window_attention_backward_workspace(n_agents, H, W, heads),
                 "window_attention_backward: workspace too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((H / window) * (W / window), heads, n_agents);
    float4* stats = reinterpret_cast<float4*>(ws);
#define HEAL_WAB(WS_, D_)                                                                                                     \
    if (window == WS_ && dim_head == D_) {                                                                                    \
        constexpr int NW_ = wattn_waves<WS_>();                                                                                \
        k_window_attn_bwd_q<WS_, D_><<<grid, 64 * NW_, 0, s>>>(qkv, pos_bias, out, grad_out, H, W, heads, scale, grad_qkv,     \
                                                              grad_bias, stats);                                             \
        k_window_attn_bwd_kv<WS_, D_><<<grid, 64 * NW_, 0, s>>>(qkv, pos_bias, grad_out, H, W, heads, scale, stats, grad_qkv); \
        HEAL_LAUNCH_CHECK();                                                                                                  \
        return 0;                                                                                                             \
    }
    HEAL_WATTN_SHAPES(HEAL_WAB)
#undef HEAL_WAB
    return set_error("window_attention_backward: window %d with dim_head %d is not instantiated", window, dim_head);
}
