// Backward of the masked agent-window attention of CoBEVT's swap fusion (swap_attn.hip; include/heal_amd_train_attn.h): per group of
// T = 16 L tokens and per head, with P = softmax(scale Q K^T + bias[h]) over the keys of the valid agents,
//     dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(dO o O)),  dQ = scale dS K,  dK = scale dS^T Q,  dbias[h] = sum_groups dS.
// The row term rowsum(dO o O) = sum_j P_j dP_j is formed in that second way, from the recomputed tiles: it is then the P-weighted mean
// of the very dP values it is subtracted from (the rows of dS sum to zero to rounding, as in the library's softmax backward), and the
// forward's output is neither saved nor read.
// One block per (part, head) walks the groups of its part with one wave per agent and Q / K / V / dO of the group in LDS:
//   phase 1, query-owned (the forward's scheme): wave l holds the 16 queries of agent l, recomputes S^T = K Q^T tile by tile, forms
//     dP^T = V dO^T per key tile, keeps (max, 1 / sum, sum_j P_j dP_j) of its queries in LDS, forms dS^T, adds dS^T to its share of dbias (registers,
//     the forward's s[cb] layout) and accumulates dQ^T += K^T dS^T;
//   phase 2, key-owned (the tile body of k_window_attn_bwd_kv: row_tile, key_tile_accumulate): wave l < n_valid holds the 16 keys of agent l, rebuilds the
//     P / dS tiles of every query tile from the statistics and accumulates dV^T += dO^T P and dK^T += Q^T dS; wave l >= n_valid writes
//     the zeros of its masked agent's dK / dV rows.
// A masked agent is a whole 16-key tile that is neither staged nor multiplied.  Every token belongs to one group: plain stores only.
// dbias leaves the block once, as a partial of its part; k_sum_parts adds the partials in part order (no atomics: bit-equal runs).
// The MFMA scheme and the blocks both phases are built from are in attn_tiles.h.
#include "attn_tiles.h"
#include "../../include/heal_amd.h"
#include "../../include/heal_amd_train_attn.h"

namespace heal {

constexpr int SWAPB_WS = 4;             // 16 tokens per agent and group (AgentGroupTokens)
constexpr int SWAPB_BLOCKS = 1024;      // blocks the parts policy aims at: a few per CU at 46 KB of LDS (L = 5) each

template <int L, int D>
constexpr size_t swapb_lds_bytes() {
    return (size_t)(4 * 16 * L * (D + 4) + 4 * 16 * L) * sizeof(float);       // sQ, sK, sV, sG at stride D + 4 and one float4 per query
}

template <int L, int D>
__global__ __launch_bounds__(64 * L) void k_agent_window_attn_bwd(
    const float* __restrict__ qkv /*[L,H,W,3,m,D]*/, const float* __restrict__ bias /*[m,T,T] or null*/,
    const float* __restrict__ gout /*[L,H,W,m*D]*/, int n_valid, int H, int W, int m,
    int grid_mode, float scale, int parts, float* __restrict__ gqkv /*[L,H,W,3,m,D]*/,
    float* __restrict__ gbias_parts /*[parts,m,T,T] (grad_bias itself for one part) or null*/) {
    constexpr int WS = SWAPB_WS, T = 16 * L, NB = D / 16;
    constexpr int STR = D + 4;                           // row stride (words) of the LDS tiles (attn_tiles.h)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sQ = lds;
    float* sK = sQ + T * STR;
    float* sV = sK + T * STR;
    float* sG = sV + T * STR;
    float4* sSt = reinterpret_cast<float4*>(sG + T * STR);      // (max, 1 / sum, sum_j P_j dP_j) of every query
    const int ngy = W / WS;
    const int G = (H / WS) * ngy;
    const int part = blockIdx.x, h = blockIdx.y;
    // contiguous range of this part: G % parts leading parts hold one group more
    const int gbase = G / parts, grem = G - gbase * parts;
    const int g0 = part * gbase + (part < grem ? part : grem);
    const int g1 = g0 + gbase + (part < grem ? 1 : 0);
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const float* qbase = qkv + (size_t)h * D;            // q of this head; k at + MD, v at + 2 MD
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    const int tq = wave * 16 + ln;                       // this lane's token: a query in phase 1, a key in phase 2
    const float* brow = bias ? bias + ((size_t)h * T + tq) * T + lk * 4 : nullptr;        // phase 1: keys cb * 16 + lk * 4 ..
    const size_t bcol = (size_t)h * T * T + tq;          // phase 2: bias[bcol + query * T]
    f32x4 db[L];
    zero_tiles(db);

    for (int g = g0; g < g1; ++g) {
        const int gx = g / ngy, gy = g - gx * ngy;
        const AgentGroupTokens tok{gx, gy, grid_mode, H, W};
        const size_t tpix = tok(tq);
        // stage Q and dO of every agent, K and V of the valid agents only (the masked key tiles are never read): one walk over the
        // tokens (two stage_rows calls, one per pair, measured 1 - 2 % slower per launch at L = 5)
        for (int e = threadIdx.x; e < T * (D / 4); e += 64 * L) {
            const int t = e / (D / 4), c4 = e - t * (D / 4);
            const size_t p = tok(t);
            const float* row = qbase + p * C3 + c4 * 4;
            *reinterpret_cast<float4*>(&sQ[t * STR + c4 * 4]) = *reinterpret_cast<const float4*>(row);
            *reinterpret_cast<float4*>(&sG[t * STR + c4 * 4]) =
                *reinterpret_cast<const float4*>(gout + p * MD + (size_t)h * D + c4 * 4);
            if (t < n_valid * 16) {
                *reinterpret_cast<float4*>(&sK[t * STR + c4 * 4]) = *reinterpret_cast<const float4*>(row + MD);
                *reinterpret_cast<float4*>(&sV[t * STR + c4 * 4]) = *reinterpret_cast<const float4*>(row + 2 * MD);
            }
        }
        __syncthreads();
        // ================= phase 1: the 16 queries of agent `wave` =====================================================================
        {
            float4 qf[NB], gf[NB];
            load_frag<D>(&sQ[tq * STR], lk, qf);
            load_frag<D>(&sG[tq * STR], lk, gf);
            f32x4 s[L];
            float mx, inv;
            query_scores<L, D>(sK, qf, brow, scale, n_valid, lk, ln, s, mx, inv);
            // ---- dP^T = V dO^T per valid key tile, and the row term D = sum_j P_j dP_j = dO . O from these same tiles: what is
            //      subtracted below is the mean of the very values it is subtracted from, so the rows of dS sum to zero to rounding --
            f32x4 dp[L];
            float dsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < L; ++cb)
                if (cb < n_valid) {
                    dp[cb] = row_tile<D>(sV, cb, lk, ln, gf);
                    dsum += (s[cb][0] * dp[cb][0] + s[cb][1] * dp[cb][1]) + (s[cb][2] * dp[cb][2] + s[cb][3] * dp[cb][3]);
                }
            dsum = lk_sum(dsum) * inv;                   // the four lane groups hold four keys of every tile of query ln
            if (lk == 0) sSt[tq] = make_float4(mx, inv, dsum, 0.f);
            // ---- per valid key tile: dS^T = P^T o (dP^T - D), dQ^T += K^T dS^T -------------------------------------------------------
            f32x4 dq[NB];
            zero_tiles(dq);
#pragma unroll
            for (int cb = 0; cb < L; ++cb)
                if (cb < n_valid) {
                    f32x4 ds;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ds[r] = s[cb][r] * inv * (dp[cb][r] - dsum);
                        db[cb][r] += ds[r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) col_accumulate<D>(sK, cb, r, lk, ln, ds[r], dq);
                }
            store_tiles(gqkv + tpix * C3 + (size_t)h * D + lk * 4, dq, scale);
        }
        __syncthreads();                                 // the statistics of every query are in LDS
        // ================= phase 2: the 16 keys of agent `wave` (queries are not masked: every agent's tile) ============================
        {
            float* gk = gqkv + tpix * C3 + MD + (size_t)h * D + lk * 4;
            if (wave < n_valid) {
                float4 kf[NB], vf[NB];
                load_frag<D>(&sK[tq * STR], lk, kf);
                load_frag<D>(&sV[tq * STR], lk, vf);
                f32x4 dk[NB], dv[NB];
                zero_tiles(dk);
                zero_tiles(dv);
#pragma unroll
                for (int cb = 0; cb < L; ++cb) {
                    const f32x4 sc = row_tile<D>(sQ, cb, lk, ln, kf), dp = row_tile<D>(sG, cb, lk, ln, vf);
                    f32x4 pr, ds;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = cb * 16 + lk * 4 + r;
                        const float4 stq = sSt[q];                               // (max, 1 / sum, D) of query q
                        const float bv = bias ? bias[bcol + (size_t)q * T] : 0.f;
                        pr[r] = expf(sc[r] * scale + bv - stq.x) * stq.y;
                        ds[r] = pr[r] * (dp[r] - stq.z);
                    }
                    key_tile_accumulate<D, false>(sQ, sG, cb, lk, ln, pr, ds, dk, dv);
                }
                store_tiles(gk, dk, scale);
                store_tiles(gk + MD, dv, 1.f);
            } else {
                // a masked agent: no query attends to its keys
                f32x4 z[NB];
                zero_tiles(z);
                store_tiles(gk, z, 1.f);
                store_tiles(gk + MD, z, 1.f);
            }
        }
        __syncthreads();                                 // the next group's staging overwrites the tiles
    }
    // ---- this part's share of dbias: db[cb][r] = sum over its groups of dS[query tq][key cb * 16 + lk * 4 + r]; zeros for masked keys ------
    if (gbias_parts) store_tiles(gbias_parts + (((size_t)part * m + h) * T + tq) * T + lk * 4, db, 1.f);
}

// out[i] = parts[0][i] + parts[1][i] + ...: the partials in part order.  One float4 per thread.
__global__ void k_sum_parts(const float4* __restrict__ parts, int n_parts, size_t n4, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 a = parts[i];
    for (int p = 1; p < n_parts; ++p) {
        const float4 v = parts[(size_t)p * n4 + i];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[i] = a;
}

template <int L, int D>
int launch_agent_window_attn_bwd(const float* qkv, const float* bias, const float* grad_out, int n_valid, int H,
                                 int W, int heads, int mode, float scale, int parts, float* grad_qkv, float* gbias_parts,
                                 hipStream_t s) {
    constexpr size_t LDS = swapb_lds_bytes<L, D>();
    static bool attr_set = false;
    if (!attr_set) {
        HEAL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agent_window_attn_bwd<L, D>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        attr_set = true;
    }
    k_agent_window_attn_bwd<L, D><<<dim3(parts, heads), 64 * L, LDS, s>>>(qkv, bias, grad_out, n_valid, H, W, heads, mode, scale,
                                                                         parts, grad_qkv, gbias_parts);
    HEAL_LAUNCH_CHECK();
    return 0;
}

}  // namespace heal

using namespace heal;

extern "C" int heal_agent_window_attention_backward_supported(int n_agents, int window, int dim_head, int H, int W) {
    return n_agents >= 1 && n_agents <= HEAL_AGENT_WINDOW_MAX_AGENTS && window == SWAPB_WS && dim_head == 32 && H >= SWAPB_WS && W >= SWAPB_WS &&
           H % SWAPB_WS == 0 && W % SWAPB_WS == 0;
}

extern "C" int heal_agent_window_attention_backward_parts(int n_agents, int H, int W, int heads) {
    if (!heal_agent_window_attention_backward_supported(n_agents, SWAPB_WS, 32, H, W) || heads < 1 || heads > 65535) return 0;
    const long long G = (long long)(H / SWAPB_WS) * (W / SWAPB_WS);
    const long long want = SWAPB_BLOCKS / heads > 1 ? SWAPB_BLOCKS / heads : 1;
    return (int)(G < want ? G : want);
}

extern "C" size_t heal_agent_window_attention_backward_workspace(int n_agents, int H, int W, int heads, int parts) {
    const int policy = heal_agent_window_attention_backward_parts(n_agents, H, W, heads);
    if (policy == 0 || parts < 0 || (long long)parts > (long long)(H / SWAPB_WS) * (W / SWAPB_WS)) return 0;
    if (parts == 0) parts = policy;
    const size_t T = (size_t)16 * n_agents;
    return parts > 1 ? (size_t)parts * heads * T * T * sizeof(float) : 0;
}

extern "C" int heal_agent_window_attention_backward(const float* qkv, const float* bias, const float* grad_out,
                                                    int n_agents, int n_valid, int H, int W, int heads, int dim_head, int window,
                                                    int mode, float scale, int parts, float* grad_qkv, float* grad_bias, void* ws,
                                                    size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && n_agents <= HEAL_AGENT_WINDOW_MAX_AGENTS, "agent_window_attention_backward: n_agents %d outside 1..%d", n_agents,
                 HEAL_AGENT_WINDOW_MAX_AGENTS);
    HEAL_REQUIRE(n_valid >= 1 && n_valid <= n_agents, "agent_window_attention_backward: n_valid %d outside 1..%d", n_valid, n_agents);
    HEAL_REQUIRE(window == SWAPB_WS, "agent_window_attention_backward: window %d is not instantiated (4 only)", window);
    HEAL_REQUIRE(dim_head == 32, "agent_window_attention_backward: dim_head %d is not instantiated (32 only)", dim_head);
    HEAL_REQUIRE(mode == 0 || mode == 1, "agent_window_attention_backward: mode must be 0 (window) or 1 (grid)");
    HEAL_REQUIRE(heads >= 1 && heads <= 65535, "agent_window_attention_backward: bad shape");
    HEAL_REQUIRE(heal_agent_window_attention_backward_supported(n_agents, window, dim_head, H, W),
                 "agent_window_attention_backward: H, W must be positive multiples of the window size");
    const long long G = (long long)(H / window) * (W / window);
    HEAL_REQUIRE(parts >= 0 && parts <= G, "agent_window_attention_backward: parts %d outside 0..%lld (the groups)", parts, G);
    if (parts == 0) parts = heal_agent_window_attention_backward_parts(n_agents, H, W, heads);
    HEAL_REQUIRE(qkv && grad_out && grad_qkv, "agent_window_attention_backward: null pointer");
    HEAL_REQUIRE((bias != nullptr) == (grad_bias != nullptr), "agent_window_attention_backward: grad_bias goes with bias");
    HEAL_REQUIRE((((uintptr_t)qkv | (uintptr_t)grad_out | (uintptr_t)grad_qkv | (uintptr_t)bias |
                   (uintptr_t)grad_bias) & 15) == 0, "agent_window_attention_backward: pointers must be 16-B aligned");
    float* gparts = grad_bias;
    if (bias && parts > 1) {
        const size_t need = heal_agent_window_attention_backward_workspace(n_agents, H, W, heads, parts);
        HEAL_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need,
                     "agent_window_attention_backward: workspace too small or misaligned");
        gparts = reinterpret_cast<float*>(ws);
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = 1;
    switch (n_agents) {
#define HEAL_AWAB(L_)                                                                                                            \
    case L_:                                                                                                                     \
        rc = launch_agent_window_attn_bwd<L_, 32>(qkv, bias, grad_out, n_valid, H, W, heads, mode, scale, parts, grad_qkv,  \
                                                  gparts, s);                                                                    \
        break;
        HEAL_AWAB(1) HEAL_AWAB(2) HEAL_AWAB(3) HEAL_AWAB(4) HEAL_AWAB(5) HEAL_AWAB(6) HEAL_AWAB(7) HEAL_AWAB(8)
#undef HEAL_AWAB
    }
    if (rc) return rc;
    if (bias && parts > 1) {
        const size_t n4 = (size_t)heads * 16 * n_agents * 16 * n_agents / 4;
        k_sum_parts<<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(reinterpret_cast<const float4*>(gparts), parts, n4,
                                                                 reinterpret_cast<float4*>(grad_bias));
        HEAL_LAUNCH_CHECK();
    }
    return 0;
}
