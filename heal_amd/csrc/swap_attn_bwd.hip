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
//   phase 2, key-owned (k_window_attn_bwd_kv's scheme): wave l < n_valid holds the 16 keys of agent l, rebuilds the P / dS tiles of every
//     query tile from the statistics and accumulates dV^T += dO^T P and dK^T += Q^T dS; wave l >= n_valid writes the zeros of its
//     masked agent's dK / dV rows.
// A masked agent is a whole 16-key tile that is neither staged nor multiplied.  Every token belongs to one group: plain stores only.
// dbias leaves the block once, as a partial of its part; k_sum_parts adds the partials in part order (no atomics: bit-equal runs).
#include "common.h"
#include "../../include/heal_amd.h"
#include "../../include/heal_amd_train_attn.h"

namespace heal {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int SWAPB_WS = 4;
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
    constexpr int WS = SWAPB_WS, T = 16 * L, NB = D / 16, DQ = D / 4;
    constexpr int STR = D + 4;                           // row stride (words): 16-B aligned; 4 STR = 16 (mod 64)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sQ = lds;
    float* sK = sQ + T * STR;
    float* sV = sK + T * STR;
    float* sG = sV + T * STR;
    float4* sSt = reinterpret_cast<float4*>(sG + T * STR);      // (max, 1 / sum, sum_j P_j dP_j) of every query
    const int ngy = W / WS, sh = H / WS, sw = W / WS;
    const int G = sh * sw;
    const int part = blockIdx.x, h = blockIdx.y;
    // contiguous range of this part: G % parts leading parts hold one group more
    const int gbase = G / parts, grem = G - gbase * parts;
    const int g0 = part * gbase + (part < grem ? part : grem);
    const int g1 = g0 + gbase + (part < grem ? 1 : 0);
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    const int tq = wave * 16 + ln;                       // this lane's token: a query in phase 1, a key in phase 2
    const float* brow = bias ? bias + ((size_t)h * T + tq) * T + lk * 4 : nullptr;        // phase 1: keys cb * 16 + lk * 4 ..
    const float* bcol = bias ? bias + (size_t)h * T * T + tq : nullptr;                   // phase 2: + query * T
    f32x4 db[L];
#pragma unroll
    for (int cb = 0; cb < L; ++cb) db[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int g = g0; g < g1; ++g) {
        const int gx = g / ngy, gy = g - gx * ngy;
        // token t = (l, w1, w2) of this group -> offset of its row (pixel-major inside agent l's map)
        auto pix = [&](int t) -> size_t {
            const int l = t >> 4, w1 = (t >> 2) & 3, w2 = t & 3;
            const int y = grid_mode ? w1 * sh + gx : gx * WS + w1;
            const int x = grid_mode ? w2 * sw + gy : gy * WS + w2;
            return ((size_t)l * H + y) * W + x;
        };
        const size_t tpix = pix(tq);
        // stage Q and dO of every agent, K and V of the valid agents only (the masked key tiles are never read)
        for (int e = threadIdx.x; e < T * (D / 4); e += 64 * L) {
            const int t = e / (D / 4), c4 = e - t * (D / 4);
            const size_t p = pix(t);
            const float* row = qkv + p * C3 + (size_t)h * D + c4 * 4;
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
            float4 qf[DQ / 4], gf[DQ / 4];
#pragma unroll
            for (int i = 0; i < DQ / 4; ++i) {
                qf[i] = *reinterpret_cast<const float4*>(&sQ[tq * STR + lk * DQ + 4 * i]);
                gf[i] = *reinterpret_cast<const float4*>(&sG[tq * STR + lk * DQ + 4 * i]);
            }
            // ---- S^T = K Q^T, scale, bias, softmax over the valid keys: the forward, normalised ------------------------------------
            f32x4 s[L];
#pragma unroll
            for (int cb = 0; cb < L; ++cb) {
                s[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (cb < n_valid) {
                    const float* kp = &sK[(cb * 16 + ln) * STR + lk * DQ];
#pragma unroll
                    for (int i = 0; i < DQ / 4; ++i) {
                        const float4 kf = *reinterpret_cast<const float4*>(kp + 4 * i);
                        s[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[i].x, s[cb], 0, 0, 0);
                        s[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[i].y, s[cb], 0, 0, 0);
                        s[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[i].z, s[cb], 0, 0, 0);
                        s[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[i].w, s[cb], 0, 0, 0);
                    }
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int cb = 0; cb < L; ++cb)
                if (cb < n_valid) {
                    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (brow) bv = *reinterpret_cast<const float4*>(brow + cb * 16);
                    s[cb][0] = s[cb][0] * scale + bv.x; s[cb][1] = s[cb][1] * scale + bv.y;
                    s[cb][2] = s[cb][2] * scale + bv.z; s[cb][3] = s[cb][3] * scale + bv.w;
                    mx = fmaxf(fmaxf(mx, fmaxf(s[cb][0], s[cb][1])), fmaxf(s[cb][2], s[cb][3]));
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int cb = 0; cb < L; ++cb)
                if (cb < n_valid) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = expf(s[cb][r] - mx);
                        s[cb][r] = e;
                        sum += e;
                    }
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.f / sum;
            // ---- dP^T = V dO^T per valid key tile, and the row term D = sum_j P_j dP_j = dO . O from these same tiles: what is
            //      subtracted below is the mean of the very values it is subtracted from, so the rows of dS sum to zero to rounding --
            f32x4 dp[L];
            float dsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < L; ++cb)
                if (cb < n_valid) {
                    dp[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const float* vp = &sV[(cb * 16 + ln) * STR + lk * DQ];
#pragma unroll
                    for (int i = 0; i < DQ / 4; ++i) {
                        const float4 vf = *reinterpret_cast<const float4*>(vp + 4 * i);
                        dp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.x, gf[i].x, dp[cb], 0, 0, 0);
                        dp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.y, gf[i].y, dp[cb], 0, 0, 0);
                        dp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.z, gf[i].z, dp[cb], 0, 0, 0);
                        dp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.w, gf[i].w, dp[cb], 0, 0, 0);
                    }
                    dsum += (s[cb][0] * dp[cb][0] + s[cb][1] * dp[cb][1]) + (s[cb][2] * dp[cb][2] + s[cb][3] * dp[cb][3]);
                }
            dsum += __shfl_xor(dsum, 16, 64);            // the four lane groups hold four keys of every tile of query ln
            dsum += __shfl_xor(dsum, 32, 64);
            dsum *= inv;
            if (lk == 0) sSt[tq] = make_float4(mx, inv, dsum, 0.f);
            // ---- per valid key tile: dS^T = P^T o (dP^T - D), dQ^T += K^T dS^T -------------------------------------------------------
            f32x4 dq[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) dq[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
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
                    for (int r = 0; r < 4; ++r) {
                        const float* kp = &sK[(cb * 16 + lk * 4 + r) * STR + ln];
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            dq[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[nb * 16], ds[r], dq[nb], 0, 0, 0);
                    }
                }
            // D layout of dQ^T: channels nb * 16 + lk * 4 + {0..3} of query ln
            float* gp = gqkv + tpix * C3 + (size_t)h * D + lk * 4;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                *reinterpret_cast<float4*>(gp + nb * 16) =
                    make_float4(dq[nb][0] * scale, dq[nb][1] * scale, dq[nb][2] * scale, dq[nb][3] * scale);
        }
        __syncthreads();                                 // the statistics of every query are in LDS
        // ================= phase 2: the 16 keys of agent `wave` ========================================================================
        {
            float* gk = gqkv + tpix * C3 + MD + (size_t)h * D + lk * 4;
            if (wave < n_valid) {
                float4 kf[DQ / 4], vf[DQ / 4];
#pragma unroll
                for (int i = 0; i < DQ / 4; ++i) {
                    kf[i] = *reinterpret_cast<const float4*>(&sK[tq * STR + lk * DQ + 4 * i]);
                    vf[i] = *reinterpret_cast<const float4*>(&sV[tq * STR + lk * DQ + 4 * i]);
                }
                f32x4 dk[NB], dv[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) { dk[nb] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[nb] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int cb = 0; cb < L; ++cb) {
                    // score and dP tiles of queries cb * 16 .. + 15 (rows) x this wave's 16 keys (columns): lane (lk, ln) holds queries
                    // cb * 16 + lk * 4 + {0..3} of key ln.  Queries are not masked: every agent's tile.
                    f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const float* qp = &sQ[(cb * 16 + ln) * STR + lk * DQ];
                    const float* gp = &sG[(cb * 16 + ln) * STR + lk * DQ];
#pragma unroll
                    for (int i = 0; i < DQ / 4; ++i) {
                        const float4 qv = *reinterpret_cast<const float4*>(qp + 4 * i);
                        const float4 gv = *reinterpret_cast<const float4*>(gp + 4 * i);
                        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qv.x, kf[i].x, sc, 0, 0, 0);
                        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qv.y, kf[i].y, sc, 0, 0, 0);
                        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qv.z, kf[i].z, sc, 0, 0, 0);
                        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qv.w, kf[i].w, sc, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gv.x, vf[i].x, dp, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gv.y, vf[i].y, dp, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gv.z, vf[i].z, dp, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gv.w, vf[i].w, dp, 0, 0, 0);
                    }
                    f32x4 pr, ds;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = cb * 16 + lk * 4 + r;
                        const float4 stq = sSt[q];                               // (max, 1 / sum, D) of query q
                        const float bv = bcol ? bcol[(size_t)q * T] : 0.f;
                        pr[r] = expf(sc[r] * scale + bv - stq.x) * stq.y;
                        ds[r] = pr[r] * (dp[r] - stq.z);
                    }
                    // dV^T += dO^T P and dK^T += Q^T dS: reduction step r takes query cb * 16 + lk * 4 + r from lane group lk
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* ga = &sG[(cb * 16 + lk * 4 + r) * STR + ln];
                        const float* qa = &sQ[(cb * 16 + lk * 4 + r) * STR + ln];
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) {
                            dv[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[nb * 16], pr[r], dv[nb], 0, 0, 0);
                            dk[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nb * 16], ds[r], dk[nb], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    *reinterpret_cast<float4*>(gk + nb * 16) =
                        make_float4(dk[nb][0] * scale, dk[nb][1] * scale, dk[nb][2] * scale, dk[nb][3] * scale);
                    *reinterpret_cast<float4*>(gk + MD + nb * 16) = make_float4(dv[nb][0], dv[nb][1], dv[nb][2], dv[nb][3]);
                }
            } else {
                // a masked agent: no query attends to its keys
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    *reinterpret_cast<float4*>(gk + nb * 16) = z;
                    *reinterpret_cast<float4*>(gk + MD + nb * 16) = z;
                }
            }
        }
        __syncthreads();                                 // the next group's staging overwrites the tiles
    }
    // ---- this part's share of dbias: db[cb][r] = sum over its groups of dS[query tq][key cb * 16 + lk * 4 + r]; zeros for masked keys ------
    if (gbias_parts) {
        float* gb = gbias_parts + (((size_t)part * m + h) * T + tq) * T + lk * 4;
#pragma unroll
        for (int cb = 0; cb < L; ++cb)
            *reinterpret_cast<float4*>(gb + cb * 16) = make_float4(db[cb][0], db[cb][1], db[cb][2], db[cb][3]);
    }
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
