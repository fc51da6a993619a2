// The MFMA tile blocks shared by the windowed-attention kernels: V2X-ViT's window attention (window_attn.hip: k_window_attn,
// k_window_attn_bwd_q, k_window_attn_bwd_kv) and CoBEVT's agent-window attention (swap_attn.hip: k_agent_window_attn;
// swap_attn_bwd.hip: k_agent_window_attn_bwd).  All five compute, per group of T tokens and per head,
//     O = softmax(scale * Q K^T + bias) V,      Q, K, V [T, D]
// or its gradients, in the TRANSPOSED formulation -- no operand ever changes layout between two GEMMs.  Lane = (lk, ln) =
// (lane >> 4, lane & 15); operand rows live in LDS at row stride D + 4 words (16-B aligned; the four lane groups, four rows apart,
// fall in disjoint bank groups):
//   row tile (S^T = K Q^T, dP^T = V dO^T, and their key-owned mirrors) on v_mfma_f32_16x16x4_f32: A = 16 LDS rows, B = 16 rows held
//       in registers; both operands use the SAME permutation of the reduction index (lane group lk takes d = lk * D/4 + step), so a
//       lane's operand values of four consecutive steps are 16 contiguous bytes: ds_read_b128 / 16-B loads instead of one b32 per MFMA;
//   D layout of a row tile: lane (lk, ln) holds rows tile * 16 + lk * 4 + {0..3} of COLUMN ln -- a query's scores sit in ONE lane
//       column: scale, bias (16-B loads), softmax with two xor-shuffles (across lk) per reduction;
//   column accumulate (O^T = V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS): reduction step (tile, r) takes LDS row
//       tile * 16 + lk * 4 + r from lane group lk -- exactly register r of the row tile: the probabilities ARE the B operand;
//   D layout of the result: lane (lk, ln) holds channels nb * 16 + lk * 4 + {0..3} of column ln: one 16-B store per tile.
// The order of the floating-point operations of every output is part of the contract (the kernels are compared bit for bit).
#pragma once
#include "common.h"

namespace heal {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// ---- token -> pixel maps ------------------------------------------------------------------------------------------------------------------
// token t of window (ih, iw): row-major inside the window; pixel index inside one agent's map
template <int WS>
struct WindowTokens {
    int ih, iw, W;
    __device__ __forceinline__ size_t operator()(int t) const {
        const int y = ih * WS + t / WS, x = iw * WS + t % WS;
        return (size_t)y * W + x;
    }
};

// token t = (l, w1, w2) of agent group (gx, gy), 4 x 4 tokens per agent: a tile of every agent's map (window mode) or a dilated grid
// (grid mode); pixel index inside the [L,H,W] stack
struct AgentGroupTokens {
    int gx, gy, grid_mode, H, W;
    __device__ __forceinline__ size_t operator()(int t) const {
        const int l = t >> 4, w1 = (t >> 2) & 3, w2 = t & 3;
        const int y = grid_mode ? w1 * (H / 4) + gx : gx * 4 + w1;
        const int x = grid_mode ? w2 * (W / 4) + gy : gy * 4 + w2;
        return ((size_t)l * H + y) * W + x;
    }
};

// ---- tile primitives ----------------------------------------------------------------------------------------------------------------------
// this lane's B fragment of a row tile: d = lk * D/4 .. + D/4 - 1 of row ln; `row` points at that row (LDS or global)
template <int D>
__device__ __forceinline__ void load_frag(const float* row, int lk, float4 (&f)[D / 16]) {
#pragma unroll
    for (int i = 0; i < D / 16; ++i) f[i] = *reinterpret_cast<const float4*>(row + lk * (D / 4) + 4 * i);
}

// rows `rows` of `tok` from two sources into two LDS tiles: dst[t][:] = src[tok(t) * stride + 0 .. D - 1]
template <int D, int NTHREADS, class Tok>
__device__ __forceinline__ void stage_rows(const Tok& tok, int rows, const float* srcA, size_t strideA, const float* srcB,
                                           size_t strideB, float* dstA, float* dstB) {
    for (int e = threadIdx.x; e < rows * (D / 4); e += NTHREADS) {
        const int t = e / (D / 4), c4 = e - t * (D / 4);
        const size_t p = tok(t);
        const float4 a = *reinterpret_cast<const float4*>(srcA + p * strideA + c4 * 4);
        const float4 b = *reinterpret_cast<const float4*>(srcB + p * strideB + c4 * 4);
        *reinterpret_cast<float4*>(&dstA[t * (D + 4) + c4 * 4]) = a;
        *reinterpret_cast<float4*>(&dstB[t * (D + 4) + c4 * 4]) = b;
    }
}

// row tile: LDS rows tile * 16 .. + 15 (A) x the 16 rows of `b`, reduced over D in the order i, then .x .y .z .w
template <int D>
__device__ __forceinline__ f32x4 row_tile(const float* lds, int tile, int lk, int ln, const float4 (&b)[D / 16]) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* ap = &lds[(tile * 16 + ln) * (D + 4) + lk * (D / 4)];
#pragma unroll
    for (int i = 0; i < D / 16; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(ap + 4 * i);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[i].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[i].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[i].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[i].w, acc, 0, 0, 0);
    }
    return acc;
}

// column accumulate, reduction step (tile, r): o[nb] += LDS[(tile * 16 + lk * 4 + r) * STR + ln + 16 nb] x p
template <int D>
__device__ __forceinline__ void col_accumulate(const float* lds, int tile, int r, int lk, int ln, float p, f32x4 (&o)[D / 16]) {
    const float* ap = &lds[(tile * 16 + lk * 4 + r) * (D + 4) + ln];
#pragma unroll
    for (int nb = 0; nb < D / 16; ++nb) o[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[nb * 16], p, o[nb], 0, 0, 0);
}

template <int NB>
__device__ __forceinline__ void zero_tiles(f32x4 (&o)[NB]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// sum over the four lane groups of a column
__device__ __forceinline__ float lk_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// D layout of the result -> one 16-B store per tile; `p` = this column's row + lk * 4
template <int NB>
__device__ __forceinline__ void store_tiles(float* p, const f32x4 (&o)[NB], float scale) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        *reinterpret_cast<float4*>(p + nb * 16) = make_float4(o[nb][0] * scale, o[nb][1] * scale, o[nb][2] * scale, o[nb][3] * scale);
}

// ---- passes -------------------------------------------------------------------------------------------------------------------------------
// Query-owned scores: S^T = K Q^T over key tiles 0 .. n_tiles - 1 (block-uniform; the others stay zero and out of the softmax), scale,
// bias (`brow` = bias row of query ln + lk * 4, or null), softmax over the keys of query ln: this lane's 4 values per tile + the other
// three lane groups.  Leaves the UNNORMALISED probabilities in s[], the row maximum and 1 / sum.
template <int NCB, int D>
__device__ __forceinline__ void query_scores(const float* sK, const float4 (&qf)[D / 16], const float* brow, float scale, int n_tiles,
                                             int lk, int ln, f32x4 (&s)[NCB], float& mx, float& inv) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        if (cb < n_tiles) s[cb] = row_tile<D>(sK, cb, lk, ln, qf);
        else s[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};                      // (as an else: zero first, then overwrite, compiles the agent
                                                                       //  forward to 86-174 VGPRs instead of 46-58)
        if constexpr (NCB >= 16) __builtin_amdgcn_sched_barrier(0);   // (the scheduler hoists every tile's K reads and spills)
    }
    mx = -INFINITY;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
        if (cb < n_tiles) {
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
    for (int cb = 0; cb < NCB; ++cb)
        if (cb < n_tiles) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = expf(s[cb][r] - mx);
                s[cb][r] = e;
                sum += e;
            }
        }
    inv = 1.f / lk_sum(sum);
}

// Key-owned tile, the body of k_window_attn_bwd_kv's and of the agent backward's second phase: this lane's KEY is column ln (fragments
// kf, vf), Q and dO of every query tile are in LDS.  Per query tile cb the kernel takes
//     sc = row_tile(sQ, cb, kf),  dp = row_tile(sG, cb, vf)         lane (lk, ln) holds queries cb * 16 + lk * 4 + {0..3} of key ln
//     P = exp(scale sc + bias - max) / sum,  dS = P o (dP - D)      from the (max, 1 / sum, D) statistics of those queries
// and calls this for dV^T += dO^T P and dK^T += Q^T dS: reduction step r takes query cb * 16 + lk * 4 + r from lane group lk.
// (The P / dS lines stay in the kernels: a helper that holds their bias branch is optimised on its own before it is inlined, which
// groups the four bias loads ahead of the exponentials and costs the one-tile instantiations a wave of occupancy.)
// ALTERNATE: the MFMAs of the two accumulates alternate per channel tile, or each step's dV tiles come before its dK tiles.  Same
// results; which order runs faster is measured per kernel (profiles/attn_family_refactor_ab.json): the window kernel alternates (the
// other order: +0.3 % at the 256-token window), the agent kernel does not (alternating: +1 % with masked agents at L = 5).
template <int D, bool ALTERNATE>
__device__ __forceinline__ void key_tile_accumulate(const float* sQ, const float* sG, int cb, int lk, int ln, f32x4 pr, f32x4 ds,
                                                    f32x4 (&dk)[D / 16], f32x4 (&dv)[D / 16]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if constexpr (ALTERNATE) {
            const float* ga = &sG[(cb * 16 + lk * 4 + r) * (D + 4) + ln];
            const float* qa = &sQ[(cb * 16 + lk * 4 + r) * (D + 4) + ln];
#pragma unroll
            for (int nb = 0; nb < D / 16; ++nb) {
                dv[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[nb * 16], pr[r], dv[nb], 0, 0, 0);
                dk[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nb * 16], ds[r], dk[nb], 0, 0, 0);
            }
        } else {
            col_accumulate<D>(sG, cb, r, lk, ln, pr[r], dv);
            col_accumulate<D>(sQ, cb, r, lk, ln, ds[r], dk);
        }
    }
}

}  // namespace heal
