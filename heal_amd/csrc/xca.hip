// XCA -- cross-covariance attention of the SDTA aligner reduced to one pointwise weight per image.  Arithmetic, layouts and
// reference line numbers: include/heal_amd_align.h.
//
// The reference transposes q, k and v, materialises two F.normalize results, runs a batched matmul with K = H W, a softmax, a second
// matmul, a permute copy and the projection.  Only the d x d Gram matrix and the 2 d row norms depend on the pixels; they need one read
// of q and k:
//   k_xca_gram    grid (parts, heads, B).  The Gram tile on v_mfma_f32_16x16x4_f32 with the pixel as the reduction index, the squared
//                 norms from the same registers, one partial of d d + 2 d floats per block.
//   k_xca_finish  grid (heads, B).  Partials summed in part order, logits, softmax, W[b][:, h d : (h + 1) d] = Pw[:, head h] A.
// No atomics, no zeroed destination: every word of the workspace that is read was written by the launch before.
#include <stdlib.h>
#include "common.h"
#include "../../include/heal_amd_align.h"

namespace heal {

constexpr int XCA_THREADS = 256;
constexpr int XCA_WAVES = XCA_THREADS / HEAL_WAVE;
constexpr int XCA_STEP = 64 * XCA_WAVES;        // pixels of one block step: 64 per wave, 16 per lane group, 4 float4 per lane
constexpr int XCA_TARGET_BLOCKS = 512;          // two blocks for each of the 256 CUs

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int D>
__global__ __launch_bounds__(XCA_THREADS) void k_xca_gram(const float* __restrict__ qkv, float* __restrict__ part, int C, int N,
                                                          int range) {
    constexpr int T = D / 16, E = D * D + 2 * D;
    __shared__ float s_part[XCA_WAVES][E];
    const int p = blockIdx.x, h = blockIdx.y, b = blockIdx.z, parts = gridDim.x, heads = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int begin = p * range, end = min(begin + range, N);       // both multiples of 4: a float4 lies inside or outside
    const float* q = qkv + ((size_t)b * 3 * C + (size_t)h * D) * N;
    const float* k = q + (size_t)C * N;

    f32x4 acc[T][T][2];
    float sq[T], sk[T];
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
        sq[ti] = 0.f;
        sk[ti] = 0.f;
#pragma unroll
        for (int tj = 0; tj < T; ++tj) acc[ti][tj][0] = acc[ti][tj][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int s0 = begin; s0 < end; s0 += XCA_STEP) {                // block-uniform: every wave issues every MFMA
        const int n = s0 + 64 * wave + 16 * g;
        const bool full = s0 + XCA_STEP <= end;
        float4 qv[T][4], kv[T][4];
#pragma unroll
        for (int ti = 0; ti < T; ++ti) {
            const float* qr = q + (size_t)(16 * ti + r) * N;
            const float* kr = k + (size_t)(16 * ti + r) * N;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pix = n + 4 * u;
                if (full || pix < end) {
                    qv[ti][u] = *reinterpret_cast<const float4*>(qr + pix);
                    kv[ti][u] = *reinterpret_cast<const float4*>(kr + pix);
                } else {
                    qv[ti][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    kv[ti][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ti = 0; ti < T; ++ti) {
                const float4 a = qv[ti][u], c = kv[ti][u];
                sq[ti] = fmaf(a.x, a.x, sq[ti]); sq[ti] = fmaf(a.y, a.y, sq[ti]);
                sq[ti] = fmaf(a.z, a.z, sq[ti]); sq[ti] = fmaf(a.w, a.w, sq[ti]);
                sk[ti] = fmaf(c.x, c.x, sk[ti]); sk[ti] = fmaf(c.y, c.y, sk[ti]);
                sk[ti] = fmaf(c.z, c.z, sk[ti]); sk[ti] = fmaf(c.w, c.w, sk[ti]);
#pragma unroll
                for (int tj = 0; tj < T; ++tj) {
                    const float4 kb = kv[tj][u];
                    // two accumulators per tile: the 40-cycle dependent latency of the instruction is above its 32-cycle issue interval
                    acc[ti][tj][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, kb.x, acc[ti][tj][0], 0, 0, 0);
                    acc[ti][tj][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, kb.y, acc[ti][tj][1], 0, 0, 0);
                    acc[ti][tj][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, kb.z, acc[ti][tj][0], 0, 0, 0);
                    acc[ti][tj][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, kb.w, acc[ti][tj][1], 0, 0, 0);
                }
            }
        }
    }

    // C / D layout of the instruction: column lane & 15, row 4 (lane >> 4) + register
    float* mine = s_part[wave];
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
#pragma unroll
        for (int tj = 0; tj < T; ++tj) {
            const f32x4 v = acc[ti][tj][0] + acc[ti][tj][1];
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[(16 * ti + 4 * g + e) * D + 16 * tj + r] = v[e];
        }
        float a = sq[ti], c = sk[ti];           // the four lanes r, r + 16, r + 32, r + 48 hold one row
        a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
        c += __shfl_xor(c, 16, 64); c += __shfl_xor(c, 32, 64);
        if (g == 0) {
            mine[D * D + 16 * ti + r] = a;
            mine[D * D + D + 16 * ti + r] = c;
        }
    }
    __syncthreads();
    float* dst = part + (((size_t)b * heads + h) * parts + p) * E;
    for (int e = threadIdx.x; e < E; e += XCA_THREADS)
        dst[e] = ((s_part[0][e] + s_part[1][e]) + s_part[2][e]) + s_part[3][e];
}

template <int D>
__global__ __launch_bounds__(XCA_THREADS) void k_xca_finish(const float* __restrict__ part, const float* __restrict__ temperature,
                                                            const float* __restrict__ pw, int C, int parts,
                                                            float* __restrict__ W_out, float* __restrict__ A_out,
                                                            float* __restrict__ stats_out) {
    constexpr int E = D * D + 2 * D;
    __shared__ float s_g[E];
    __shared__ float s_a[D * D];
    const int h = blockIdx.x, b = blockIdx.y, heads = gridDim.x;
    const size_t bh = (size_t)b * heads + h;
    const float* src = part + bh * parts * E;
    for (int e = threadIdx.x; e < E; e += XCA_THREADS) {
        float s = 0.f;
        for (int p = 0; p < parts; ++p) s += src[(size_t)p * E + e];
        s_g[e] = s;
        if (stats_out) stats_out[bh * E + e] = s;
    }
    __syncthreads();
    const float temp = temperature[h];
    for (int e = threadIdx.x; e < D * D; e += XCA_THREADS) {
        const int i = e / D, j = e - i * D;
        const float nq = fmaxf(sqrtf(s_g[D * D + i]), 1e-12f), nk = fmaxf(sqrtf(s_g[D * D + D + j]), 1e-12f);
        s_a[e] = s_g[e] / (nq * nk) * temp;
    }
    __syncthreads();
    if ((int)threadIdx.x < D) {                  // one row per thread: d <= 32 terms, in index order
        float* row = s_a + threadIdx.x * D;
        float m = row[0];
        for (int j = 1; j < D; ++j) m = fmaxf(m, row[j]);
        float sum = 0.f;
        for (int j = 0; j < D; ++j) {
            const float v = expf(row[j] - m);
            row[j] = v;
            sum += v;
        }
        for (int j = 0; j < D; ++j) row[j] = row[j] / sum;
    }
    __syncthreads();
    if (A_out)
        for (int e = threadIdx.x; e < D * D; e += XCA_THREADS) A_out[bh * D * D + e] = s_a[e];
    // W[b][c][h d + j] = sum_i Pw[c][h d + i] A[i][j]
    float* W = W_out + (size_t)b * C * C;
    for (int e = threadIdx.x; e < C * D; e += XCA_THREADS) {
        const int c = e / D, j = e - c * D;
        const float* prow = pw + (size_t)c * C + h * D;
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < D; ++i) s = fmaf(prow[i], s_a[i * D + j], s);
        W[(size_t)c * C + h * D + j] = s;
    }
}

static int xca_range(int B, int heads, int N) {
    const long long images = (long long)B * heads;
    long long want = (XCA_TARGET_BLOCKS + images - 1) / images;          // parts that would fill the chip
    const long long steps = ((long long)N + XCA_STEP - 1) / XCA_STEP;
    if (want > steps) want = steps;
    if (want < 1) want = 1;
    const long long per = (steps + want - 1) / want;                      // steps of one part
    return (int)(per * XCA_STEP);
}

}  // namespace heal

using namespace heal;

extern "C" int heal_align_fused_enabled(void) {
    const char* v = getenv("HEAL_ALIGN_FUSED");
    if (v == nullptr || v[0] == 0 || (v[0] == '1' && v[1] == 0)) return 1;
    return (v[0] == '0' && v[1] == 0) ? 0 : -1;
}

extern "C" int heal_xca_supported(int C, int heads, int N) {
    if (C < 1 || heads < 1 || heads > 65535 || C % heads != 0) return 0;
    const int d = C / heads;
    if (d != 16 && d != 32) return 0;
    if (N < 64 || N % 4 != 0 || N >= (1 << 30)) return 0;          // (begin + range stays an int)
    return 1;
}

extern "C" int heal_xca_range(int B, int heads, int N) {
    if (B < 1 || B > 65535 || heads < 1 || heads > 65535 || N < 1 || N >= (1 << 30)) return 0;
    return xca_range(B, heads, N);
}

extern "C" int heal_xca_parts(int B, int heads, int N) {
    const int range = heal_xca_range(B, heads, N);
    return range ? (int)(((long long)N + range - 1) / range) : 0;
}

extern "C" size_t heal_xca_workspace(int B, int C, int heads, int N) {
    if (!heal_xca_supported(C, heads, N)) return 0;
    const int parts = heal_xca_parts(B, heads, N), d = C / heads;
    if (!parts) return 0;
    return align_up((size_t)B * heads * parts * (size_t)(d * d + 2 * d) * sizeof(float));
}

extern "C" int heal_xca_weights(const float* qkv, const float* temperature, const float* proj_w_scaled, int B, int C, int heads,
                                int N, void* ws, size_t ws_bytes, float* W_out, float* A_out, float* stats_out, void* stream) {
    HEAL_REQUIRE(heal_xca_supported(C, heads, N) && B >= 1 && B <= 65535,
                 "xca_weights: unsupported problem (B %d, C %d, heads %d, N %d): d = C / heads must be 16 or 32, N %% 4 == 0, N >= 64",
                 B, C, heads, N);
    HEAL_REQUIRE(qkv && temperature && proj_w_scaled && W_out, "xca_weights: null argument");
    HEAL_REQUIRE(((uintptr_t)qkv & 15) == 0, "xca_weights: qkv must be 16-byte aligned");
    const size_t need = heal_xca_workspace(B, C, heads, N);
    HEAL_REQUIRE(ws && ws_bytes >= need, "xca_weights: workspace too small (%zu < %zu)", ws_bytes, need);
    const int range = heal_xca_range(B, heads, N), parts = heal_xca_parts(B, heads, N), d = C / heads;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    const dim3 g1((unsigned)parts, (unsigned)heads, (unsigned)B), g2((unsigned)heads, (unsigned)B);
    const LaunchEvents ev = take_launch_events();
    if (d == 16) {
        HEAL_LAUNCH_EV2(k_xca_gram<16>, g1, dim3(XCA_THREADS), 0, st, ev.start, (hipEvent_t) nullptr, qkv, part, C, N, range);
        HEAL_LAUNCH_CHECK();
        HEAL_LAUNCH_EV2(k_xca_finish<16>, g2, dim3(XCA_THREADS), 0, st, (hipEvent_t) nullptr, ev.stop, (const float*)part, temperature,
                        proj_w_scaled, C, parts, W_out, A_out, stats_out);
    } else {
        HEAL_LAUNCH_EV2(k_xca_gram<32>, g1, dim3(XCA_THREADS), 0, st, ev.start, (hipEvent_t) nullptr, qkv, part, C, N, range);
        HEAL_LAUNCH_CHECK();
        HEAL_LAUNCH_EV2(k_xca_finish<32>, g2, dim3(XCA_THREADS), 0, st, (hipEvent_t) nullptr, ev.stop, (const float*)part, temperature,
                        proj_w_scaled, C, parts, W_out, A_out, stats_out);
    }
    HEAL_LAUNCH_CHECK();
    return 0;
}
