// BatchNorm2d (+ residual) (+ ReLU) of the gradient path: batch statistics, the fused apply and its backward as streaming kernels.
//
// The composition bn(x) (+ residual) -> relu is three library operators forward and three autograd nodes backward; here it is
//   heal_bn_stats         1 read of x                                  (+ a C-block finish kernel)
//   heal_bn_act_forward   1 read of x (+ residual), 1 write of y
//   heal_bn_act_backward  reduce: reads dy, x (, y)  (+ finish);  apply: reads dy, x (, y), writes dx (, dresidual)
//
// Work decomposition (all three): the [n, C, HW] map is cut into SEGMENTS, contiguous runs of at most BN_SEG elements of one
// (sample, channel) plane; segment g = plane * spp + j, plane = sample * C + channel, spp = ceil(HW / BN_SEG).  A 256-thread block
// takes whole segments g = blockIdx.x, + gridDim.x, ...; inside a segment thread t owns the 16-byte groups t, t + 256, ... (or the
// single elements, on the dword path), so WHICH thread adds WHICH element depends on the segment alone.  The per-channel values
// (mean, rstd, gamma, ...) are uniform over a segment.
//
// Reductions: every thread accumulates in fp64, the 64 lanes of a wave are added by an xor tree, the four waves in wave order, and
// the pair of sums is stored at partial[g].  k_bn_*_finish (one block per channel) adds the n * spp partials of its channel:
// thread t those with index t, t + 256, ... in order, then a fixed LDS tree.  No floating-point atomics; nothing depends on the
// grid size or on an address, so repeated launches are bit-equal.  The partials are written before they are read: the workspace
// need not be initialised.
//
// Arithmetic (the library is built with -ffp-contract=off: every fp32 operation below is rounded on its own, in this order):
//   stats     d = (double)x - (double)K_c, S1 += d, S2 += d * d;  mean = K_c + S1 / M, var = max(S2 / M - (S1 / M)^2, 0),
//             rstd = 1 / sqrt(var + eps), all fp64, each result rounded once
//   forward   xh = (x - mean) * rstd;  z = xh * gamma + beta (+ residual);  y = relu ? max(z, 0) : z
//   backward  dz = relu ? (y > 0 ? dy : 0) : dy;  xh as above;  SB += (double)dz, SG += (double)dz * (double)xh;
//             m1 = (float)(SB / M), m2 = (float)(SG / M);  dx = (gamma * rstd) * ((dz - m1) - xh * m2)   [batch statistics]
//             dx = (gamma * rstd) * dz                                                                  [frozen statistics]
#include "common.h"
#include "../../include/heal_amd_train_bn.h"

namespace heal {

constexpr int BN_SEG = HEAL_BN_SEGMENT;
constexpr int BN_THREADS = 256;
constexpr int BN_DEFAULT_BLOCKS = 2048;
static_assert(BN_SEG % (4 * BN_THREADS) == 0, "a full segment is a whole number of 16-byte groups per thread");

static int g_bn_max_blocks = BN_DEFAULT_BLOCKS;

struct BnSeg { size_t base; int len; int c; };

// segment g -> (offset of its first element, its length, its channel)
__device__ __forceinline__ BnSeg bn_segment(long long g, int C, int HW, int spp) {
    const long long plane = g / spp;
    const int j = (int)(g - plane * spp);
    BnSeg s;
    s.base = (size_t)plane * (size_t)HW + (size_t)j * BN_SEG;
    s.len = min(BN_SEG, HW - j * BN_SEG);
    s.c = (int)(plane % C);
    return s;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (a, b) summed over the block: lanes by an xor tree, the waves in wave order; thread 0 stores the pair.  `red` is reused by the
// next segment of the grid-stride loop, hence the trailing barrier.
__device__ __forceinline__ void bn_block_store2(double a, double b, double (*red)[2], double* __restrict__ dst) {
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = red[0][0], sb = red[0][1];
#pragma unroll
        for (int w = 1; w < BN_THREADS / 64; ++w) { sa += red[w][0]; sb += red[w][1]; }
        dst[0] = sa;
        dst[1] = sb;
    }
    __syncthreads();
}

// the n * spp partial pairs of channel c, added in (sample, segment) order: thread t takes p = t, t + 256, ...; result in thread 0
__device__ __forceinline__ void bn_channel_sum2(const double* __restrict__ partial, int n, int C, int spp, int c, double (*red)[2],
                                                double& a, double& b) {
    const long long count = (long long)n * spp;
    double va = 0.0, vb = 0.0;
    for (long long p = threadIdx.x; p < count; p += BN_THREADS) {
        const long long s = p / spp, j = p - s * spp;
        const double* q = partial + 2 * ((s * C + c) * spp + j);
        va += q[0];
        vb += q[1];
    }
    red[threadIdx.x][0] = va;
    red[threadIdx.x][1] = vb;
    __syncthreads();
    for (int o = BN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[threadIdx.x][0] += red[threadIdx.x + o][0];
            red[threadIdx.x][1] += red[threadIdx.x + o][1];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[0][1];
}

// ---------------------------------------------------------------------------------------------------------------- statistics
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void k_bn_stats(const float* __restrict__ x, int C, int HW, int spp, long long segs,
                                                         double* __restrict__ partial) {
    __shared__ double red[BN_THREADS / 64][2];
    for (long long g = blockIdx.x; g < segs; g += gridDim.x) {
        const BnSeg s = bn_segment(g, C, HW, spp);
        const double K = (double)x[(size_t)s.c * HW];
        const float* __restrict__ p = x + s.base;
        double s1 = 0.0, s2 = 0.0;
        if (VEC) {
#pragma unroll 4
            for (int i = threadIdx.x * 4; i < s.len; i += BN_THREADS * 4) {
                const float4 v = *reinterpret_cast<const float4*>(p + i);
                const double d0 = (double)v.x - K, d1 = (double)v.y - K, d2 = (double)v.z - K, d3 = (double)v.w - K;
                s1 += d0; s2 += d0 * d0;
                s1 += d1; s2 += d1 * d1;
                s1 += d2; s2 += d2 * d2;
                s1 += d3; s2 += d3 * d3;
            }
        } else {
#pragma unroll 4
            for (int i = threadIdx.x; i < s.len; i += BN_THREADS) {
                const double d = (double)p[i] - K;
                s1 += d; s2 += d * d;
            }
        }
        bn_block_store2(s1, s2, red, partial + 2 * g);
    }
}

__global__ __launch_bounds__(BN_THREADS) void k_bn_stats_finish(const float* __restrict__ x, const double* __restrict__ partial,
                                                                int n, int C, int HW, int spp, double eps, double momentum,
                                                                float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                                float* __restrict__ running_mean, float* __restrict__ running_var) {
    __shared__ double red[BN_THREADS][2];
    const int c = blockIdx.x;
    double s1, s2;
    bn_channel_sum2(partial, n, C, spp, c, red, s1, s2);
    if (threadIdx.x == 0) {
        const double M = (double)n * (double)HW;
        const double K = (double)x[(size_t)c * HW];
        const double m = s1 / M;
        const double mean = K + m;
        double var = s2 / M - m * m;
        var = var > 0.0 ? var : 0.0;
        save_mean[c] = (float)mean;
        save_rstd[c] = (float)(1.0 / sqrt(var + eps));
        if (running_mean != nullptr) {
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * (M / (M - 1.0))));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- forward
__device__ __forceinline__ float bn_fwd1(float x, float mean, float rstd, float gamma, float beta, bool has_res, float r, bool relu) {
    const float xh = (x - mean) * rstd;
    float z = xh * gamma + beta;
    if (has_res) z = z + r;
    return relu ? fmaxf(z, 0.f) : z;
}

template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void k_bn_act_forward(const float* __restrict__ x, const float* __restrict__ residual,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               int C, int HW, int spp, long long segs, int relu_i,
                                                               float* __restrict__ y) {
    const bool relu = relu_i != 0, has_res = residual != nullptr;
    for (long long g = blockIdx.x; g < segs; g += gridDim.x) {
        const BnSeg s = bn_segment(g, C, HW, spp);
        const float mu = mean[s.c], rs = rstd[s.c], ga = gamma[s.c], be = beta[s.c];
        const float* __restrict__ px = x + s.base;
        const float* __restrict__ pr = has_res ? residual + s.base : nullptr;
        float* __restrict__ py = y + s.base;
        if (VEC) {
#pragma unroll 4
            for (int i = threadIdx.x * 4; i < s.len; i += BN_THREADS * 4) {
                const float4 v = *reinterpret_cast<const float4*>(px + i);
                float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                if (has_res) r = *reinterpret_cast<const float4*>(pr + i);
                float4 o;
                o.x = bn_fwd1(v.x, mu, rs, ga, be, has_res, r.x, relu);
                o.y = bn_fwd1(v.y, mu, rs, ga, be, has_res, r.y, relu);
                o.z = bn_fwd1(v.z, mu, rs, ga, be, has_res, r.z, relu);
                o.w = bn_fwd1(v.w, mu, rs, ga, be, has_res, r.w, relu);
                *reinterpret_cast<float4*>(py + i) = o;
            }
        } else {
#pragma unroll 4
            for (int i = threadIdx.x; i < s.len; i += BN_THREADS)
                py[i] = bn_fwd1(px[i], mu, rs, ga, be, has_res, has_res ? pr[i] : 0.f, relu);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ float bn_dz(float dy, bool relu, float y) { return relu ? (y > 0.f ? dy : 0.f) : dy; }

template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_reduce(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ y, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, int C, int HW, int spp, long long segs,
                                                              double* __restrict__ partial) {
    __shared__ double red[BN_THREADS / 64][2];
    const bool relu = y != nullptr;
    for (long long g = blockIdx.x; g < segs; g += gridDim.x) {
        const BnSeg s = bn_segment(g, C, HW, spp);
        const float mu = mean[s.c], rs = rstd[s.c];
        const float* __restrict__ pd = dy + s.base;
        const float* __restrict__ px = x + s.base;
        const float* __restrict__ py = relu ? y + s.base : nullptr;
        double sb = 0.0, sg = 0.0;
        if (VEC) {
#pragma unroll 4
            for (int i = threadIdx.x * 4; i < s.len; i += BN_THREADS * 4) {
                const float4 d = *reinterpret_cast<const float4*>(pd + i);
                const float4 v = *reinterpret_cast<const float4*>(px + i);
                float4 o = make_float4(1.f, 1.f, 1.f, 1.f);
                if (relu) o = *reinterpret_cast<const float4*>(py + i);
                const float z0 = bn_dz(d.x, relu, o.x), z1 = bn_dz(d.y, relu, o.y), z2 = bn_dz(d.z, relu, o.z), z3 = bn_dz(d.w, relu, o.w);
                sb += (double)z0; sg += (double)z0 * (double)((v.x - mu) * rs);
                sb += (double)z1; sg += (double)z1 * (double)((v.y - mu) * rs);
                sb += (double)z2; sg += (double)z2 * (double)((v.z - mu) * rs);
                sb += (double)z3; sg += (double)z3 * (double)((v.w - mu) * rs);
            }
        } else {
#pragma unroll 4
            for (int i = threadIdx.x; i < s.len; i += BN_THREADS) {
                const float z = bn_dz(pd[i], relu, relu ? py[i] : 1.f);
                sb += (double)z; sg += (double)z * (double)((px[i] - mu) * rs);
            }
        }
        bn_block_store2(sb, sg, red, partial + 2 * g);
    }
}

// coef[c] = m1 = (float)(sum dz / M), coef[C + c] = m2 = (float)(sum dz xh / M): what the apply kernel subtracts
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_finish(const double* __restrict__ partial, int n, int C, int HW, int spp,
                                                              float* __restrict__ coef, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
    __shared__ double red[BN_THREADS][2];
    const int c = blockIdx.x;
    double sb, sg;
    bn_channel_sum2(partial, n, C, spp, c, red, sb, sg);
    if (threadIdx.x == 0) {
        const double M = (double)n * (double)HW;
        coef[c] = (float)(sb / M);
        coef[C + c] = (float)(sg / M);
        if (dbeta != nullptr) dbeta[c] = (float)sb;
        if (dgamma != nullptr) dgamma[c] = (float)sg;
    }
}

__device__ __forceinline__ float bn_dx1(float dz, float x, float mu, float rs, float a, bool batch, float m1, float m2) {
    if (!batch) return a * dz;
    const float xh = (x - mu) * rs;
    return a * ((dz - m1) - xh * m2);
}

template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ coef, int C, int HW, int spp, long long segs,
                                                             int batch_i, float* __restrict__ dx, float* __restrict__ dres) {
    // coef exists only when the reduction ran: it is read for dx with batch statistics and for nothing else (a call that asks for
    // dresidual alone gets coef == nullptr)
    const bool relu = y != nullptr, want_dx = dx != nullptr, want_dr = dres != nullptr, batch = batch_i != 0 && want_dx;
    for (long long g = blockIdx.x; g < segs; g += gridDim.x) {
        const BnSeg s = bn_segment(g, C, HW, spp);
        const float mu = mean[s.c], rs = rstd[s.c];
        const float a = gamma[s.c] * rs;
        const float m1 = batch ? coef[s.c] : 0.f, m2 = batch ? coef[C + s.c] : 0.f;
        const float* __restrict__ pd = dy + s.base;
        const float* __restrict__ px = x + s.base;
        const float* __restrict__ py = relu ? y + s.base : nullptr;
        float* __restrict__ pdx = want_dx ? dx + s.base : nullptr;
        float* __restrict__ pdr = want_dr ? dres + s.base : nullptr;
        const bool need_x = batch;
        if (VEC) {
#pragma unroll 4
            for (int i = threadIdx.x * 4; i < s.len; i += BN_THREADS * 4) {
                const float4 d = *reinterpret_cast<const float4*>(pd + i);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f), o = make_float4(1.f, 1.f, 1.f, 1.f);
                if (need_x) v = *reinterpret_cast<const float4*>(px + i);
                if (relu) o = *reinterpret_cast<const float4*>(py + i);
                float4 z;
                z.x = bn_dz(d.x, relu, o.x); z.y = bn_dz(d.y, relu, o.y); z.z = bn_dz(d.z, relu, o.z); z.w = bn_dz(d.w, relu, o.w);
                if (want_dr) *reinterpret_cast<float4*>(pdr + i) = z;
                if (want_dx) {
                    float4 r;
                    r.x = bn_dx1(z.x, v.x, mu, rs, a, batch, m1, m2);
                    r.y = bn_dx1(z.y, v.y, mu, rs, a, batch, m1, m2);
                    r.z = bn_dx1(z.z, v.z, mu, rs, a, batch, m1, m2);
                    r.w = bn_dx1(z.w, v.w, mu, rs, a, batch, m1, m2);
                    *reinterpret_cast<float4*>(pdx + i) = r;
                }
            }
        } else {
#pragma unroll 4
            for (int i = threadIdx.x; i < s.len; i += BN_THREADS) {
                const float z = bn_dz(pd[i], relu, relu ? py[i] : 1.f);
                if (want_dr) pdr[i] = z;
                if (want_dx) pdx[i] = bn_dx1(z, need_x ? px[i] : 0.f, mu, rs, a, batch, m1, m2);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- host
struct BnPlan { int spp; long long segs; unsigned blocks; size_t partial_bytes, coef_bytes; };

static bool bn_plan(int n, int C, int HW, BnPlan* p) {
    if (n < 1 || C < 1 || HW < 1 || HW > (1 << 30)) return false;
    const long long spp = ((long long)HW + BN_SEG - 1) / BN_SEG;
    const long long planes = (long long)n * C;
    if (planes > (1LL << 30) || planes * spp > (1LL << 30)) return false;
    p->spp = (int)spp;
    p->segs = planes * spp;
    p->blocks = (unsigned)(p->segs < g_bn_max_blocks ? p->segs : g_bn_max_blocks);
    p->partial_bytes = align_up((size_t)p->segs * 2 * sizeof(double));
    p->coef_bytes = align_up((size_t)C * 2 * sizeof(float));
    return true;
}

static bool bn_aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

}  // namespace heal

using namespace heal;

extern "C" int heal_bn_train_supported(int n, int C, int HW) {
    BnPlan p;
    return bn_plan(n, C, HW, &p) ? 1 : 0;
}

extern "C" size_t heal_bn_train_workspace(int n, int C, int HW) {
    BnPlan p;
    if (!bn_plan(n, C, HW, &p)) return 0;
    return p.partial_bytes + p.coef_bytes;
}

extern "C" int heal_bn_train_max_blocks(int blocks) {
    const int before = g_bn_max_blocks;
    g_bn_max_blocks = blocks >= 1 ? blocks : BN_DEFAULT_BLOCKS;
    return before;
}

extern "C" int heal_bn_stats(const float* x, int n, int C, int HW, double eps, double momentum, float* save_mean, float* save_rstd,
                             float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BnPlan p;
    HEAL_REQUIRE(bn_plan(n, C, HW, &p), "bn_stats: unsupported shape [%d, %d, %d] (heal_bn_train_supported)", n, C, HW);
    HEAL_REQUIRE(x != nullptr && save_mean != nullptr && save_rstd != nullptr, "bn_stats: x, save_mean and save_rstd must be set");
    HEAL_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_stats: running_mean and running_var go together");
    HEAL_REQUIRE(running_mean == nullptr || (long long)n * HW >= 2, "bn_stats: the unbiased variance needs n * HW >= 2");
    HEAL_REQUIRE(eps >= 0.0, "bn_stats: eps must not be negative");
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= p.partial_bytes, "bn_stats: workspace of %zu bytes, need %zu (heal_bn_train_workspace)",
                 ws_bytes, p.partial_bytes);
    HEAL_REQUIRE(((uintptr_t)ws & 7u) == 0, "bn_stats: the workspace must be 8-byte aligned");
    double* partial = (double*)ws;
    const dim3 grid(p.blocks), block(BN_THREADS);
    const LaunchEvents ev = take_launch_events();
    if (HW % 4 == 0 && bn_aligned16(x))
        HEAL_LAUNCH_EV2(k_bn_stats<true>, grid, block, 0, s, ev.start, nullptr, x, C, HW, p.spp, p.segs, partial);
    else
        HEAL_LAUNCH_EV2(k_bn_stats<false>, grid, block, 0, s, ev.start, nullptr, x, C, HW, p.spp, p.segs, partial);
    HEAL_LAUNCH_CHECK();
    HEAL_LAUNCH_EV2(k_bn_stats_finish, dim3((unsigned)C), block, 0, s, nullptr, ev.stop, x, (const double*)partial, n, C, HW, p.spp, eps,
                    momentum, save_mean, save_rstd, running_mean, running_var);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" int heal_bn_act_forward(const float* x, const float* residual, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, int n, int C, int HW, int relu, float* y, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BnPlan p;
    HEAL_REQUIRE(bn_plan(n, C, HW, &p), "bn_act_forward: unsupported shape [%d, %d, %d] (heal_bn_train_supported)", n, C, HW);
    HEAL_REQUIRE(x != nullptr && mean != nullptr && rstd != nullptr && gamma != nullptr && beta != nullptr && y != nullptr,
                 "bn_act_forward: x, mean, rstd, gamma, beta and y must be set");
    const dim3 grid(p.blocks), block(BN_THREADS);
    if (HW % 4 == 0 && bn_aligned16(x) && bn_aligned16(residual) && bn_aligned16(y))
        HEAL_LAUNCH_EV(k_bn_act_forward<true>, grid, block, 0, s, x, residual, mean, rstd, gamma, beta, C, HW, p.spp, p.segs, relu, y);
    else
        HEAL_LAUNCH_EV(k_bn_act_forward<false>, grid, block, 0, s, x, residual, mean, rstd, gamma, beta, C, HW, p.spp, p.segs, relu, y);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" int heal_bn_act_backward(const float* dy, const float* x, const float* y, const float* mean, const float* rstd,
                                    const float* gamma, int n, int C, int HW, int relu, int batch_stats, float* dx, float* dresidual,
                                    float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BnPlan p;
    HEAL_REQUIRE(bn_plan(n, C, HW, &p), "bn_act_backward: unsupported shape [%d, %d, %d] (heal_bn_train_supported)", n, C, HW);
    HEAL_REQUIRE(dy != nullptr && x != nullptr && mean != nullptr && rstd != nullptr && gamma != nullptr,
                 "bn_act_backward: dy, x, mean, rstd and gamma must be set");
    HEAL_REQUIRE((relu != 0) == (y != nullptr), "bn_act_backward: y (the forward's result) is required exactly when relu is set");
    const bool batch = batch_stats != 0;
    const bool reduce = dgamma != nullptr || dbeta != nullptr || (batch && dx != nullptr);
    const bool apply = dx != nullptr || dresidual != nullptr;
    const bool vec = HW % 4 == 0 && bn_aligned16(dy) && bn_aligned16(x) && bn_aligned16(y) && bn_aligned16(dx) && bn_aligned16(dresidual);
    const dim3 grid(p.blocks), block(BN_THREADS);
    float* coef = nullptr;
    const LaunchEvents ev = take_launch_events();
    if (reduce) {
        HEAL_REQUIRE(ws != nullptr && ws_bytes >= p.partial_bytes + p.coef_bytes,
                     "bn_act_backward: workspace of %zu bytes, need %zu (heal_bn_train_workspace)", ws_bytes,
                     p.partial_bytes + p.coef_bytes);
        HEAL_REQUIRE(((uintptr_t)ws & 7u) == 0, "bn_act_backward: the workspace must be 8-byte aligned");
        double* partial = (double*)ws;
        coef = (float*)((char*)ws + p.partial_bytes);
        if (vec)
            HEAL_LAUNCH_EV2(k_bn_bwd_reduce<true>, grid, block, 0, s, ev.start, nullptr, dy, x, y, mean, rstd, C, HW, p.spp, p.segs, partial);
        else
            HEAL_LAUNCH_EV2(k_bn_bwd_reduce<false>, grid, block, 0, s, ev.start, nullptr, dy, x, y, mean, rstd, C, HW, p.spp, p.segs, partial);
        HEAL_LAUNCH_CHECK();
        HEAL_LAUNCH_EV2(k_bn_bwd_finish, dim3((unsigned)C), block, 0, s, nullptr, apply ? nullptr : ev.stop, (const double*)partial, n, C,
                        HW, p.spp, coef, dgamma, dbeta);
        HEAL_LAUNCH_CHECK();
    }
    if (apply) {
        hipEvent_t e0 = reduce ? nullptr : ev.start;
        if (vec)
            HEAL_LAUNCH_EV2(k_bn_bwd_apply<true>, grid, block, 0, s, e0, ev.stop, dy, x, y, mean, rstd, gamma, (const float*)coef, C, HW,
                            p.spp, p.segs, batch_stats, dx, dresidual);
        else
            HEAL_LAUNCH_EV2(k_bn_bwd_apply<false>, grid, block, 0, s, e0, ev.stop, dy, x, y, mean, rstd, gamma, (const float*)coef, C, HW,
                            p.spp, p.segs, batch_stats, dx, dresidual);
        HEAL_LAUNCH_CHECK();
    }
    return 0;
}
