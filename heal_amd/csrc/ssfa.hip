// SSFA -- the dense neck of the SECOND + SSFA detectors: the overlapping 3x3 stride-2 transposed convolution as four output-parity
// GEMMs on the fp32 matrix cores, and the two-way attention blend as one streaming pass.  Arithmetic, tiles and layouts:
// include/heal_amd_ssfa.h.
//
// Neither kernel uses atomics or a workspace; k_deconv3x3_s2 has no LDS and no barrier (a wave whose base rows lie below the map
// leaves at once), k_ssfa_blend one barrier that every thread of the block reaches.
#include <stdlib.h>
#include "common.h"
#include "../../include/heal_amd_ssfa.h"

namespace heal {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DC_THREADS = 256;
constexpr int DC_ROWS = 8;      // base rows of a block: two per wave
constexpr int DC_COLS = 16;     // base columns of a block: the N of the MFMA
constexpr int DC_CO = 32;       // output channels of a block: two 16-row tiles
constexpr int DC_KC = 8;        // input channels of a chunk: two k-steps of 4
constexpr int DC_SEG = 4;       // chunks summed in the MFMA accumulator before they are added to the total (32 channels)

struct DcOperands {
    float2 a[2][9];             // [cout tile][tap]: the two k-steps of the chunk
    float b[2][3][2];           // [k-step][input row by0 + r][column bx + dx]
};

// nine MFMAs of one cout tile x one base row x one k-step: ee, eo, oe, oo
__device__ __forceinline__ void dc_taps(f32x4 (&acc)[4], const float2 (&a)[9], int j, float x00, float x01, float x10, float x11) {
#define DC_W(t) (j == 0 ? a[t].x : a[t].y)
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(4), x00, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(5), x00, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(7), x00, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(8), x00, acc[3], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(3), x01, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(1), x10, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(6), x01, acc[3], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(2), x10, acc[3], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(DC_W(0), x11, acc[3], 0, 0, 0);
#undef DC_W
}

__global__ __launch_bounds__(DC_THREADS) void k_deconv3x3_s2(const float* __restrict__ x, const float2* __restrict__ wfrag,
                                                             const float* __restrict__ bias, const float* __restrict__ residual,
                                                             int res_channels, int cin, int cout, int H, int W, int relu,
                                                             float* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int tiles_x = (W + DC_COLS - 1) / DC_COLS;
    const int tx = blockIdx.y % tiles_x, ty = blockIdx.y / tiles_x, n = blockIdx.z;
    const int mt0 = blockIdx.x * (DC_CO / 16);
    const int by0 = ty * DC_ROWS + 2 * wave, bx = tx * DC_COLS + c;
    if (by0 >= H) return;                                           // wave-uniform; the kernel has no barrier
    const int nk = cin / DC_KC;
    const size_t plane = (size_t)H * W;

    // the six taps of the wave's three input rows: offset inside a channel plane, and whether the pixel exists
    int off[3][2];
    bool ok[3][2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            ok[r][dx] = by0 + r < H && bx + dx < W;
            off[r][dx] = ok[r][dx] ? (by0 + r) * W + bx + dx : 0;
        }
    const float* xl = x + ((size_t)n * cin + g) * plane;            // channel g of chunk 0, k-step 0
    const float2* wl = wfrag + (size_t)mt0 * nk * 9 * 64 + lane;

    auto load = [&](DcOperands& o, int kc) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 9; ++t) o.a[m][t] = wl[((size_t)(m * nk + kc) * 9 + t) * 64];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* xc = xl + (size_t)(kc * DC_KC + 4 * j) * plane;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) o.b[j][r][dx] = ok[r][dx] ? xc[off[r][dx]] : 0.f;
        }
    };

    f32x4 run[2][2][4], tot[2][2][4];                               // [cout tile][base row][parity]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int p = 0; p < 4; ++p) tot[m][rr][p] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](const DcOperands& o) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
                    dc_taps(run[m][rr], o.a[m], j, o.b[j][rr][0], o.b[j][rr][1], o.b[j][rr + 1][0], o.b[j][rr + 1][1]);
    };

    DcOperands o0, o1;
    load(o0, 0);
    for (int kc = 0; kc < nk; kc += DC_SEG) {                       // cin % 32 == 0: whole segments
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int p = 0; p < 4; ++p) run[m][rr][p] = f32x4{0.f, 0.f, 0.f, 0.f};
        load(o1, kc + 1);
        compute(o0);
        load(o0, kc + 2);
        compute(o1);
        load(o1, kc + 3);
        compute(o0);
        if (kc + DC_SEG < nk) load(o0, kc + DC_SEG);
        compute(o1);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int p = 0; p < 4; ++p) tot[m][rr][p] += run[m][rr][p];
    }

    // C / D layout of the instruction: column (pixel) lane & 15, row (channel) 4 (lane >> 4) + register
    if (bx >= W) return;
    const int Ho = 2 * H, Wo = 2 * W;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = 16 * (mt0 + m) + 4 * g + e;
            const float bv = bias ? bias[co] : 0.f;
            const bool res = co < res_channels;
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                if (by0 + rr >= H) continue;
#pragma unroll
                for (int py = 0; py < 2; ++py) {
                    float2 v = make_float2(tot[m][rr][2 * py][e] + bv, tot[m][rr][2 * py + 1][e] + bv);
                    if (relu) {
                        v.x = fmaxf(v.x, 0.f);
                        v.y = fmaxf(v.y, 0.f);
                    }
                    const size_t row = (size_t)(2 * (by0 + rr) + py) * Wo + 2 * bx;
                    if (res) {
                        const float2 rv = *reinterpret_cast<const float2*>(residual + ((size_t)n * res_channels + co) * Ho * Wo + row);
                        v.x += rv.x;
                        v.y += rv.y;
                    }
                    *reinterpret_cast<float2*>(y + ((size_t)n * cout + co) * Ho * Wo + row) = v;
                }
            }
        }
}

constexpr int BL_THREADS = 256;
constexpr int BL_GROUPS = 16;               // channel groups of a block
constexpr int BL_QUADS = 16;                // pixel quads of a block
constexpr int BL_PIX = 4 * BL_QUADS;

template <int CPT>                          // channels of a thread: C / 16
__global__ __launch_bounds__(BL_THREADS) void k_ssfa_blend(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ wa, const float* __restrict__ wb,
                                                           const float* __restrict__ ba, const float* __restrict__ bb, int HW,
                                                           float* __restrict__ out, float* __restrict__ pa_out) {
    constexpr int C = CPT * BL_GROUPS;
    __shared__ float4 s_a[BL_GROUPS][BL_QUADS + 1], s_b[BL_GROUPS][BL_QUADS + 1];
    const int q = threadIdx.x & (BL_QUADS - 1), g = threadIdx.x / BL_QUADS, n = blockIdx.y;
    const int pix = blockIdx.x * BL_PIX + 4 * q;
    const bool live = pix < HW;                                     // HW % 4 == 0: a quad lies inside or outside
    const size_t base = ((size_t)n * C + (size_t)g * CPT) * HW + pix;
    float4 va[CPT], vb[CPT];
    float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = sa;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        va[i] = live ? *reinterpret_cast<const float4*>(a + base + (size_t)i * HW) : make_float4(0.f, 0.f, 0.f, 0.f);
        vb[i] = live ? *reinterpret_cast<const float4*>(b + base + (size_t)i * HW) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const float u = wa[g * CPT + i], v = wb[g * CPT + i];
        sa.x = fmaf(u, va[i].x, sa.x); sa.y = fmaf(u, va[i].y, sa.y); sa.z = fmaf(u, va[i].z, sa.z); sa.w = fmaf(u, va[i].w, sa.w);
        sb.x = fmaf(v, vb[i].x, sb.x); sb.y = fmaf(v, vb[i].y, sb.y); sb.z = fmaf(v, vb[i].z, sb.z); sb.w = fmaf(v, vb[i].w, sb.w);
    }
    s_a[g][q] = sa;
    s_b[g][q] = sb;
    __syncthreads();
    sa = s_a[0][q];
    sb = s_b[0][q];
#pragma unroll
    for (int k = 1; k < BL_GROUPS; ++k) {                           // group order: the same sum in every thread and every launch
        const float4 ta = s_a[k][q], tb = s_b[k][q];
        sa.x += ta.x; sa.y += ta.y; sa.z += ta.z; sa.w += ta.w;
        sb.x += tb.x; sb.y += tb.y; sb.z += tb.z; sb.w += tb.w;
    }
    if (!live) return;
    const float ca = ba[0], cb = bb[0];
    float4 p;
    p.x = 1.f / (1.f + expf((sb.x + cb) - (sa.x + ca)));
    p.y = 1.f / (1.f + expf((sb.y + cb) - (sa.y + ca)));
    p.z = 1.f / (1.f + expf((sb.z + cb) - (sa.z + ca)));
    p.w = 1.f / (1.f + expf((sb.w + cb) - (sa.w + ca)));
    const float4 r = make_float4(1.f - p.x, 1.f - p.y, 1.f - p.z, 1.f - p.w);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        float4 o;
        o.x = va[i].x * p.x + vb[i].x * r.x;
        o.y = va[i].y * p.y + vb[i].y * r.y;
        o.z = va[i].z * p.z + vb[i].z * r.z;
        o.w = va[i].w * p.w + vb[i].w * r.w;
        *reinterpret_cast<float4*>(out + base + (size_t)i * HW) = o;
    }
    if (pa_out && g == 0) *reinterpret_cast<float4*>(pa_out + (size_t)n * HW + pix) = p;
}

}  // namespace heal

using namespace heal;

extern "C" int heal_ssfa_fused_enabled(void) {
    const char* v = getenv("HEAL_SSFA_FUSED");
    if (v == nullptr || v[0] == 0 || (v[0] == '1' && v[1] == 0)) return 1;
    return (v[0] == '0' && v[1] == 0) ? 0 : -1;
}

extern "C" int heal_deconv3x3_s2_supported(int cin, int cout, int H, int W) {
    if (cin < 32 || cin > 2048 || cin % (DC_KC * DC_SEG) != 0 || cout < DC_CO || cout > 2048 || cout % DC_CO != 0) return 0;
    if (H < 1 || W < 1) return 0;
    if ((long long)H * W >= (1ll << 29)) return 0;                                  // 4 H W and every in-plane offset stay an int
    const long long tiles = (long long)((H + DC_ROWS - 1) / DC_ROWS) * ((W + DC_COLS - 1) / DC_COLS);
    return tiles <= 65535 ? 1 : 0;
}

extern "C" int heal_deconv3x3_s2(const float* x, const float* wfrag, const float* bias, const float* residual, int res_channels,
                                 int n, int cin, int cout, int H, int W, int relu, float* y, void* stream) {
    HEAL_REQUIRE(heal_deconv3x3_s2_supported(cin, cout, H, W) && n >= 1 && n <= 65535,
                 "deconv3x3_s2: unsupported problem (n %d, cin %d, cout %d, %d x %d): cin and cout must be multiples of 32 in "
                 "32 .. 2048", n, cin, cout, H, W);
    HEAL_REQUIRE(x && wfrag && y, "deconv3x3_s2: null argument");
    HEAL_REQUIRE(res_channels >= 0 && res_channels <= cout && (residual != nullptr) == (res_channels > 0),
                 "deconv3x3_s2: residual of %d channels for %d output channels (a residual needs 1 .. cout channels, none needs 0)",
                 res_channels, cout);
    HEAL_REQUIRE((((uintptr_t)x | (uintptr_t)wfrag | (uintptr_t)residual | (uintptr_t)y) & 15) == 0,
                 "deconv3x3_s2: x, wfrag, residual and y must be 16-byte aligned");
    const int tiles = ((H + DC_ROWS - 1) / DC_ROWS) * ((W + DC_COLS - 1) / DC_COLS);
    const dim3 grid((unsigned)(cout / DC_CO), (unsigned)tiles, (unsigned)n);
    HEAL_LAUNCH_EV(k_deconv3x3_s2, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, x, reinterpret_cast<const float2*>(wfrag), bias,
                   residual, res_channels, cin, cout, H, W, relu ? 1 : 0, y);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" int heal_ssfa_blend_supported(int C, int HW) {
    return (C == 64 || C == 128) && HW >= 4 && HW % 4 == 0 && HW < (1 << 24) ? 1 : 0;
}

extern "C" int heal_ssfa_blend(const float* a, const float* b, const float* wa, const float* wb, const float* ba, const float* bb,
                               int n, int C, int HW, float* out, float* pa_out, void* stream) {
    HEAL_REQUIRE(heal_ssfa_blend_supported(C, HW) && n >= 1 && n <= 65535,
                 "ssfa_blend: unsupported problem (n %d, C %d, HW %d): C must be 64 or 128 and HW a multiple of 4", n, C, HW);
    HEAL_REQUIRE(a && b && wa && wb && ba && bb && out, "ssfa_blend: null argument");
    HEAL_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out | (uintptr_t)pa_out) & 15) == 0,
                 "ssfa_blend: a, b, out and pa_out must be 16-byte aligned");
    const dim3 grid((unsigned)((HW + BL_PIX - 1) / BL_PIX), (unsigned)n);
    if (C == 64)
        HEAL_LAUNCH_EV(k_ssfa_blend<4>, grid, dim3(BL_THREADS), 0, (hipStream_t)stream, a, b, wa, wb, ba, bb, HW, out, pa_out);
    else
        HEAL_LAUNCH_EV(k_ssfa_blend<8>, grid, dim3(BL_THREADS), 0, (hipStream_t)stream, a, b, wa, wb, ba, bb, HW, out, pa_out);
    HEAL_LAUNCH_CHECK();
    return 0;
}
