// heal_conv_wgrad: weight gradient of the dense BEV convolutions (3x3 pad 1 and 1x1, stride 1 | 2) -- include/heal_amd_train.h.
//
//   dW[co][ci][ky][kx] = sum_{n, oy, ox} g[n][co][oy][ox] * x[n][ci][oy*s + ky - p][ox*s + kx - p]
//
// A GEMM with M = Cout, N = Cin per tap and K = the pixels, on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate).  Both operands are
// K-contiguous in NCHW (a channel's pixels are contiguous), so a k-step of the MFMA is 4 neighbouring output columns of one row.
//
// Block (256 threads, 4 waves): WG_TM = 64 output channels x WG_TN = 32 input channels x all k*k taps.  Wave w owns the 16 output
// channels w*16.. and both 16-wide input-channel tiles: 2 * k*k accumulator tiles (72 VGPRs for 3x3).  The block walks the pixel
// tiles of its split: R output rows x WG_TW = 32 output columns (R = 4 at stride 1, 2 at stride 2).  Per tile it stages
//   sG [64 co][R * 32 px]                         (+2 words per row: the two k-columns of a 32-lane read phase fall in disjoint banks)
//   sX [32 ci][(R-1)*s + k rows][31*s + k cols]   (the halo tile; row padded likewise)
// ONCE, with zeros where the tile leaves the image, the map's tail or the channel range, and every tap reads it shifted: the A
// operand (g) of a k-step is loaded once and feeds 2 * k*k MFMAs.  Nothing is predicated per MFMA.
//
// The pixel reduction is cut into `splits` contiguous runs of tiles (grid.z): 64 -> 64 channels would otherwise be a 1 x 2 grid.
// Each split writes its partial [split][Cout][Cin][k*k]; k_conv_wgrad_reduce adds them in split order (no atomics: bit-equal
// across launches).  With one split the kernel writes dW itself.
#include "common.h"
#include "../../include/heal_amd_train.h"

namespace heal {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WG_TM = 64;            // output channels per block (16 per wave)
constexpr int WG_TN = 32;            // input channels per block (two 16-wide MFMA tiles per wave)
constexpr int WG_TW = 32;            // output columns per pixel tile
constexpr int WG_TARGET_BLOCKS = 512;  // two blocks of ~62 KB LDS per CU x 256 CUs: what is resident at once
constexpr int WG_MIN_TILES = 2;      // pixel tiles per split, at least
constexpr int WG_MAX_SPLITS = 4096;

constexpr int wg_rows(int s) { return s == 1 ? 4 : 2; }
// smallest v >= n with v % 32 == r
constexpr int wg_pad(int n, int r) { return n + ((r - n % 32) + 32) % 32; }

template <int KS, int S>
struct WgCfg {
    static constexpr int R = wg_rows(S);
    static constexpr int PX = R * WG_TW;                 // output pixels per tile = 4 * (k-steps per tile)
    static constexpr int RI = (R - 1) * S + KS;          // input rows of the halo tile
    static constexpr int CI = (WG_TW - 1) * S + KS;      // input columns of the halo tile
    static constexpr int GS = wg_pad(PX, 2);             // words per output channel in sG
    static constexpr int XS = wg_pad(RI * CI, S == 1 ? 2 : 4);   // words per input channel in sX
    static constexpr int LDS_BYTES = (WG_TM * GS + WG_TN * XS) * 4;
};

template <int KS, int S>
__global__ __launch_bounds__(256) void k_conv_wgrad(const float* __restrict__ x, const float* __restrict__ g, int cin, int cout,
                                                   int H, int W, int Ho, int Wo, int tiles_y, int tiles_x, int tiles, int splits,
                                                   float* __restrict__ dst /* [splits][cout][cin][KS*KS] */) {
    using C = WgCfg<KS, S>;
    constexpr int KK = KS * KS, P = KS / 2;
    static_assert(C::LDS_BYTES <= 65536, "tile does not fit the static LDS limit");
    __shared__ float sG[WG_TM * C::GS];
    __shared__ float sX[WG_TN * C::XS];
    const int co0 = blockIdx.x * WG_TM, ci0 = blockIdx.y * WG_TN, split = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lk = lane >> 4, ln = lane & 15;
    // this split's run of tiles: the first tiles % splits runs hold one tile more (none is empty: splits <= tiles)
    const int base = tiles / splits, rem = tiles % splits;
    const int t_begin = split * base + (split < rem ? split : rem);
    const int t_end = t_begin + base + (split < rem ? 1 : 0);
    const bool wave_on = co0 + wave * 16 < cout;
    const bool tile_on[2] = {ci0 < cin, ci0 + 16 < cin};

    f32x4 acc[2][KK];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < KK; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int img = tile / (tiles_y * tiles_x), rest = tile - img * (tiles_y * tiles_x);
        const int oy0 = (rest / tiles_x) * C::R, ox0 = (rest % tiles_x) * WG_TW;
        const int iy0 = oy0 * S - P, ix0 = ox0 * S - P;
        // ---- stage g: [co][r][c], zero outside the channel range and the map
        const float* gi = g + (size_t)img * cout * Ho * Wo;
        for (int e = tid; e < WG_TM * C::PX; e += 256) {
            const int co = e / C::PX, px = e % C::PX;
            const int oy = oy0 + px / WG_TW, ox = ox0 + px % WG_TW;
            float v = 0.f;
            if (co0 + co < cout && oy < Ho && ox < Wo) v = gi[((size_t)(co0 + co) * Ho + oy) * Wo + ox];
            sG[co * C::GS + px] = v;
        }
        // ---- stage x: [ci][row][col] of the halo tile, zero outside the channel range and the image (the padding)
        const float* xi = x + (size_t)img * cin * H * W;
        for (int e = tid; e < WG_TN * C::RI * C::CI; e += 256) {
            const int ci = e / (C::RI * C::CI), q = e % (C::RI * C::CI);
            const int ri = q / C::CI, cc = q % C::CI;
            const int iy = iy0 + ri, ix = ix0 + cc;
            float v = 0.f;
            if (ci0 + ci < cin && iy >= 0 && iy < H && ix >= 0 && ix < W) v = xi[((size_t)(ci0 + ci) * H + iy) * W + ix];
            sX[ci * C::XS + ri * C::CI + cc] = v;
        }
        __syncthreads();
        if (wave_on) {
            const float* ga = sG + (wave * 16 + ln) * C::GS + lk;          // A: g[co = ln][pixel = lk]
            const float* xb = sX + ln * C::XS + lk * S;                    // B: x[pixel = lk][ci = ln]
            for (int r = 0; r < C::R; ++r) {
#pragma unroll
                for (int c4 = 0; c4 < WG_TW / 4; ++c4) {
                    const float a = ga[r * WG_TW + c4 * 4];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        if (!tile_on[t]) continue;
#pragma unroll
                        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                            for (int kx = 0; kx < KS; ++kx) {
                                const float b = xb[t * 16 * C::XS + (r * S + ky) * C::CI + c4 * 4 * S + kx];
                                acc[t][ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t][ky * KS + kx], 0, 0, 0);
                            }
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- D[row = lk*4 + r (co)][col = ln (ci)] of every tap
    if (!wave_on) return;
    float* out = dst + (size_t)split * cout * cin * KK;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ci = ci0 + t * 16 + ln;
        if (ci >= cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + wave * 16 + lk * 4 + r;
            if (co >= cout) continue;
#pragma unroll
            for (int q = 0; q < KK; ++q) out[((size_t)co * cin + ci) * KK + q] = acc[t][q][r];
        }
    }
}

// dW[e] = partial[0][e] + partial[1][e] + ... in split order
__global__ __launch_bounds__(256) void k_conv_wgrad_reduce(const float* __restrict__ part, int splits, int count,
                                                          float* __restrict__ dw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float s = part[e];
    for (int k = 1; k < splits; ++k) s += part[(size_t)k * count + e];
    dw[e] = s;
}

struct WgShape { int Ho, Wo, tiles_y, tiles_x, tiles, splits; };

// false: a shape the kernel does not take (bad k / stride / sizes, or an index range that does not fit)
static bool wg_shape(int n, int cin, int cout, int H, int W, int k, int stride, WgShape* s) {
    if ((k != 1 && k != 3) || (stride != 1 && stride != 2) || n < 1 || cin < 1 || cout < 1 || H < 1 || W < 1) return false;
    s->Ho = (H - 1) / stride + 1;
    s->Wo = (W - 1) / stride + 1;
    s->tiles_y = ceil_div(s->Ho, wg_rows(stride));
    s->tiles_x = ceil_div(s->Wo, WG_TW);
    const int64_t tiles = (int64_t)n * s->tiles_y * s->tiles_x;
    const int64_t count = (int64_t)cout * cin * k * k;
    if (tiles > 0x3fffffff || count > 0x3fffffff || ceil_div(cin, WG_TN) > 65535) return false;
    s->tiles = (int)tiles;
    const int mn = ceil_div(cout, WG_TM) * ceil_div(cin, WG_TN);
    int splits = WG_TARGET_BLOCKS / mn;          // rounded down: one resident round of blocks, no tail round of a few
    const int most = ceil_div(s->tiles, WG_MIN_TILES);
    if (splits > most) splits = most;
    if (splits > WG_MAX_SPLITS) splits = WG_MAX_SPLITS;
    s->splits = splits < 1 ? 1 : splits;
    return true;
}

}  // namespace heal

using namespace heal;

extern "C" int heal_conv_wgrad_supported(int n, int cin, int cout, int H, int W, int k, int stride) {
    WgShape s;
    return wg_shape(n, cin, cout, H, W, k, stride, &s) ? 1 : 0;
}

extern "C" int heal_conv_wgrad_splits(int n, int cin, int cout, int H, int W, int k, int stride) {
    WgShape s;
    return wg_shape(n, cin, cout, H, W, k, stride, &s) ? s.splits : 0;
}

extern "C" size_t heal_conv_wgrad_workspace(int n, int cin, int cout, int H, int W, int k, int stride) {
    WgShape s;
    if (!wg_shape(n, cin, cout, H, W, k, stride, &s) || s.splits < 2) return 0;
    return (size_t)s.splits * cout * cin * k * k * sizeof(float);
}

extern "C" int heal_conv_wgrad(const float* x, const float* g, int n, int cin, int cout, int H, int W, int k, int stride, float* dw,
                               void* ws, size_t ws_bytes, void* stream) {
    WgShape s;
    HEAL_REQUIRE(wg_shape(n, cin, cout, H, W, k, stride, &s),
                 "conv_wgrad: unsupported shape n=%d Cin=%d Cout=%d HxW=%dx%d k=%d stride=%d (k 1 | 3, stride 1 | 2, sizes >= 1)", n,
                 cin, cout, H, W, k, stride);
    HEAL_REQUIRE(x && g && dw, "conv_wgrad: null pointer");
    const size_t need = heal_conv_wgrad_workspace(n, cin, cout, H, W, k, stride);
    HEAL_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv_wgrad: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                 need);
    HEAL_REQUIRE(need == 0 || ((uintptr_t)ws & 3) == 0, "conv_wgrad: workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* dst = s.splits > 1 ? (float*)ws : dw;
    const dim3 grid(ceil_div(cout, WG_TM), ceil_div(cin, WG_TN), s.splits);
#define HEAL_WG_LAUNCH(KS, S)                                                                                                   \
    hipLaunchKernelGGL((k_conv_wgrad<KS, S>), grid, dim3(256), 0, st, x, g, cin, cout, H, W, s.Ho, s.Wo, s.tiles_y, s.tiles_x, \
                       s.tiles, s.splits, dst)
    if (k == 3 && stride == 1) HEAL_WG_LAUNCH(3, 1);
    else if (k == 3) HEAL_WG_LAUNCH(3, 2);
    else if (stride == 1) HEAL_WG_LAUNCH(1, 1);
    else HEAL_WG_LAUNCH(1, 2);
#undef HEAL_WG_LAUNCH
    HEAL_LAUNCH_CHECK();
    if (s.splits > 1) {
        const int count = cout * cin * k * k;
        hipLaunchKernelGGL(k_conv_wgrad_reduce, dim3(ceil_div(count, 256)), dim3(256), 0, st, (const float*)ws, s.splits, count, dw);
        HEAL_LAUNCH_CHECK();
    }
    return 0;
}
