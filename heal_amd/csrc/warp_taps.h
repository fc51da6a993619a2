// The sampling arithmetic of warp_affine_simple (torch_transformation_utils.py:323-332), shared by every kernel that warps an
// agent's map into the ego frame (warp_fuse.hip, disco_fuse.hip, warp_mha.hip, warp_affine.hip).  It follows PyTorch operation for operation: base grid =
// linspace(-1,1,W)*(W-1)/W in the dtype of the affine matrix (float64 when pairwise_t_matrix comes from numpy), grid =
// base @ M^T, rounded to fp32, unnormalise ((g+1)*size-1)/2, floor, corner weights as products of fp32 differences, taps
// outside the image contribute zero.  This header also owns everything around that arithmetic: where the affine rows come from
// (AffineRows), the tap preamble (affine_taps, flat_taps, tap4), the plain agent softmax and the agent-count dispatch.
#pragma once
#include "common.h"
#include "../../include/heal_amd.h"

namespace heal {

constexpr int WF_MAXA = HEAL_WARP_MAX_AGENTS;     // agents handled per launch (max_cav is 5..8 in the reference configs)

// How a launch gets its poses: the rows of affine_matrix[b][0, a] (m00 m01 m02 m10 m11 m12) sit by value in the kernel arguments;
// a device copy wins when non-null (a captured HIP graph then follows the poses of the frame it is replayed on instead of the
// captured ones); f64 is the dtype the grid is evaluated in.  Embedded by value in every parameter block of the warp kernels.
struct AffineRows {
    const double* dev;      // [n][6] on the device, or null
    double m[WF_MAXA][6];
    int f64;
};

// Host: fills `r` for n agents (rows past n are zero).  `who` names the entry point in the message.
inline int fill_affine_rows(AffineRows& r, const char* who, const double* affine_host, const double* affine_dev, int n,
                            int grid_f64) {
    HEAL_REQUIRE(affine_host != nullptr || affine_dev != nullptr, "%s: affine is NULL (host and device)", who);
    r.dev = affine_dev; r.f64 = grid_f64;
    for (int a = 0; a < WF_MAXA; ++a)
        for (int k = 0; k < 6; ++k) r.m[a][k] = (a < n && affine_host) ? affine_host[a * 6 + k] : 0.0;
    return 0;
}

// One switch over the agent count for every kernel templated on it: `...` is the launch, written with NA for the count.
#define HEAL_AGENTS_CASE_(N, ...) case N: { constexpr int NA = N; __VA_ARGS__; } break;
#define HEAL_FOR_AGENTS(n, who, ...)                                                                                   \
    do {                                                                                                               \
        static_assert(heal::WF_MAXA == 8, "HEAL_FOR_AGENTS spells out cases 1..8: extend it with HEAL_WARP_MAX_AGENTS"); \
        switch (n) {                                                                                                   \
            HEAL_AGENTS_CASE_(1, __VA_ARGS__) HEAL_AGENTS_CASE_(2, __VA_ARGS__) HEAL_AGENTS_CASE_(3, __VA_ARGS__)      \
            HEAL_AGENTS_CASE_(4, __VA_ARGS__) HEAL_AGENTS_CASE_(5, __VA_ARGS__) HEAL_AGENTS_CASE_(6, __VA_ARGS__)      \
            HEAL_AGENTS_CASE_(7, __VA_ARGS__) HEAL_AGENTS_CASE_(8, __VA_ARGS__)                                        \
            default: return heal::set_error("%s: no kernel for %d agents", who, (int)(n));                             \
        }                                                                                                              \
    } while (0)

struct Taps {
    int off;       // y0*W + x0 (may point outside; guarded by `ok`)
    float w[4];    // nw, ne, sw, se
    unsigned ok;   // bit k set: tap k lies inside the image
};

template <typename T>
__device__ __forceinline__ T base_coord(int j, int n) {
    // torch.linspace(-1, 1, n) * (n - 1) / n, element j
    if (n <= 1) return (T)0;
    const T step = (T)2 / (T)(n - 1);
    const T v = (j < n / 2) ? (T)-1 + step * (T)j : (T)1 - step * (T)(n - 1 - j);
    return v * (T)(n - 1) / (T)n;
}

// the grid point of base coordinates (xs, ys): base @ M^T in T, rounded once to fp32
template <typename T>
__device__ __forceinline__ void grid_from_base(const double* m, T xs, T ys, float& gx, float& gy) {
    gx = (float)(((T)m[0] * xs + (T)m[1] * ys) + (T)m[2]);
    gy = (float)(((T)m[3] * xs + (T)m[4] * ys) + (T)m[5]);
}

template <typename T>
__device__ __forceinline__ void grid_point(const double* m, int h, int w, int H, int W, float& gx, float& gy) {
    grid_from_base<T>(m, base_coord<T>(w, W), base_coord<T>(h, H), gx, gy);
}

// x0c, y0c: the north-west tap's coordinates as t.off holds them (clamped into [-2, W] x [-2, H])
__device__ __forceinline__ Taps make_taps(float gx, float gy, int H, int W, int& x0c, int& y0c) {
    const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
    const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = x0 + 1.f, y1 = y0 + 1.f;
    Taps t;
    t.w[0] = (x1 - ix) * (y1 - iy);
    t.w[1] = (ix - x0) * (y1 - iy);
    t.w[2] = (x1 - ix) * (iy - y0);
    t.w[3] = (ix - x0) * (iy - y0);
    const bool xin0 = x0 >= 0.f && x0 <= (float)(W - 1);
    const bool xin1 = x1 >= 0.f && x1 <= (float)(W - 1);
    const bool yin0 = y0 >= 0.f && y0 <= (float)(H - 1);
    const bool yin1 = y1 >= 0.f && y1 <= (float)(H - 1);
    t.ok = (unsigned)(xin0 && yin0) | ((unsigned)(xin1 && yin0) << 1) | ((unsigned)(xin0 && yin1) << 2) |
           ((unsigned)(xin1 && yin1) << 3);
    // offsets are only dereferenced for taps with their bit set; keep the int conversion defined
    const float xc = fminf(fmaxf(x0, -2.f), (float)W), yc = fminf(fmaxf(y0, -2.f), (float)H);
    x0c = (int)xc; y0c = (int)yc;
    t.off = y0c * W + x0c;
    return t;
}

__device__ __forceinline__ Taps make_taps(float gx, float gy, int H, int W) {
    int x0c, y0c;
    return make_taps(gx, gy, H, W, x0c, y0c);
}

__device__ __forceinline__ void affine_row(const AffineRows& r, int a, double (&m)[6]) {
    // wave-uniform: six scalar loads from the kernel arguments or from the device buffer
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = r.dev ? r.dev[a * 6 + k] : r.m[a][k];
}

// the taps of ego pixel (h, w) of an H x W map on agent a's map
__device__ __forceinline__ Taps affine_taps(const AffineRows& r, int a, int h, int w, int H, int W) {
    float gx, gy;
    double m[6];
    affine_row(r, a, m);
    if (r.f64) grid_point<double>(m, h, w, H, W, gx, gy);
    else grid_point<float>(m, h, w, H, W, gx, gy);
    return make_taps(gx, gy, H, W);
}

// The four taps as (offset, weight) pairs for a branch-free channel loop: a tap outside the image gets weight 0 on offset
// `outside` (0: a valid address)
__device__ __forceinline__ void flat_taps(const Taps& t, int W, int (&off)[4], float (&wt)[4], int outside = 0) {
    const int o4[4] = {t.off, t.off + 1, t.off + W, t.off + W + 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = (t.ok >> k) & 1u;
        off[k] = ok ? o4[k] : outside;
        wt[k] = ok ? t.w[k] : 0.f;
    }
}

// affine_taps + flat_taps for a thread that may stand outside the ego map (`live` false: every weight 0, no early return)
__device__ __forceinline__ void pixel_taps(const AffineRows& r, int a, int h, int w, int H, int W, bool live, int (&off)[4],
                                           float (&wt)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { off[k] = 0; wt[k] = 0.f; }
    if (live) flat_taps(affine_taps(r, a, h, w, H, W), W, off, wt);
}

__device__ __forceinline__ float tap4(const float* __restrict__ src, const int (&off)[4], const float (&wt)[4]) {
    // sample() on flat taps: nw, ne, sw, se accumulated in that order
    float v = src[off[0]] * wt[0];
    v += src[off[1]] * wt[1];
    v += src[off[2]] * wt[2];
    v += src[off[3]] * wt[3];
    return v;
}

// plain softmax over the agents: max, exp, sum, divide -- torch's order
template <int NA>
__device__ __forceinline__ void softmax_agents(float (&p)[NA]) {
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < NA; ++a) mx = fmaxf(mx, p[a]);
    float den = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) { p[a] = expf(p[a] - mx); den += p[a]; }
#pragma unroll
    for (int a = 0; a < NA; ++a) p[a] = p[a] / den;
}

__device__ __forceinline__ float sample(const float* __restrict__ src, const Taps& t, int W) {
    // nw, ne, sw, se accumulated in that order (taps outside contribute exactly zero)
    float acc = 0.f;
    if (t.ok & 1u) acc = src[t.off] * t.w[0];
    if (t.ok & 2u) acc += src[t.off + 1] * t.w[1];
    if (t.ok & 4u) acc += src[t.off + W] * t.w[2];
    if (t.ok & 8u) acc += src[t.off + W + 1] * t.w[3];
    return acc;
}

}  // namespace heal
