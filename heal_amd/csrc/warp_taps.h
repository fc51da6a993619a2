// The sampling arithmetic of warp_affine_simple (torch_transformation_utils.py:323-332), shared by every kernel that warps an
// agent's map into the ego frame (warp_fuse.hip, disco_fuse.hip, warp_mha.hip, warp_affine.hip).  It follows PyTorch operation for operation: base grid =
// linspace(-1,1,W)*(W-1)/W in the dtype of the affine matrix (float64 when pairwise_t_matrix comes from numpy), grid =
// base @ M^T, rounded to fp32, unnormalise ((g+1)*size-1)/2, floor, corner weights as products of fp32 differences, taps
// outside the image contribute zero.
#pragma once
#include "common.h"
#include "../../include/heal_amd.h"

namespace heal {

constexpr int WF_MAXA = HEAL_WARP_MAX_AGENTS;     // agents handled per launch (max_cav is 5..8 in the reference configs)

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

__device__ __forceinline__ Taps make_taps(float gx, float gy, int H, int W) {
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
    t.off = (int)yc * W + (int)xc;
    return t;
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
