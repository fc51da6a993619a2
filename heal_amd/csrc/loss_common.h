// What the streaming criterion kernels share (det_loss.hip, unc_loss.hip): the tile geometry, the focal term, the integer count of
// the positives per sample and the one-block fp64 finish.  Moved here from det_loss.hip as they were: no arithmetic differs.
#pragma once
#include "common.h"
#include "../../include/heal_amd.h"

namespace heal {

constexpr int DL_TILE = 64;       // pixels per wave
constexpr int DL_WAVES = 4;       // tiles per block
constexpr int DL_MAX_A = HEAL_LOSS_MAX_ANCHORS;
constexpr int DL_CB = 64;         // count blocks per sample (and level): the main kernels add their 64 words, one per lane

struct DetParams {
    float pos_cls_weight, alpha, sigma2, inv_sigma2;
    float scale[3];               // weight / N of cls, reg, dir
    double yaw[DL_MAX_A];         // anchor yaw, radians
    double dir_offset;
};

// e = exp(-|x|) -> p = sigmoid(x) and q = 1 - p without cancellation
__device__ __forceinline__ void dl_sigmoid(float x, float& p, float& q, float& e) {
    e = expf(-fabsf(x));
    const float r = 1.0f / (1.0f + e);
    const float s = e * r;
    p = x >= 0.f ? r : s;
    q = x >= 0.f ? s : r;
}

// sigmoid focal loss with gamma = 2 (point_pillar_loss.py:230-244) and its derivative in x; w = 0 gives exactly (0, 0)
//   ce = max(x, 0) - x t + log1p(exp(-|x|)),  1 - p_t = t (1 - p) + (1 - t) p,  loss = (1 - p_t)^2 (t a + (1 - t)(1 - a)) ce w
__device__ __forceinline__ void dl_focal(float x, float t, float w, float alpha, float& loss, float& dx) {
    float p, q, e;
    dl_sigmoid(x, p, q, e);
    const float ce = fmaxf(x, 0.f) - x * t + log1pf(e);
    const float m = t * q + (1.0f - t) * p;
    const float at = t * alpha + (1.0f - t) * (1.0f - alpha);
    const float dm = (1.0f - 2.0f * t) * (p * q);          // d (1 - p_t) / dx
    loss = (m * m) * at * ce * w;
    dx = at * w * (2.0f * m * dm * ce + (m * m) * (p - t));
}

// ---------------------------------------------------------------------------------------------------------- counts
// counts[n * DL_CB + b] <- number of anchors with pos > 0 in the b-th of DL_CB equal chunks of sample n: grid (DL_CB, N).  Every
// block writes its word (possibly 0); the readers add the DL_CB words of a sample -- integers, exact in any order
template <typename T>
__global__ __launch_bounds__(256) void k_dl_count(const T* __restrict__ pos, long long per_sample, int* __restrict__ counts) {
    __shared__ int sc[4];
    const T* __restrict__ p = pos + (size_t)blockIdx.y * per_sample;
    const long long chunk = (per_sample + DL_CB - 1) / DL_CB;
    const long long i0 = (long long)blockIdx.x * chunk, i1 = min(i0 + chunk, per_sample);
    int c = 0;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) c += p[i] > (T)0 ? 1 : 0;
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.y * DL_CB + blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

// the sum of one sample's DL_CB count words, clamped at 1; every lane of the wave must call it
__device__ __forceinline__ float dl_normaliser(const int* __restrict__ counts, int slot, int lane) {
    return (float)max(wave_sum_i(counts[slot * DL_CB + lane]), 1);
}

// ---------------------------------------------------------------------------------------------------------- finish
struct FinishScales { double s[4]; };

// out[t] <- scale[t] * sum_i partials[t * n_partials + i], t < terms: thread j adds partials j, j + 256, ... in fp64, then a fixed
// LDS tree.  (static: one copy per translation unit that launches it)
static __global__ __launch_bounds__(256) void k_dl_finish(const float* __restrict__ partials, int n_partials, int terms,
                                                          FinishScales sc, float* __restrict__ out) {
    __shared__ double acc[256];
    for (int t = 0; t < terms; ++t) {
        double v = 0.0;
        for (int i = threadIdx.x; i < n_partials; i += 256) v += (double)partials[(size_t)t * n_partials + i];
        acc[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[t] = (float)(acc[0] * sc.s[t]);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------- host
static long long dl_tiles(long long n, long long hw) { return n * ((hw + DL_TILE - 1) / DL_TILE); }

static bool dl_map_ok(int n, int channels, int H, int W, long long* tiles) {
    if (n < 1 || channels < 1 || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL - DL_TILE || hw * channels > 0x7fffffffLL) return false;
    const long long t = dl_tiles(n, hw);
    if (t > 0x7fffffffLL - DL_WAVES) return false;
    *tiles = t;
    return true;
}

}  // namespace heal
