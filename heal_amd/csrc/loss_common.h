// What the streaming criterion kernels share (det_loss.hip, unc_loss.hip, kd_loss.hip): the tile geometry, the focal term, the
// three per-anchor blocks of the anchor heads (cls, one smooth-L1 component, dir) that k_dl_det and k_ul_unc both call, the integer
// count of the positives per sample, the one-block fp64 finish (kd_loss.hip launches it too) and the host side of the two
// anchor-head entry points: parameters, argument checks and the count -> pass -> finish launches.
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

// ---------------------------------------------------------------------------------------------------------- anchor blocks
// The per-anchor blocks of k_dl_det and k_ul_unc: one copy, so that on the same inputs both kernels' cls, reg and dir partials and
// gradients are bit-equal.  wr = 1 / normaliser; the accumulators are the caller's lane sums, added to in anchor order.

// cls: the focal term of anchor score `at`, exactly 0 where pos = neg = 0, and its gradient
__device__ __forceinline__ void dl_cls_block(const float* __restrict__ cls, float* __restrict__ gcls, size_t at, bool live, float pv,
                                             float nv, bool is_pos, float nrm, const DetParams& prm, float& s_cls) {
    const float x = live ? cls[at] : 0.f;
    const float w = ((is_pos ? prm.pos_cls_weight : 0.f) + (nv > 0.f ? 1.0f : 0.f)) / nrm;
    float l, dx;
    dl_focal(x, pv, w, prm.alpha, l, dx);
    if (w == 0.f) { l = 0.f; dx = 0.f; }          // pos = neg = 0: exactly nothing, whatever the logit
    s_cls += l;
    if (gcls != nullptr && live) gcls[at] = dx * prm.scale[0];
}

// reg: one smooth-L1 component of a positive anchor, x against its target t; the yaw (component 6) as sin(a) cos(b) against
// cos(a) sin(b) with its chain factor.  -> the term; g <- d term / d x, scaled
__device__ __forceinline__ float dl_smooth_l1(bool yaw, float x, float t, float wr, const DetParams& prm, float& g) {
    float d, chain = 1.0f;
    if (yaw) {
        const float sa = sinf(x), ca = cosf(x), sb = sinf(t), cb = cosf(t);
        d = sa * cb - ca * sb;
        chain = ca * cb + sa * sb;
    } else {
        d = x - t;
    }
    const float ad = fabsf(d);
    const bool small = ad <= prm.inv_sigma2;
    const float l = small ? 0.5f * (ad * ad) * prm.sigma2 : ad - 0.5f * prm.inv_sigma2;
    const float dl = small ? d * prm.sigma2 : (d > 0.f ? 1.0f : -1.0f);
    g = dl * chain * wr * prm.scale[1];
    return l * wr;
}

// dir: two-bin cross-entropy = softplus(other - chosen) of the logits at at0 and at0 + HW; the bin in double from the label as
// stored (tyaw) and the anchor's yaw
__device__ __forceinline__ void dl_dir_block(const float* __restrict__ dir, float* __restrict__ gdir, size_t at0, int HW, bool live,
                                             bool is_pos, double tyaw, double anchor_yaw, float wr, const DetParams& prm,
                                             float& s_dir) {
    float g0 = 0.f, g1 = 0.f;
    if (is_pos) {
        const double two_pi = 6.283185307179586476925286766559, pi = 3.141592653589793238462643383279;
        const double v = (tyaw + anchor_yaw) - prm.dir_offset;
        const double off = v - floor(v / two_pi) * two_pi;
        const int bin = min(max((int)floor(off / pi), 0), 1);
        const float l0 = dir[at0], l1 = dir[at0 + HW];
        const float z = bin == 0 ? l1 - l0 : l0 - l1;          // other - chosen
        float p, q, e;
        dl_sigmoid(z, p, q, e);
        s_dir += (fmaxf(z, 0.f) + log1pf(e)) * wr;
        const float go = p * wr * prm.scale[2];                // d / d other; chosen gets the negative
        g0 = bin == 0 ? -go : go;
        g1 = bin == 0 ? go : -go;
    }
    if (gdir != nullptr && live) {
        gdir[at0] = g0;
        gdir[at0 + HW] = g1;
    }
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

// ---------------------------------------------------------------------------------------------------------- anchor heads, host
// What heal_det_loss and heal_unc_loss are launched with.  A pass type derives from it and adds its own parameters and
// `template <typename T, int A> void launch() const`, the launch of its kernel for label type T and A anchors.
struct HeadLaunch {
    const float *cls, *reg, *dir;
    const void *pos, *neg, *tgt;
    float *gcls, *greg, *gdir;
    hipStream_t s;
    int* counts;
    float* partials;
    int HW, tiles, total;
    dim3 grid;
};

static bool dl_head_shape_ok(int n, int anchors, int H, int W) {
    long long tiles;
    return anchors >= 1 && anchors <= DL_MAX_A && dl_map_ok(n, 7 * anchors, H, W, &tiles);
}

// the counts of n samples + `terms` partials per tile; 0 for a shape out of range
static size_t dl_head_workspace(int n, int anchors, int H, int W, int terms) {
    if (!dl_head_shape_ok(n, anchors, H, W)) return 0;
    return align_up((size_t)n * DL_CB * sizeof(int)) + align_up((size_t)terms * dl_tiles(n, (long long)H * W) * sizeof(float));
}

// the checks both entry points make after their shape's (maps: the names of the head maps in the message; set: they, the labels
// and terms are), then the workspace's layout
static int dl_head_setup(const char* who, const char* maps, bool set, const double* anchor_yaw, float sigma, void* ws,
                         size_t ws_bytes, int n, int anchors, int H, int W, int terms, HeadLaunch& h) {
    HEAL_REQUIRE(set, "%s: %s, the three labels and terms must be set", who, maps);
    HEAL_REQUIRE(h.dir == nullptr || anchor_yaw != nullptr, "%s: dir_preds needs anchor_yaw[anchors]", who);
    HEAL_REQUIRE(h.dir != nullptr || h.gdir == nullptr, "%s: grad_dir without dir_preds", who);
    HEAL_REQUIRE(sigma > 0.f, "%s: sigma must be positive, got %g", who, (double)sigma);
    const size_t need = dl_head_workspace(n, anchors, H, W, terms);
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu (heal_%s_workspace)", who, ws_bytes, need,
                 who);
    h.HW = H * W;
    h.tiles = ceil_div(h.HW, DL_TILE);
    h.total = (int)dl_tiles(n, h.HW);
    h.grid = dim3((unsigned)ceil_div(h.total, DL_WAVES));
    Arena arena(ws, ws_bytes);
    h.counts = arena.take<int>((size_t)n * DL_CB);
    h.partials = arena.take<float>((size_t)terms * h.total);
    return 0;
}

static void dl_det_params(DetParams& prm, float pos_cls_weight, float alpha, float sigma, float cls_weight, float reg_weight,
                          float dir_weight, int n, const double* anchor_yaw, int anchors, double dir_offset) {
    prm.pos_cls_weight = pos_cls_weight;
    prm.alpha = alpha;
    prm.sigma2 = sigma * sigma;
    prm.inv_sigma2 = 1.0f / (sigma * sigma);
    prm.scale[0] = (float)((double)cls_weight / n);
    prm.scale[1] = (float)((double)reg_weight / n);
    prm.scale[2] = (float)((double)dir_weight / n);
    for (int a = 0; a < DL_MAX_A; ++a) prm.yaw[a] = (anchor_yaw != nullptr && a < anchors) ? anchor_yaw[a] : 0.0;
    prm.dir_offset = dir_offset;
}

template <typename T, typename L>
static int dl_head_passes(const L& l, int n, int anchors, hipEvent_t start) {
    HEAL_LAUNCH_EV2(k_dl_count<T>, dim3(DL_CB, n), dim3(256), 0, l.s, start, nullptr, (const T*)l.pos, (long long)l.HW * anchors,
                    l.counts);
    HEAL_LAUNCH_CHECK();
    switch (anchors) {
        case 1: l.template launch<T, 1>(); break;
        case 2: l.template launch<T, 2>(); break;
        case 3: l.template launch<T, 3>(); break;
        default: l.template launch<T, 4>(); break;
    }
    HEAL_LAUNCH_CHECK();
    return 0;
}

// count -> L's pass -> finish: terms[t] <- sc.s[t] x the sum of term t's partials
template <typename L>
static int dl_head_run(const L& l, int labels_f64, int n, int anchors, int terms, const FinishScales& sc, float* out) {
    const LaunchEvents ev = take_launch_events();
    const int rc = labels_f64 ? dl_head_passes<double>(l, n, anchors, ev.start) : dl_head_passes<float>(l, n, anchors, ev.start);
    if (rc != 0) return rc;
    HEAL_LAUNCH_EV2(k_dl_finish, dim3(1), dim3(256), 0, l.s, nullptr, ev.stop, (const float*)l.partials, l.total, terms, sc, out);
    HEAL_LAUNCH_CHECK();
    return 0;
}

}  // namespace heal
