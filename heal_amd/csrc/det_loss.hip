// DL -- the three criterion terms of the training step, each with its gradient, in one streaming pass over the NCHW maps.
//
// Reference arithmetic:
//   heal_det_loss          opencood/loss/point_pillar_loss.py:36-122   sigmoid focal loss on the anchor scores, smooth-L1 with the
//                          sin-difference yaw encoding on the box deltas, two-bin cross-entropy on the direction logits
//   heal_occ_loss          opencood/loss/point_pillar_pyramid_loss.py:71-107   the focal term on every pyramid level's occupancy map
//                          against the anchor labels pooled to the level (max of the positives, min of the negatives)
//   heal_depth_focal_loss  opencood/loss/point_pillar_depth_loss.py:97-181   multi-class focal loss over the depth bins
//
// The torch compositions make permuted copies of every head map, one-hot scatters, max_pool2d pairs per level, float64 arithmetic
// wherever a float64 label meets a float32 map, and the mirror image of all of it in backward.  Here, as in kd_loss.hip, lanes run
// along the pixels of the NCHW maps: a WAVE owns 64 consecutive pixels of one image (a tile), every channel row of the tile is one
// 256-B access, nothing is permuted or copied, and the labels ([N, H, W, A] and [N, H, W, 7A], float32 or float64) are read where
// they lie.  A block is four waves = four consecutive tiles; the waves never talk to each other, so there is no LDS and no barrier
// in the main kernels.
//
// Phases are separate launches (no hand-shake between blocks): (1) integer counts of the positives per sample, 64 blocks per
// sample -- every block writes its own word, nothing accumulates into uninitialised memory, and the readers add the 64 words
// (integers: exact in any order); (2) the pass over the maps, which writes the gradients and one
// partial sum per tile and term; (3) k_dl_finish, one block, adds the partials in a fixed order in fp64.
//
// Reduction: no floating-point atomics.  Lane sums over anchors / channels in index order -> xor tree over the 64 lanes ->
// partial[term][tile] -> fixed-order fp64 sum.  No path depends on an address: two launches on the same values are bit-equal
// wherever the data lies.  fp32 arithmetic (the library is built with -ffp-contract=off); the direction bin is computed in double
// from the label as stored, as the reference does whatever the label type (its anchor_yaw_map is a float64 tensor).
//
// loss_common.h holds what this file shares with unc_loss.hip and kd_loss.hip: the per-anchor cls / smooth-L1 / dir blocks
// k_dl_det calls, k_dl_count, k_dl_finish and the host side of the anchor-head entry points (dl_head_*).
#include "loss_common.h"

namespace heal {

constexpr int DL_MAX_LEVELS = HEAL_OCC_LOSS_MAX_LEVELS;

struct OccLevels {
    const float* occ[DL_MAX_LEVELS];
    float* grad[DL_MAX_LEVELS];
    int k[DL_MAX_LEVELS], Hl[DL_MAX_LEVELS], Wl[DL_MAX_LEVELS];
    int tiles[DL_MAX_LEVELS];     // per image
    int tile0[DL_MAX_LEVELS + 1]; // first global tile of the level; [levels] = total
    float scale[DL_MAX_LEVELS];   // pyramid weight / N
    int levels;
};

// foreground / background of one pooled cell: any anchor of any pixel of the k x k window positive; every one negative
template <typename T>
__device__ __forceinline__ void dl_pool(const T* __restrict__ pos, const T* __restrict__ neg, int A, int W, int k, int y, int x,
                                        bool& fg, bool& bg) {
    fg = false;
    bg = true;
    for (int dy = 0; dy < k; ++dy) {
        const size_t row = ((size_t)(y * k + dy) * W + (size_t)x * k) * A;
        for (int j = 0; j < k * A; ++j) {
            fg = fg || pos[row + j] != (T)0;
            bg = bg && neg[row + j] != (T)0;
        }
    }
}

// counts[(l * N + n) * DL_CB + b] <- pooled foreground cells in the b-th chunk of sample n at level l: grid (DL_CB, N, levels)
template <typename T>
__global__ __launch_bounds__(256) void k_dl_occ_count(const T* __restrict__ pos, const T* __restrict__ neg, int A, int H, int W,
                                                      OccLevels lv, int* __restrict__ counts) {
    __shared__ int sc[4];
    const int n = blockIdx.y, l = blockIdx.z;
    const int k = lv.k[l], Wl = lv.Wl[l], cells = lv.Hl[l] * Wl;
    const int chunk = (cells + DL_CB - 1) / DL_CB;
    const int i0 = min((int)blockIdx.x * chunk, cells), i1 = min(i0 + chunk, cells);
    const T* __restrict__ p = pos + (size_t)n * H * W * A;
    const T* __restrict__ q = neg + (size_t)n * H * W * A;
    int c = 0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        bool fg, bg;
        dl_pool(p, q, A, W, k, i / Wl, i % Wl, fg, bg);
        c += fg ? 1 : 0;
    }
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[(l * gridDim.y + n) * DL_CB + blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

// ---------------------------------------------------------------------------------------------------------- detection
template <typename T, int A>
__global__ __launch_bounds__(256) void k_dl_det(const float* __restrict__ cls, const float* __restrict__ reg,
                                                const float* __restrict__ dir, const T* __restrict__ pos,
                                                const T* __restrict__ neg, const T* __restrict__ tgt,
                                                const int* __restrict__ counts, int HW, int tiles, int total_tiles,
                                                DetParams prm, float* __restrict__ gcls, float* __restrict__ greg,
                                                float* __restrict__ gdir, float* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * DL_WAVES + wave;
    if (tile >= total_tiles) return;                      // wave-uniform; the waves of a block share nothing
    const int n = tile / tiles, pix = (tile % tiles) * DL_TILE + lane;
    const bool live = pix < HW;                           // the tail of an image is masked, never read or written
    const float nrm = dl_normaliser(counts, n, lane);
    const size_t lab0 = ((size_t)n * HW + (size_t)pix) * A;
    float s_cls = 0.f, s_reg = 0.f, s_dir = 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float pv = live ? (float)pos[lab0 + a] : 0.f;
        const float nv = live ? (float)neg[lab0 + a] : 0.f;
        const bool is_pos = pv > 0.f;
        dl_cls_block(cls, gcls, ((size_t)n * A + a) * HW + (size_t)pix, live, pv, nv, is_pos, nrm, prm, s_cls);
        const float wr = 1.0f / nrm;
        const size_t t0 = (lab0 + a) * 7;
        // reg: seven smooth-L1 terms, each gradient stored at once
        float tyaw_f = 0.f;
        double tyaw = 0.0;
        if (is_pos) {
            tyaw = (double)tgt[t0 + 6];
            tyaw_f = (float)tyaw;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const size_t at = ((size_t)n * 7 * A + (size_t)a * 7 + k) * HW + (size_t)pix;
            float g = 0.f;
            if (is_pos) s_reg += dl_smooth_l1(k == 6, reg[at], k == 6 ? tyaw_f : (float)tgt[t0 + k], wr, prm, g);
            if (greg != nullptr && live) greg[at] = g;
        }
        if (dir != nullptr)
            dl_dir_block(dir, gdir, ((size_t)n * 2 * A + (size_t)a * 2) * HW + (size_t)pix, HW, live, is_pos, tyaw, prm.yaw[a], wr, prm,
                         s_dir);
    }
    s_cls = wave_sum(s_cls);
    s_reg = wave_sum(s_reg);
    s_dir = wave_sum(s_dir);
    if (lane == 0) {
        partials[tile] = s_cls;
        partials[(size_t)total_tiles + tile] = s_reg;
        partials[(size_t)2 * total_tiles + tile] = s_dir;
    }
}

struct DetLaunch : HeadLaunch {
    DetParams prm;
    template <typename T, int A>
    void launch() const {
        hipLaunchKernelGGL((k_dl_det<T, A>), grid, dim3(256), 0, s, cls, reg, dir, (const T*)pos, (const T*)neg, (const T*)tgt,
                           (const int*)counts, HW, tiles, total, prm, gcls, greg, gdir, partials);
    }
};

// ---------------------------------------------------------------------------------------------------------- occupancy
template <typename T>
__global__ __launch_bounds__(256) void k_dl_occ(const T* __restrict__ pos, const T* __restrict__ neg, const int* __restrict__ counts,
                                                int N, int A, int H, int W, OccLevels lv, float pos_cls_weight, float alpha,
                                                float* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * DL_WAVES + wave;
    if (tile >= lv.tile0[lv.levels]) return;
    int l = 0;
    while (l + 1 < lv.levels && tile >= lv.tile0[l + 1]) ++l;
    const int local = tile - lv.tile0[l];
    const int n = local / lv.tiles[l], c = (local % lv.tiles[l]) * DL_TILE + lane;
    const int Wl = lv.Wl[l], cells = lv.Hl[l] * Wl;
    float loss = 0.f;
    const float nrm = dl_normaliser(counts, l * N + n, lane);
    if (c < cells) {
        bool fg, bg;
        dl_pool(pos + (size_t)n * H * W * A, neg + (size_t)n * H * W * A, A, W, lv.k[l], c / Wl, c % Wl, fg, bg);
        const float t = fg ? 1.0f : 0.f;
        const float w = ((fg ? pos_cls_weight : 0.f) + (bg ? 1.0f : 0.f)) / nrm;
        const size_t at = (size_t)n * cells + c;
        float dx;
        dl_focal(lv.occ[l][at], t, w, alpha, loss, dx);
        if (w == 0.f) { loss = 0.f; dx = 0.f; }
        if (lv.grad[l] != nullptr) lv.grad[l][at] = dx * lv.scale[l];
    }
    loss = wave_sum(loss) * lv.scale[l];
    if (lane == 0) partials[tile] = loss;
}

// ---------------------------------------------------------------------------------------------------------- depth
// per pixel: M = max_k x, d = x - M, e = exp(d), Z = sum e, log p_g = d_g - log Z, 1 - p_g = (sum_{k != g} e) / Z
//   loss = -alpha (1 - p_g)^2 log p_g,   d loss / d x_k = -alpha F (delta_gk - p_k),   F = (1 - p_g)^2 - 2 (1 - p_g) p_g log p_g
__device__ __forceinline__ float dl_depth_weight(const float* __restrict__ mask, size_t at, float scale) {
    if (mask == nullptr) return scale;
    const float f = mask[at];
    return (f > 0.f ? 3.25f : (f == 0.f ? 0.25f : 0.f)) * scale;   // (fg > 0) * 3.25 + (fg == 0) * 0.25, as the loss module
}

template <int DCAP>
__global__ __launch_bounds__(256) void k_dl_depth_regs(const float* __restrict__ logit, const long long* __restrict__ index,
                                                       const float* __restrict__ mask, int D, int HW, int tiles, int total_tiles,
                                                       float alpha, float scale, float* __restrict__ grad,
                                                       float* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * DL_WAVES + wave;
    if (tile >= total_tiles) return;
    const int n = tile / tiles, pix = (tile % tiles) * DL_TILE + lane;
    const bool live = pix < HW;
    const size_t base = (size_t)n * D * HW + (size_t)pix;
    float x[DCAP];
#pragma unroll
    for (int i = 0; i < DCAP; ++i) x[i] = (live && i < D) ? logit[base + (size_t)i * HW] : -INFINITY;
    float loss = 0.f;
    const long long g = live ? index[(size_t)n * HW + pix] : -1;
    const bool valid = g >= 0 && g < D;
    float M = x[0];
#pragma unroll
    for (int i = 1; i < DCAP; ++i) M = fmaxf(M, x[i]);
    if (!live) M = 0.f;
    float Z = 0.f, Zo = 0.f, dg = 0.f;
#pragma unroll
    for (int i = 0; i < DCAP; ++i) {
        const float d = x[i] - M;                 // -inf beyond D: e = 0
        const float e = expf(d);
        x[i] = e;
        Z += e;
        if (i == (int)g) dg = d; else Zo += e;
    }
    const float rZ = live ? 1.0f / Z : 0.f, logZ = live ? logf(Z) : 0.f;
    float coef = 0.f;
    int gi = -1;
    if (valid) {
        const float w = dl_depth_weight(mask, (size_t)n * HW + pix, scale);
        const float lp = dg - logZ, om = Zo * rZ, pg = expf(dg) * rZ;
        loss = -alpha * (om * om) * lp * w;
        coef = -alpha * ((om * om) - 2.0f * om * pg * lp) * w;
        gi = (int)g;
    }
    if (grad != nullptr && live) {
#pragma unroll
        for (int i = 0; i < DCAP; ++i)
            if (i < D) grad[base + (size_t)i * HW] = valid ? coef * ((i == gi ? 1.0f : 0.f) - x[i] * rZ) : 0.f;
    }
    loss = wave_sum(loss);
    if (lane == 0) partials[tile] = loss;
}

// any D >= 1: the tile is read three times (max; sum; gradient), from L2 after the first
__global__ __launch_bounds__(256) void k_dl_depth_generic(const float* __restrict__ logit, const long long* __restrict__ index,
                                                          const float* __restrict__ mask, int D, int HW, int tiles, int total_tiles,
                                                          float alpha, float scale, float* __restrict__ grad,
                                                          float* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * DL_WAVES + wave;
    if (tile >= total_tiles) return;
    const int n = tile / tiles, pix = (tile % tiles) * DL_TILE + lane;
    const bool live = pix < HW;
    const size_t base = (size_t)n * D * HW + (size_t)pix;
    float loss = 0.f;
    if (live) {
        const long long g = index[(size_t)n * HW + pix];
        const bool valid = g >= 0 && g < D;
        float M = logit[base];
        for (int i = 1; i < D; ++i) M = fmaxf(M, logit[base + (size_t)i * HW]);
        float Z = 0.f, Zo = 0.f, dg = 0.f;
        for (int i = 0; i < D; ++i) {
            const float d = logit[base + (size_t)i * HW] - M;
            const float e = expf(d);
            Z += e;
            if (i == (int)g) dg = d; else Zo += e;
        }
        const float rZ = 1.0f / Z, logZ = logf(Z);
        float coef = 0.f;
        int gi = -1;
        if (valid) {
            const float w = dl_depth_weight(mask, (size_t)n * HW + pix, scale);
            const float lp = dg - logZ, om = Zo * rZ, pg = expf(dg) * rZ;
            loss = -alpha * (om * om) * lp * w;
            coef = -alpha * ((om * om) - 2.0f * om * pg * lp) * w;
            gi = (int)g;
        }
        if (grad != nullptr) {
            for (int i = 0; i < D; ++i) {
                const float e = expf(logit[base + (size_t)i * HW] - M);
                grad[base + (size_t)i * HW] = valid ? coef * ((i == gi ? 1.0f : 0.f) - e * rZ) : 0.f;
            }
        }
    }
    loss = wave_sum(loss);
    if (lane == 0) partials[tile] = loss;
}

// ---------------------------------------------------------------------------------------------------------- host
// (the count kernel, k_dl_finish and dl_map_ok are in loss_common.h)
static bool occ_layout(int n, int H, int W, int levels, const int* ks, OccLevels* lv) {
    if (n < 1 || H < 1 || W < 1 || levels < 1 || levels > DL_MAX_LEVELS) return false;
    if ((long long)H * W > 0x7fffffffLL / DL_MAX_A) return false;
    long long t = 0;
    lv->levels = levels;
    for (int l = 0; l < levels; ++l) {
        const int k = ks[l];
        if (k < 1 || H / k < 1 || W / k < 1) return false;
        lv->k[l] = k;
        lv->Hl[l] = H / k;
        lv->Wl[l] = W / k;
        lv->tiles[l] = (int)(((long long)lv->Hl[l] * lv->Wl[l] + DL_TILE - 1) / DL_TILE);
        lv->tile0[l] = (int)t;
        t += (long long)n * lv->tiles[l];
        if (t > 0x7fffffffLL - DL_WAVES) return false;
    }
    lv->tile0[levels] = (int)t;
    return true;
}

}  // namespace heal

using namespace heal;

extern "C" size_t heal_det_loss_workspace(int n, int anchors, int H, int W) { return dl_head_workspace(n, anchors, H, W, 3); }

extern "C" int heal_det_loss(const float* cls_preds, const float* reg_preds, const float* dir_preds, const void* pos_equal_one,
                             const void* neg_equal_one, const void* targets, int labels_f64, int n, int anchors, int H, int W,
                             float pos_cls_weight, float alpha, float sigma, float cls_weight, float reg_weight, float dir_weight,
                             const double* anchor_yaw, double dir_offset, float* terms, float* grad_cls, float* grad_reg,
                             float* grad_dir, void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(dl_head_shape_ok(n, anchors, H, W), "det_loss: bad shape n=%d anchors=%d (1..%d) H=%d W=%d", n, anchors, DL_MAX_A, H,
                 W);
    DetLaunch l{{cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, grad_cls, grad_reg, grad_dir,
                 (hipStream_t)stream}};
    if (dl_head_setup("det_loss", "cls_preds, reg_preds", cls_preds && reg_preds && pos_equal_one && neg_equal_one && targets && terms,
                      anchor_yaw, sigma, ws, ws_bytes, n, anchors, H, W, 3, l))
        return 1;
    dl_det_params(l.prm, pos_cls_weight, alpha, sigma, cls_weight, reg_weight, dir_weight, n, anchor_yaw, anchors, dir_offset);
    const FinishScales sc{{(double)l.prm.scale[0], (double)l.prm.scale[1], dir_preds != nullptr ? (double)l.prm.scale[2] : 0.0, 0.0}};
    return dl_head_run(l, labels_f64, n, anchors, 3, sc, terms);
}

extern "C" size_t heal_occ_loss_workspace(int n, int H, int W, int levels, const int* relative_downsample) {
    OccLevels lv;
    if (relative_downsample == nullptr || !occ_layout(n, H, W, levels, relative_downsample, &lv)) return 0;
    return align_up((size_t)levels * n * DL_CB * sizeof(int)) + align_up((size_t)lv.tile0[levels] * sizeof(float));
}

extern "C" int heal_occ_loss(const float* const* occ, const void* pos_equal_one, const void* neg_equal_one, int labels_f64, int n,
                             int anchors, int H, int W, int levels, const int* relative_downsample, const float* level_weight,
                             float pos_cls_weight, float alpha, float* loss, float* const* grad, void* ws, size_t ws_bytes,
                             void* stream) {
    hipStream_t s = (hipStream_t)stream;
    OccLevels lv;
    HEAL_REQUIRE(relative_downsample != nullptr && level_weight != nullptr && occ != nullptr,
                 "occ_loss: occ, relative_downsample and level_weight must be set");
    HEAL_REQUIRE(anchors >= 1 && anchors <= DL_MAX_A && occ_layout(n, H, W, levels, relative_downsample, &lv),
                 "occ_loss: bad shape n=%d anchors=%d (1..%d) H=%d W=%d levels=%d (1..%d, every H / k, W / k >= 1)", n, anchors,
                 DL_MAX_A, H, W, levels, DL_MAX_LEVELS);
    HEAL_REQUIRE(pos_equal_one && neg_equal_one && loss, "occ_loss: the labels and loss must be set");
    for (int l = 0; l < DL_MAX_LEVELS; ++l) {
        lv.occ[l] = l < levels ? occ[l] : nullptr;
        lv.grad[l] = (l < levels && grad != nullptr) ? grad[l] : nullptr;
        lv.scale[l] = l < levels ? (float)((double)level_weight[l] / n) : 0.f;
        HEAL_REQUIRE(l >= levels || lv.occ[l] != nullptr, "occ_loss: occ[%d] is NULL", l);
        if (l >= levels) { lv.k[l] = 1; lv.Hl[l] = 0; lv.Wl[l] = 0; lv.tiles[l] = 0; }
    }
    for (int l = levels + 1; l <= DL_MAX_LEVELS; ++l) lv.tile0[l] = lv.tile0[levels];
    const size_t need = heal_occ_loss_workspace(n, H, W, levels, relative_downsample);
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need, "occ_loss: workspace of %zu bytes, need %zu (heal_occ_loss_workspace)", ws_bytes,
                 need);
    Arena arena(ws, ws_bytes);
    int* counts = arena.take<int>((size_t)levels * n * DL_CB);
    float* partials = arena.take<float>((size_t)lv.tile0[levels]);
    const int total = lv.tile0[levels];
    const dim3 block(256), grid((unsigned)ceil_div(total, DL_WAVES)), cgrid(DL_CB, n, levels);
    const LaunchEvents ev = take_launch_events();
    if (labels_f64) {
        const double *p = (const double*)pos_equal_one, *q = (const double*)neg_equal_one;
        HEAL_LAUNCH_EV2(k_dl_occ_count<double>, cgrid, block, 0, s, ev.start, nullptr, p, q, anchors, H, W, lv, counts);
        HEAL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_dl_occ<double>, grid, block, 0, s, p, q, (const int*)counts, n, anchors, H, W, lv, pos_cls_weight, alpha,
                           partials);
    } else {
        const float *p = (const float*)pos_equal_one, *q = (const float*)neg_equal_one;
        HEAL_LAUNCH_EV2(k_dl_occ_count<float>, cgrid, block, 0, s, ev.start, nullptr, p, q, anchors, H, W, lv, counts);
        HEAL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_dl_occ<float>, grid, block, 0, s, p, q, (const int*)counts, n, anchors, H, W, lv, pos_cls_weight, alpha,
                           partials);
    }
    HEAL_LAUNCH_CHECK();
    FinishScales sc;
    sc.s[0] = 1.0;                                      // the partials carry their level's weight / N already
    sc.s[1] = sc.s[2] = sc.s[3] = 0.0;
    HEAL_LAUNCH_EV2(k_dl_finish, dim3(1), block, 0, s, nullptr, ev.stop, (const float*)partials, total, 1, sc, loss);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t heal_depth_focal_loss_workspace(int m, int depth_bins, int h, int w) {
    long long tiles;
    if (!dl_map_ok(m, depth_bins, h, w, &tiles)) return 0;
    return align_up((size_t)tiles * sizeof(float));
}

extern "C" int heal_depth_focal_loss(const float* depth_logit, const int64_t* depth_gt_indices, const float* fg_mask, int m,
                                     int depth_bins, int h, int w, float alpha, float weight, float* loss, float* grad, void* ws,
                                     size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    long long tiles_ll;
    HEAL_REQUIRE(dl_map_ok(m, depth_bins, h, w, &tiles_ll), "depth_focal_loss: bad shape [%d, %d, %d, %d]", m, depth_bins, h, w);
    HEAL_REQUIRE(depth_logit && depth_gt_indices && loss, "depth_focal_loss: depth_logit, depth_gt_indices and loss must be set");
    const size_t need = heal_depth_focal_loss_workspace(m, depth_bins, h, w);
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need,
                 "depth_focal_loss: workspace of %zu bytes, need %zu (heal_depth_focal_loss_workspace)", ws_bytes, need);
    const int HW = h * w, tiles = ceil_div(HW, DL_TILE), total = (int)tiles_ll, D = depth_bins;
    const float scale = (float)((double)weight / ((double)m * HW));      // the mean over M*h*w, x the depth weight
    float* partials = (float*)ws;
    const long long* idx = (const long long*)depth_gt_indices;
    const dim3 block(256), grid((unsigned)ceil_div(total, DL_WAVES));
    const LaunchEvents ev = take_launch_events();
    const int cap = (D <= 64 && D % 4 == 0) ? (D + 15) / 16 * 16 : 0;
    switch (cap) {
        case 16: HEAL_LAUNCH_EV2(k_dl_depth_regs<16>, grid, block, 0, s, ev.start, nullptr, depth_logit, idx, fg_mask, D, HW, tiles, total, alpha, scale, grad, partials); break;
        case 32: HEAL_LAUNCH_EV2(k_dl_depth_regs<32>, grid, block, 0, s, ev.start, nullptr, depth_logit, idx, fg_mask, D, HW, tiles, total, alpha, scale, grad, partials); break;
        case 48: HEAL_LAUNCH_EV2(k_dl_depth_regs<48>, grid, block, 0, s, ev.start, nullptr, depth_logit, idx, fg_mask, D, HW, tiles, total, alpha, scale, grad, partials); break;
        case 64: HEAL_LAUNCH_EV2(k_dl_depth_regs<64>, grid, block, 0, s, ev.start, nullptr, depth_logit, idx, fg_mask, D, HW, tiles, total, alpha, scale, grad, partials); break;
        default: HEAL_LAUNCH_EV2(k_dl_depth_generic, grid, block, 0, s, ev.start, nullptr, depth_logit, idx, fg_mask, D, HW, tiles, total, alpha, scale, grad, partials); break;
    }
    HEAL_LAUNCH_CHECK();
    FinishScales sc;
    sc.s[0] = 1.0;
    sc.s[1] = sc.s[2] = sc.s[3] = 0.0;
    HEAL_LAUNCH_EV2(k_dl_finish, dim3(1), block, 0, s, nullptr, ev.stop, (const float*)partials, total, 1, sc, loss);
    HEAL_LAUNCH_CHECK();
    return 0;
}
