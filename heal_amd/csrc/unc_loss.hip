// UL -- the criterion of CoAlign's uncertainty detector: the four terms (cls, reg, unc, dir) and the gradients of the four head
// maps in one streaming pass (include/heal_amd_unc.h).
//
// Reference arithmetic: opencood/loss/point_pillar_uncertainty_loss.py:24-124 (forward) and :195-293 (KLLoss).  The torch
// composition is PointPillarLoss's plus one more permuted copy (the uncertainty map), the 8-wide concatenations of
// add_sin_difference_and_angle, float64 arithmetic wherever a float64 label meets a float32 map, and all of it once more in
// backward.  Here the layout of k_dl_det (det_loss.hip): a WAVE owns 64 consecutive pixels of one image, every channel row of the
// tile is one 256-B access, the labels are read where they lie, no LDS, no barrier, no floating-point atomic.  Phases: k_dl_count
// (integer positives per sample), k_ul_unc (gradients + one partial per tile and term), k_dl_finish (fixed-order fp64 sums).
//
// The cls, reg and dir blocks of k_ul_unc are k_dl_det's, statement by statement: on the same inputs their partials, and with
// them the finished terms and grad_cls / grad_dir, are bit-equal to heal_det_loss's (tests/test_gpu_unc_loss.py holds them to it).
// The unc block reads the seven regression values and targets the reg block has loaded.
#include "loss_common.h"
#include "../../include/heal_amd_unc.h"

namespace heal {

struct UncParams {
    DetParams det;
    float scale_unc;              // uncertainty weight / N
    float angle_weight, lambda_v, s0;
    int xy_l1, angle_vm, limit_period;
};

// ---------------------------------------------------------------------------------------------------------- Bessel
// Cephes' Chebyshev expansions of exp(-x) I0(x) and exp(-x) I1(x) (x >= 0), two intervals split at 8, evaluated in fp32 by the
// recurrence of chbevl.  The coefficients are the tail of the double tables that reaches fp32: a coefficient adds at most its own
// magnitude (|T_i| <= 1) to a value of 0.1 .. 1, so what lies below 1e-9 is dropped -- for i1e these are the float tables of
// ATen/native/Math.h (chebyshev_coefficients_i1e_A/B<float>), for i0e the same cut of chebyshev_coefficients_i0e_A/B.
template <int LEN>
__device__ __forceinline__ float ul_chbevl(float x, const float (&c)[LEN]) {
    float b0 = c[0], b1 = 0.f, b2 = 0.f;
#pragma unroll
    for (int i = 1; i < LEN; ++i) {
        b2 = b1;
        b1 = b0;
        b0 = x * b1 - b2 + c[i];
    }
    return 0.5f * (b0 - b2);
}

__device__ __forceinline__ float ul_i0e(float x) {
    constexpr float A[18] = {-1.30002500998624804212E-8f, 6.04699502254191894932E-8f,  -2.67079385394061173391E-7f,
                             1.11738753912010371815E-6f,  -4.41673835845875056359E-6f, 1.64484480707288970893E-5f,
                             -5.75419501008210370398E-5f, 1.88502885095841655729E-4f,  -5.76375574538582365885E-4f,
                             1.63947561694133579842E-3f,  -4.32430999505057594430E-3f, 1.05464603945949983183E-2f,
                             -2.37374148058994688156E-2f, 4.93052842396707084878E-2f,  -9.49010970480476444210E-2f,
                             1.71620901522208775349E-1f,  -3.04682672343198398683E-1f, 6.76795274409476084995E-1f};
    constexpr float B[7] = {3.39623202570838634515E-9f, 2.26666899049817806459E-8f, 2.04891858946906374183E-7f,
                            2.89137052083475648297E-6f, 6.88975834691682398426E-5f, 3.36911647825569408990E-3f,
                            8.04490411014108831608E-1f};
    if (x <= 8.0f) return ul_chbevl(x / 2.0f - 2.0f, A);
    return ul_chbevl(32.0f / x - 2.0f, B) / sqrtf(x);
}

__device__ __forceinline__ float ul_i1e(float x) {
    constexpr float A[17] = {9.38153738649577178388E-9f,  -4.44505912879632808065E-8f, 2.00329475355213526229E-7f,
                             -8.56872026469545474066E-7f, 3.47025130813767847674E-6f,  -1.32731636560394358279E-5f,
                             4.78156510755005422638E-5f,  -1.61760815825896745588E-4f, 5.12285956168575772895E-4f,
                             -1.51357245063125314899E-3f, 4.15642294431288815669E-3f,  -1.05640848946261981558E-2f,
                             2.47264490306265168283E-2f,  -5.29459812080949914269E-2f, 1.02643658689847095384E-1f,
                             -1.76416518357834055153E-1f, 2.52587186443633654823E-1f};
    constexpr float B[7] = {-3.83538038596423702205E-9f, -2.63146884688951950684E-8f, -2.51223623787020892529E-7f,
                            -3.88256480887769039346E-6f, -1.10588938762623716291E-4f, -9.76109749136146840777E-3f,
                            7.78576235018280120474E-1f};
    if (x <= 8.0f) return ul_chbevl(x / 2.0f - 2.0f, A) * x;
    return ul_chbevl(32.0f / x - 2.0f, B) / sqrtf(x);
}

// ---------------------------------------------------------------------------------------------------------- KL terms
// kl_loss_l2 (:219-228): 0.5 (exp(-s) d^2 + s);  kl_loss_l1 (:231-240): 0.5 exp(-s) |d| + s.  -> loss, d/dd, d/ds
__device__ __forceinline__ void ul_xy(float d, float s, bool l1, float& loss, float& dd, float& ds) {
    const float e = expf(-s);
    if (l1) {
        const float ad = fabsf(d);
        loss = 0.5f * e * ad + s;
        dd = d > 0.f ? 0.5f * e : (d < 0.f ? -0.5f * e : 0.f);
        ds = 1.0f - 0.5f * e * ad;
    } else {
        loss = 0.5f * (e * (d * d) + s);
        dd = e * d;
        ds = 0.5f * (1.0f - e * (d * d));
    }
}

// kl_loss_angular (:243-260) with log I0(k) = log(i0e(k)) + k (finite where the reference's log(i0e(k) exp(k)) is inf)
__device__ __forceinline__ void ul_von_mises(float d, float s, const UncParams& p, float& loss, float& dd, float& ds) {
    const float k = expf(-s);
    const float c = p.limit_period ? fabsf(cosf(d)) : cosf(d);
    const float i0 = ul_i0e(k), i1 = ul_i1e(k);
    const float z = s - p.s0;
    const float elu = z > 0.f ? z : expm1f(z), delu = z > 0.f ? 1.0f : expf(z);
    loss = logf(i0) + k * (1.0f - c) + p.lambda_v * elu;
    ds = k * (c - i1 / i0) + p.lambda_v * delu;
    dd = p.limit_period ? 0.f : k * sinf(d);
}

// ---------------------------------------------------------------------------------------------------------- the pass
template <typename T, int A, int DIM>
__global__ __launch_bounds__(256) void k_ul_unc(const float* __restrict__ cls, const float* __restrict__ reg,
                                                const float* __restrict__ unc, const float* __restrict__ dir,
                                                const T* __restrict__ pos, const T* __restrict__ neg, const T* __restrict__ tgt,
                                                const int* __restrict__ counts, int HW, int tiles, int total_tiles,
                                                UncParams up, float* __restrict__ gcls, float* __restrict__ greg,
                                                float* __restrict__ gunc, float* __restrict__ gdir,
                                                float* __restrict__ partials) {
    const DetParams& prm = up.det;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * DL_WAVES + wave;
    if (tile >= total_tiles) return;                      // wave-uniform; the waves of a block share nothing
    const int n = tile / tiles, pix = (tile % tiles) * DL_TILE + lane;
    const bool live = pix < HW;                           // the tail of an image is masked, never read or written
    const float nrm = dl_normaliser(counts, n, lane);
    const size_t lab0 = ((size_t)n * HW + (size_t)pix) * A;
    float s_cls = 0.f, s_reg = 0.f, s_dir = 0.f, s_unc = 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float pv = live ? (float)pos[lab0 + a] : 0.f;
        const float nv = live ? (float)neg[lab0 + a] : 0.f;
        const bool is_pos = pv > 0.f;
        // cls (k_dl_det)
        {
            const size_t at = ((size_t)n * A + a) * HW + (size_t)pix;
            const float x = live ? cls[at] : 0.f;
            const float w = ((is_pos ? prm.pos_cls_weight : 0.f) + (nv > 0.f ? 1.0f : 0.f)) / nrm;
            float l, dx;
            dl_focal(x, pv, w, prm.alpha, l, dx);
            if (w == 0.f) { l = 0.f; dx = 0.f; }          // pos = neg = 0: exactly nothing, whatever the logit
            s_cls += l;
            if (gcls != nullptr && live) gcls[at] = dx * prm.scale[0];
        }
        const float wr = 1.0f / nrm;
        const size_t t0 = (lab0 + a) * 7;
        // reg (k_dl_det): seven smooth-L1 terms, the yaw as sin(a) cos(b) against cos(a) sin(b); the values stay for the unc term
        float tyaw_f = 0.f;
        double tyaw = 0.0;
        if (is_pos) {
            tyaw = (double)tgt[t0 + 6];
            tyaw_f = (float)tyaw;
        }
        float g[7], diff[7];                              // d term / d reg; the raw residual x - target (0 for a NaN target)
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const size_t at = ((size_t)n * 7 * A + (size_t)a * 7 + k) * HW + (size_t)pix;
            g[k] = 0.f;
            diff[k] = 0.f;
            if (is_pos) {
                const float x = reg[at];
                const float tk = k == 6 ? tyaw_f : (float)tgt[t0 + k];
                float d, chain = 1.0f;
                if (k == 6) {
                    const float sa = sinf(x), ca = cosf(x), sb = sinf(tyaw_f), cb = cosf(tyaw_f);
                    d = sa * cb - ca * sb;
                    chain = ca * cb + sa * sb;
                } else {
                    d = x - tk;
                }
                const float ad = fabsf(d);
                const bool small = ad <= prm.inv_sigma2;
                const float l = small ? 0.5f * (ad * ad) * prm.sigma2 : ad - 0.5f * prm.inv_sigma2;
                const float dl = small ? d * prm.sigma2 : (d > 0.f ? 1.0f : -1.0f);
                s_reg += l * wr;
                g[k] = dl * chain * wr * prm.scale[1];
                diff[k] = tk != tk ? 0.f : x - tk;
            }
        }
        // unc: component j of the anchor's DIM channels against residual j (0..5), the last one of dim 3 / 7 against the raw yaw
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            const size_t at = ((size_t)n * DIM * A + (size_t)a * DIM + j) * HW + (size_t)pix;
            const bool angle = DIM != 2 && j == DIM - 1;
            const int k = angle ? 6 : j;
            float gs = 0.f;
            if (is_pos) {
                const float s = unc[at];
                float l, dd, ds;
                if (DIM == 3 && angle) {
                    if (up.angle_vm) ul_von_mises(diff[k], s, up, l, dd, ds);
                    else ul_xy(diff[k], s, false, l, dd, ds);
                    l = up.angle_weight * l;
                    dd = up.angle_weight * dd;
                    ds = up.angle_weight * ds;
                } else {
                    ul_xy(diff[k], s, up.xy_l1 != 0, l, dd, ds);
                }
                s_unc += l * wr;
                g[k] += dd * wr * up.scale_unc;
                gs = ds * wr * up.scale_unc;
            }
            if (gunc != nullptr && live) gunc[at] = gs;
        }
        if (greg != nullptr && live) {
#pragma unroll
            for (int k = 0; k < 7; ++k) greg[((size_t)n * 7 * A + (size_t)a * 7 + k) * HW + (size_t)pix] = g[k];
        }
        // dir (k_dl_det): two-bin cross-entropy = softplus(other - chosen)
        if (dir != nullptr) {
            const size_t at0 = ((size_t)n * 2 * A + (size_t)a * 2) * HW + (size_t)pix;
            float g0 = 0.f, g1 = 0.f;
            if (is_pos) {
                const double two_pi = 6.283185307179586476925286766559, pi = 3.141592653589793238462643383279;
                const double v = (tyaw + prm.yaw[a]) - prm.dir_offset;
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
    }
    s_cls = wave_sum(s_cls);
    s_reg = wave_sum(s_reg);
    s_unc = wave_sum(s_unc);
    s_dir = wave_sum(s_dir);
    if (lane == 0) {
        partials[tile] = s_cls;
        partials[(size_t)total_tiles + tile] = s_reg;
        partials[(size_t)2 * total_tiles + tile] = s_unc;
        partials[(size_t)3 * total_tiles + tile] = s_dir;
    }
}

struct UncLaunch {
    const float *cls, *reg, *unc, *dir;
    const void *pos, *neg, *tgt;
    const int* counts;
    int HW, tiles, total;
    UncParams prm;
    float *gcls, *greg, *gunc, *gdir, *partials;
    dim3 grid;
    hipStream_t s;
};

template <typename T, int A, int DIM>
static void ul_launch(const UncLaunch& u) {
    hipLaunchKernelGGL((k_ul_unc<T, A, DIM>), u.grid, dim3(256), 0, u.s, u.cls, u.reg, u.unc, u.dir, (const T*)u.pos,
                       (const T*)u.neg, (const T*)u.tgt, u.counts, u.HW, u.tiles, u.total, u.prm, u.gcls, u.greg, u.gunc, u.gdir,
                       u.partials);
}

template <typename T, int A>
static void ul_launch_dim(const UncLaunch& u, int dim) {
    switch (dim) {
        case 2: ul_launch<T, A, 2>(u); break;
        case 3: ul_launch<T, A, 3>(u); break;
        default: ul_launch<T, A, 7>(u); break;
    }
}

template <typename T>
static void ul_launch_anchors(const UncLaunch& u, int anchors, int dim) {
    switch (anchors) {
        case 1: ul_launch_dim<T, 1>(u, dim); break;
        case 2: ul_launch_dim<T, 2>(u, dim); break;
        case 3: ul_launch_dim<T, 3>(u, dim); break;
        default: ul_launch_dim<T, 4>(u, dim); break;
    }
}

}  // namespace heal

using namespace heal;

extern "C" int heal_unc_loss_supported(int anchors, int dim, int xy_type, int angle_type, int with_dir) {
    if (anchors < 1 || anchors > DL_MAX_A || (dim != 2 && dim != 3 && dim != 7)) return 0;
    if ((xy_type != HEAL_UNC_L2 && xy_type != HEAL_UNC_L1) || (angle_type != HEAL_UNC_L2 && angle_type != HEAL_UNC_VON_MISES))
        return 0;
    return (with_dir && anchors != 2) ? 0 : 1;
}

extern "C" size_t heal_unc_loss_workspace(int n, int anchors, int H, int W) {
    long long tiles;
    if (anchors > DL_MAX_A || !dl_map_ok(n, 7 * anchors, H, W, &tiles)) return 0;
    return align_up((size_t)n * DL_CB * sizeof(int)) + align_up((size_t)4 * tiles * sizeof(float));
}

extern "C" int heal_unc_loss(const float* cls_preds, const float* reg_preds, const float* unc_preds, const float* dir_preds,
                             const void* pos_equal_one, const void* neg_equal_one, const void* targets, int labels_f64, int n,
                             int anchors, int H, int W, int dim, float pos_cls_weight, float alpha, float sigma, float cls_weight,
                             float reg_weight, float unc_weight, float dir_weight, int xy_type, int angle_type,
                             float angle_weight, float lambda_V, float s0, int limit_period, const double* anchor_yaw,
                             double dir_offset, float* terms, float* grad_cls, float* grad_reg, float* grad_unc, float* grad_dir,
                             void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    long long tiles_ll;
    HEAL_REQUIRE(anchors >= 1 && anchors <= DL_MAX_A && dl_map_ok(n, 7 * anchors, H, W, &tiles_ll),
                 "unc_loss: bad shape n=%d anchors=%d (1..%d) H=%d W=%d", n, anchors, DL_MAX_A, H, W);
    HEAL_REQUIRE(heal_unc_loss_supported(anchors, dim, xy_type, angle_type, dir_preds != nullptr),
                 "unc_loss: dim=%d (2, 3, 7) xy_type=%d angle_type=%d anchors=%d%s is not supported", dim, xy_type, angle_type,
                 anchors, dir_preds ? " with a direction map (2 anchors)" : "");
    HEAL_REQUIRE(cls_preds && reg_preds && unc_preds && pos_equal_one && neg_equal_one && targets && terms,
                 "unc_loss: cls_preds, reg_preds, unc_preds, the three labels and terms must be set");
    HEAL_REQUIRE(dir_preds == nullptr || anchor_yaw != nullptr, "unc_loss: dir_preds needs anchor_yaw[anchors]");
    HEAL_REQUIRE(dir_preds != nullptr || grad_dir == nullptr, "unc_loss: grad_dir without dir_preds");
    HEAL_REQUIRE(sigma > 0.f, "unc_loss: sigma must be positive, got %g", (double)sigma);
    const size_t need = heal_unc_loss_workspace(n, anchors, H, W);
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need, "unc_loss: workspace of %zu bytes, need %zu (heal_unc_loss_workspace)", ws_bytes,
                 need);
    Arena arena(ws, ws_bytes);
    int* counts = arena.take<int>((size_t)n * DL_CB);
    float* partials = arena.take<float>((size_t)4 * tiles_ll);
    UncLaunch u;
    u.HW = H * W;
    u.tiles = ceil_div(u.HW, DL_TILE);
    u.total = (int)tiles_ll;
    DetParams& prm = u.prm.det;
    prm.pos_cls_weight = pos_cls_weight;
    prm.alpha = alpha;
    prm.sigma2 = sigma * sigma;
    prm.inv_sigma2 = 1.0f / (sigma * sigma);
    prm.scale[0] = (float)((double)cls_weight / n);
    prm.scale[1] = (float)((double)reg_weight / n);
    prm.scale[2] = (float)((double)dir_weight / n);
    for (int a = 0; a < DL_MAX_A; ++a) prm.yaw[a] = (anchor_yaw != nullptr && a < anchors) ? anchor_yaw[a] : 0.0;
    prm.dir_offset = dir_offset;
    u.prm.scale_unc = (float)((double)unc_weight / n);
    u.prm.angle_weight = angle_weight;
    u.prm.lambda_v = lambda_V;
    u.prm.s0 = s0;
    u.prm.xy_l1 = xy_type == HEAL_UNC_L1;
    u.prm.angle_vm = angle_type == HEAL_UNC_VON_MISES;
    u.prm.limit_period = limit_period != 0;
    u.cls = cls_preds; u.reg = reg_preds; u.unc = unc_preds; u.dir = dir_preds;
    u.pos = pos_equal_one; u.neg = neg_equal_one; u.tgt = targets;
    u.counts = counts;
    u.gcls = grad_cls; u.greg = grad_reg; u.gunc = grad_unc; u.gdir = grad_dir;
    u.partials = partials;
    u.grid = dim3((unsigned)ceil_div(u.total, DL_WAVES));
    u.s = s;
    const long long per_sample = (long long)u.HW * anchors;
    const dim3 block(256), cgrid(DL_CB, n);
    const LaunchEvents ev = take_launch_events();
    if (labels_f64) {
        HEAL_LAUNCH_EV2(k_dl_count<double>, cgrid, block, 0, s, ev.start, nullptr, (const double*)pos_equal_one, per_sample, counts);
        HEAL_LAUNCH_CHECK();
        ul_launch_anchors<double>(u, anchors, dim);
    } else {
        HEAL_LAUNCH_EV2(k_dl_count<float>, cgrid, block, 0, s, ev.start, nullptr, (const float*)pos_equal_one, per_sample, counts);
        HEAL_LAUNCH_CHECK();
        ul_launch_anchors<float>(u, anchors, dim);
    }
    HEAL_LAUNCH_CHECK();
    FinishScales sc;
    sc.s[0] = (double)prm.scale[0];
    sc.s[1] = (double)prm.scale[1];
    sc.s[2] = (double)u.prm.scale_unc;
    sc.s[3] = dir_preds != nullptr ? (double)prm.scale[2] : 0.0;
    HEAL_LAUNCH_EV2(k_dl_finish, dim3(1), block, 0, s, nullptr, ev.stop, (const float*)partials, u.total, 4, sc, terms);
    HEAL_LAUNCH_CHECK();
    return 0;
}
