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
// The cls, reg and dir blocks of k_ul_unc are the same functions k_dl_det calls (dl_cls_block, dl_smooth_l1, dl_dir_block of
// loss_common.h): on the same inputs their partials, and with them the finished terms and grad_cls / grad_dir, are bit-equal to
// heal_det_loss's (tests/test_gpu_unc_loss.py holds them to it).  The unc block reads the seven regression values and targets the
// reg block has loaded.  The host side -- checks, DetParams, count -> pass -> finish -- is heal_det_loss's too (dl_head_*).
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
        dl_cls_block(cls, gcls, ((size_t)n * A + a) * HW + (size_t)pix, live, pv, nv, is_pos, nrm, prm, s_cls);
        const float wr = 1.0f / nrm;
        const size_t t0 = (lab0 + a) * 7;
        // reg: seven smooth-L1 terms; the gradients and residuals stay for the unc term
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
                s_reg += dl_smooth_l1(k == 6, x, tk, wr, prm, g[k]);
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
        if (dir != nullptr)
            dl_dir_block(dir, gdir, ((size_t)n * 2 * A + (size_t)a * 2) * HW + (size_t)pix, HW, live, is_pos, tyaw, prm.yaw[a], wr, prm,
                         s_dir);
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

struct UncLaunch : HeadLaunch {
    const float* unc;
    float* gunc;
    int dim;
    UncParams prm;
    template <typename T, int A, int DIM>
    void launch_dim() const {
        hipLaunchKernelGGL((k_ul_unc<T, A, DIM>), grid, dim3(256), 0, s, cls, reg, unc, dir, (const T*)pos, (const T*)neg,
                           (const T*)tgt, (const int*)counts, HW, tiles, total, prm, gcls, greg, gunc, gdir, partials);
    }
    template <typename T, int A>
    void launch() const {
        switch (dim) {
            case 2: launch_dim<T, A, 2>(); break;
            case 3: launch_dim<T, A, 3>(); break;
            default: launch_dim<T, A, 7>(); break;
        }
    }
};

}  // namespace heal

using namespace heal;

extern "C" int heal_unc_loss_supported(int anchors, int dim, int xy_type, int angle_type, int with_dir) {
    if (anchors < 1 || anchors > DL_MAX_A || (dim != 2 && dim != 3 && dim != 7)) return 0;
    if ((xy_type != HEAL_UNC_L2 && xy_type != HEAL_UNC_L1) || (angle_type != HEAL_UNC_L2 && angle_type != HEAL_UNC_VON_MISES))
        return 0;
    return (with_dir && anchors != 2) ? 0 : 1;
}

extern "C" size_t heal_unc_loss_workspace(int n, int anchors, int H, int W) { return dl_head_workspace(n, anchors, H, W, 4); }

extern "C" int heal_unc_loss(const float* cls_preds, const float* reg_preds, const float* unc_preds, const float* dir_preds,
                             const void* pos_equal_one, const void* neg_equal_one, const void* targets, int labels_f64, int n,
                             int anchors, int H, int W, int dim, float pos_cls_weight, float alpha, float sigma, float cls_weight,
                             float reg_weight, float unc_weight, float dir_weight, int xy_type, int angle_type,
                             float angle_weight, float lambda_V, float s0, int limit_period, const double* anchor_yaw,
                             double dir_offset, float* terms, float* grad_cls, float* grad_reg, float* grad_unc, float* grad_dir,
                             void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(dl_head_shape_ok(n, anchors, H, W), "unc_loss: bad shape n=%d anchors=%d (1..%d) H=%d W=%d", n, anchors, DL_MAX_A, H,
                 W);
    HEAL_REQUIRE(heal_unc_loss_supported(anchors, dim, xy_type, angle_type, dir_preds != nullptr),
                 "unc_loss: dim=%d (2, 3, 7) xy_type=%d angle_type=%d anchors=%d%s is not supported", dim, xy_type, angle_type,
                 anchors, dir_preds ? " with a direction map (2 anchors)" : "");
    UncLaunch u{{cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, grad_cls, grad_reg, grad_dir,
                 (hipStream_t)stream}, unc_preds, grad_unc, dim};
    if (dl_head_setup("unc_loss", "cls_preds, reg_preds, unc_preds",
                      cls_preds && reg_preds && unc_preds && pos_equal_one && neg_equal_one && targets && terms, anchor_yaw, sigma, ws,
                      ws_bytes, n, anchors, H, W, 4, u))
        return 1;
    const DetParams& prm = u.prm.det;
    dl_det_params(u.prm.det, pos_cls_weight, alpha, sigma, cls_weight, reg_weight, dir_weight, n, anchor_yaw, anchors, dir_offset);
    u.prm.scale_unc = (float)((double)unc_weight / n);
    u.prm.angle_weight = angle_weight;
    u.prm.lambda_v = lambda_V;
    u.prm.s0 = s0;
    u.prm.xy_l1 = xy_type == HEAL_UNC_L1;
    u.prm.angle_vm = angle_type == HEAL_UNC_VON_MISES;
    u.prm.limit_period = limit_period != 0;
    const FinishScales sc{{(double)prm.scale[0], (double)prm.scale[1], (double)u.prm.scale_unc,
                           dir_preds != nullptr ? (double)prm.scale[2] : 0.0}};
    return dl_head_run(u, labels_f64, n, anchors, 4, sc, terms);
}
