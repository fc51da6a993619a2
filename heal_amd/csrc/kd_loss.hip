// KD -- DiscoNet's distillation term and its gradient with respect to the student, in one pass over both maps.
//
// Reference arithmetic: opencood/loss/point_pillar_disconet_loss.py:35-46
//     KLDivLoss(size_average=True, reduce=True)(log_softmax(S', 1), softmax(T', 1)),   S', T' = [N,C,H,W] permuted to [N*H*W, C]
// i.e. per pixel the channel softmax of both maps, sum_c p_t (log p_t - log p_s), and the MEAN OVER ELEMENTS (N*C*H*W, not
// pixels).  Under autograd the student receives (p_s - p_t) / (N*C*H*W).
//
// The torch composition makes two permuted copies, a log_softmax, a softmax, the pointwise kl_div, a mean and their mirror image
// in backward.  Here a block owns 64 consecutive pixels of one image of the NCHW maps: lanes run along pixels (every channel
// row of the tile is one 256-B access of a wave), its four waves (eight for C = 256) split the channels, and for C in {64, 128,
// 256} each lane keeps its 16 or 32 student and as many teacher logits in registers -- every input byte is read once, the gradient is written once.  The
// waves merge their (max, sum) pairs through LDS with the online-softmax rule.  Any other C >= 1 takes k_kd_generic, the same
// arithmetic with the tile re-read from L2 in each of its three passes.
//
// Arithmetic per pixel and map: M = max_c x, d = x - M, e = exp(d), Z = sum_c e, p = e * (1 / Z), log p = d - log Z.  The student and
// the teacher go through the SAME inlined instruction sequence (the library is built with -ffp-contract=off), so student ==
// teacher gives log p_t - log p_s == 0 and p_s - p_t == 0 exactly.  A teacher probability that underflows to 0 contributes
// 0 * finite = 0 (torch's kl_div for a zero target); d is clamped at -3e38 so that logits 6e38 apart cannot make it -inf and the
// difference of two log-probabilities NaN.  exp(d) is v_exp_f32(d * log2 e): d <= 0 is exact or rounded once, and the
// product's rounding moves p by less than |d| * 2^-23 * p <= 5e-8.
//
// Reduction: no floating-point atomics.  Lane sums over channels in index order -> the waves' sums in wave order -> xor
// tree over the 64 lanes -> partial[block] (already divided by the element count); k_dl_finish (loss_common.h: one block, one term,
// scale 1) adds the partials in a fixed order in fp64.  Two launches on the same values are bit-equal wherever the data lies: no
// path depends on an address.
#include "loss_common.h"

namespace heal {

constexpr int KD_TILE = 64;      // pixels per block = lanes per wave
constexpr int KD_WAVES = 4;     // of the generic kernel
constexpr float KD_LOG2E = 1.44269504088896340736f;
constexpr float KD_DMIN = -3.0e38f;

__device__ __forceinline__ float kd_exp(float d) { return __builtin_amdgcn_exp2f(d * KD_LOG2E); }   // d <= 0; exp(-inf) = 0

// merge the waves' (m, z) of one map: every wave computes the same (M, log Z, 1/Z) from the same LDS entries, in wave order
template <int WAVES>
__device__ __forceinline__ void kd_merge(const float* __restrict__ sm, const float* __restrict__ sz, int lane, float& M,
                                         float& logZ, float& rZ) {
    float m = sm[lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = fmaxf(m, sm[w * KD_TILE + lane]);
    float z = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) z += sz[w * KD_TILE + lane] * kd_exp(fmaxf(sm[w * KD_TILE + lane] - m, KD_DMIN));
    M = m;
    logZ = logf(z);      // z >= 1: the channel holding the maximum contributes exp(0)
    rZ = 1.0f / z;
}

// one element's share of the mean KL and of the gradient.  qs, qt = 1 / (Z * count): the probabilities are formed already divided
// by the element count, so that the sums stay below max |log p_t - log p_s| / C and cannot overflow for any finite input
__device__ __forceinline__ void kd_term(float xs, float xt, float Ms, float logZs, float qs, float Mt, float logZt, float qt,
                                        float& kl, float& g) {
    const float ds = fmaxf(xs - Ms, KD_DMIN), dt = fmaxf(xt - Mt, KD_DMIN);
    const float ps = kd_exp(ds) * qs, pt = kd_exp(dt) * qt;
    const float ls = ds - logZs, lt = dt - logZt;
    kl += pt * (lt - ls);
    g = ps - pt;
}

template <int WAVES>
__device__ __forceinline__ void kd_block_partial(float kl, float* __restrict__ skl, int wave, int lane,
                                                 float* __restrict__ partials) {
    skl[wave * KD_TILE + lane] = kl;
    __syncthreads();
    if (wave == 0) {
        float v = skl[lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += skl[w * KD_TILE + lane];
        v = wave_sum(v);
        if (lane == 0) partials[blockIdx.x] = v;
    }
}

// register-resident: WAVES waves of CPW channels each, C = WAVES * CPW.  64 values of each map per lane (C = 256 on four waves)
// compile to 204 VGPRs, two waves per SIMD; 32 + 32 compile to 108, four waves per SIMD, so C = 256 runs on eight waves
template <int CPW, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_kd_regs(const float* __restrict__ student, const float* __restrict__ teacher, int HW,
                                                 int tiles, float inv_count, float* __restrict__ grad,
                                                 float* __restrict__ partials) {
    __shared__ float sred[4][WAVES * KD_TILE];
    __shared__ float skl[WAVES * KD_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = blockIdx.x / tiles, pix0 = (blockIdx.x % tiles) * KD_TILE;
    const bool live = pix0 + lane < HW;                           // the H*W tail of an image is masked, never read or written
    // wave-uniform row base (scalar registers) + the lane: one address register serves every load and store
    const size_t base = ((size_t)n * (WAVES * CPW) + (size_t)wave * CPW) * HW + pix0;
    const float* __restrict__ sp = student + base;
    const float* __restrict__ tp = teacher + base;
    float xs[CPW], xt[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i) xs[i] = live ? sp[(size_t)i * HW + (unsigned)lane] : 0.f;
#pragma unroll
    for (int i = 0; i < CPW; ++i) xt[i] = live ? tp[(size_t)i * HW + (unsigned)lane] : 0.f;
    float ms = xs[0], mt = xt[0];
#pragma unroll
    for (int i = 1; i < CPW; ++i) { ms = fmaxf(ms, xs[i]); mt = fmaxf(mt, xt[i]); }
    float zs = 0.f, zt = 0.f;
#pragma unroll
    for (int i = 0; i < CPW; ++i) { zs += kd_exp(fmaxf(xs[i] - ms, KD_DMIN)); zt += kd_exp(fmaxf(xt[i] - mt, KD_DMIN)); }
    sred[0][wave * KD_TILE + lane] = ms;
    sred[1][wave * KD_TILE + lane] = zs;
    sred[2][wave * KD_TILE + lane] = mt;
    sred[3][wave * KD_TILE + lane] = zt;
    __syncthreads();
    float Ms, logZs, rZs, Mt, logZt, rZt;
    kd_merge<WAVES>(sred[0], sred[1], lane, Ms, logZs, rZs);
    kd_merge<WAVES>(sred[2], sred[3], lane, Mt, logZt, rZt);
    const float qs = rZs * inv_count, qt = rZt * inv_count;
    float kl = 0.f;
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        float g;
        kd_term(xs[i], xt[i], Ms, logZs, qs, Mt, logZt, qt, kl, g);
        if (grad != nullptr && live) grad[base + (size_t)i * HW + (unsigned)lane] = g;
    }
    kd_block_partial<WAVES>(live ? kl : 0.f, skl, wave, lane, partials);
}

// any C >= 1: wave w owns channels [w * per, min(C, (w + 1) * per)), per = ceil(C / 4) (possibly none: m = -inf, z = 0 drop out
// of the merge); the tile (64 pixels x C) is read three times, from L2 after the first
__global__ __launch_bounds__(256) void k_kd_generic(const float* __restrict__ student, const float* __restrict__ teacher, int C,
                                                    int HW, int tiles, float inv_count, float* __restrict__ grad,
                                                    float* __restrict__ partials) {
    __shared__ float sred[4][KD_WAVES * KD_TILE];
    __shared__ float skl[KD_WAVES * KD_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, pix = (blockIdx.x % tiles) * KD_TILE + lane;
    const bool live = pix < HW;
    const int per = (C + KD_WAVES - 1) / KD_WAVES;
    const int c0 = min(wave * per, C), c1 = min(c0 + per, C);
    const size_t base = (size_t)n * C * HW + pix;
    float ms = -INFINITY, mt = -INFINITY;
    for (int c = c0; c < c1; ++c) {
        const float a = live ? student[base + (size_t)c * HW] : 0.f, b = live ? teacher[base + (size_t)c * HW] : 0.f;
        ms = fmaxf(ms, a);
        mt = fmaxf(mt, b);
    }
    float zs = 0.f, zt = 0.f;
    for (int c = c0; c < c1; ++c) {
        const float a = live ? student[base + (size_t)c * HW] : 0.f, b = live ? teacher[base + (size_t)c * HW] : 0.f;
        zs += kd_exp(fmaxf(a - ms, KD_DMIN));
        zt += kd_exp(fmaxf(b - mt, KD_DMIN));
    }
    sred[0][wave * KD_TILE + lane] = ms;
    sred[1][wave * KD_TILE + lane] = zs;
    sred[2][wave * KD_TILE + lane] = mt;
    sred[3][wave * KD_TILE + lane] = zt;
    __syncthreads();
    float Ms, logZs, rZs, Mt, logZt, rZt;
    kd_merge<KD_WAVES>(sred[0], sred[1], lane, Ms, logZs, rZs);
    kd_merge<KD_WAVES>(sred[2], sred[3], lane, Mt, logZt, rZt);
    const float qs = rZs * inv_count, qt = rZt * inv_count;
    float kl = 0.f;
    for (int c = c0; c < c1; ++c) {
        const float a = live ? student[base + (size_t)c * HW] : 0.f, b = live ? teacher[base + (size_t)c * HW] : 0.f;
        float g;
        kd_term(a, b, Ms, logZs, qs, Mt, logZt, qt, kl, g);
        if (grad != nullptr && live) grad[base + (size_t)c * HW] = g;
    }
    kd_block_partial<KD_WAVES>(live ? kl : 0.f, skl, wave, lane, partials);
}

static bool kd_shape_ok(int n, int channels, int H, int W, long long* blocks) {
    if (n < 1 || channels < 1 || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL - KD_TILE) return false;
    const long long b = (long long)n * ((hw + KD_TILE - 1) / KD_TILE);
    if (b > 0x7fffffffLL) return false;
    *blocks = b;
    return true;
}

}  // namespace heal

using namespace heal;

extern "C" size_t heal_kd_kl_loss_workspace(int n, int channels, int H, int W) {
    long long blocks;
    if (!kd_shape_ok(n, channels, H, W, &blocks)) return 0;
    return align_up((size_t)blocks * sizeof(float));
}

extern "C" int heal_kd_kl_loss(const float* student, const float* teacher, int n, int channels, int H, int W, float* loss,
                               float* grad, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    long long blocks;
    HEAL_REQUIRE(kd_shape_ok(n, channels, H, W, &blocks), "kd_kl_loss: bad shape [%d, %d, %d, %d]", n, channels, H, W);
    HEAL_REQUIRE(student != nullptr && teacher != nullptr && loss != nullptr, "kd_kl_loss: student, teacher and loss must be set");
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= (size_t)blocks * sizeof(float),
                 "kd_kl_loss: workspace of %zu bytes, need %zu (heal_kd_kl_loss_workspace)", ws_bytes,
                 (size_t)blocks * sizeof(float));
    const int HW = H * W, tiles = ceil_div(HW, KD_TILE);
    const double count = (double)n * channels * (double)HW;
    const float inv_count = (float)(1.0 / count);
    float* partials = (float*)ws;
    const dim3 grid((unsigned)blocks), block(256);
    const LaunchEvents ev = take_launch_events();
    switch (channels) {
        case 64: HEAL_LAUNCH_EV2((k_kd_regs<16, 4>), grid, block, 0, s, ev.start, nullptr, student, teacher, HW, tiles, inv_count, grad, partials); break;
        case 128: HEAL_LAUNCH_EV2((k_kd_regs<32, 4>), grid, block, 0, s, ev.start, nullptr, student, teacher, HW, tiles, inv_count, grad, partials); break;
        case 256: HEAL_LAUNCH_EV2((k_kd_regs<32, 8>), grid, dim3(512), 0, s, ev.start, nullptr, student, teacher, HW, tiles, inv_count, grad, partials); break;
        default: HEAL_LAUNCH_EV2(k_kd_generic, grid, block, 0, s, ev.start, nullptr, student, teacher, channels, HW, tiles, inv_count, grad, partials); break;
    }
    HEAL_LAUNCH_CHECK();
    const FinishScales sc{{1.0, 0.0, 0.0, 0.0}};            // one term; (float)(acc * 1.0) == (float)acc
    HEAL_LAUNCH_EV2(k_dl_finish, dim3(1), block, 0, s, nullptr, ev.stop, (const float*)partials, (int)blocks, 1, sc, loss);
    HEAL_LAUNCH_CHECK();
    return 0;
}
