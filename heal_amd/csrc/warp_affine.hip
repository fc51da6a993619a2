// warp_affine_simple as a stand-alone differentiable operator (include/heal_amd_train_warp.h): every agent of a scene warped into
// the ego frame in one launch, NCHW in and out, and the adjoint of that warp in gather form.
//
// Reference arithmetic: opencood/models/sub_modules/torch_transformation_utils.py:323-332 (warp_affine_simple =
// F.affine_grid(M, size, align_corners=False).to(src) + F.grid_sample(bilinear, zeros padding, align_corners=False)), the first step
// of every fusion of fusion_in_one.py and of every level of heter_model_baseline_ms.py:199-207.  Under autograd the library's
// grid_sample backward scatters with float atomics (two runs of a training step differ in the last bits) and affine_grid +
// grid_sample stream the [n, H, W, 2] grid besides the maps.  Here the forward is the sampling code of K5 (warp_taps.h: bit-equal to
// heal_warp_agent) and the backward GATHERS: a thread owns a source pixel, finds the destination pixels that can have it among
// their four taps from the inverse of the row's pixel-space map, re-runs the forward's own grid_point + make_taps on each candidate
// and adds w * G where a tap is its pixel.  Membership and weights are therefore exactly the forward's; the candidate box only has
// to be a superset.  No atomics, no zero fill, bit-equal across launches.
#include <math.h>
#include "common.h"
#include "warp_taps.h"
#include "../../include/heal_amd_train_warp.h"

namespace heal {

constexpr int WAF_TW = 32, WAF_TH = 8, WAF_CCH = 16;       // forward: the tile and channel chunk of k_warp_agent
constexpr int WAB_TW = 16, WAB_TH = 4;                     // backward: one wave = 16 x 4 source pixels, lanes along x
constexpr int WAB_CCH = HEAL_WARP_BWD_CHANNELS;            // channels per thread: the candidates' taps are computed once per chunk

struct WarpAffineParams {
    AffineRows rows;
    int n, C, H, W, cchunks;
};

__global__ __launch_bounds__(256) void k_warp_affine_forward(const float* __restrict__ src, WarpAffineParams p,
                                                            float* __restrict__ out) {
    const Block3 bk = xcd_block();
    const int w = bk.x * WAF_TW + (threadIdx.x & (WAF_TW - 1));
    const int h = bk.y * WAF_TH + (threadIdx.x / WAF_TW);
    if (w >= p.W || h >= p.H) return;
    const int a = bk.z / p.cchunks, c0 = (bk.z - a * p.cchunks) * WAF_CCH;
    const int HW = p.H * p.W;
    const Taps t = affine_taps(p.rows, a, h, w, p.H, p.W);
    const int pix = h * p.W + w;
    const float* __restrict__ s = src + ((size_t)a * p.C + c0) * HW;
    float* __restrict__ o = out + ((size_t)a * p.C + c0) * HW + pix;
#pragma unroll 4
    for (int c = 0; c < WAF_CCH && c0 + c < p.C; ++c) o[(size_t)c * HW] = sample(s + (size_t)c * HW, t, p.W);
}

struct WarpAffineBwdParams {
    double m[WF_MAXA][6];     // the forward's rows
    double win[WF_MAXA][8];   // heal_warp_affine_window: Ainv (4), b (2), r_x + margin, r_y + margin
    int n, C, H, W, cchunks;
};

// clamp(v, lo, hi) in double before the conversion: the centre of an agent far outside the map may not fit an int
__device__ __forceinline__ int to_index(double v, int lo, int hi) { return (int)fmin(fmax(v, (double)lo), (double)hi); }

template <typename T>
__global__ __launch_bounds__(WAB_TW * WAB_TH) void k_warp_affine_backward(const float* __restrict__ gout, WarpAffineBwdParams p,
                                                                         float* __restrict__ gsrc) {
    const int sx = blockIdx.x * WAB_TW + (threadIdx.x & (WAB_TW - 1));
    const int sy = blockIdx.y * WAB_TH + (threadIdx.x / WAB_TW);
    if (sx >= p.W || sy >= p.H) return;
    const int a = blockIdx.z / p.cchunks, c0 = (blockIdx.z - a * p.cchunks) * WAB_CCH;
    const int H = p.H, W = p.W, HW = H * W;
    const int nc = min(WAB_CCH, p.C - c0);
    double m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = p.m[a][k];
    // the candidates: integer d within (r_x, r_y) of Ainv (s - b), clipped to the map (an empty range: no contributor)
    const double* q = p.win[a];
    const double ex = (double)sx - q[4], ey = (double)sy - q[5];
    const double cx = q[0] * ex + q[1] * ey, cy = q[2] * ex + q[3] * ey;
    const int w_lo = to_index(ceil(cx - q[6]), 0, W), w_hi = to_index(floor(cx + q[6]), -1, W - 1);
    const int h_lo = to_index(ceil(cy - q[7]), 0, H), h_hi = to_index(floor(cy + q[7]), -1, H - 1);
    const int sidx = sy * W + sx;
    float acc[WAB_CCH];
#pragma unroll
    for (int u = 0; u < WAB_CCH; ++u) acc[u] = 0.f;
    const float* __restrict__ g0 = gout + ((size_t)a * p.C + c0) * HW;
    for (int h = h_lo; h <= h_hi; ++h) {
        const T ys = base_coord<T>(h, H);
        for (int w = w_lo; w <= w_hi; ++w) {
            float gx, gy;
            grid_from_base<T>(m, base_coord<T>(w, W), ys, gx, gy);      // = grid_point<T>(m, h, w, H, W, gx, gy)
            const Taps t = make_taps(gx, gy, H, W);
            // a tap inside the map has index t.off + (0, 1, W, W + 1) (make_taps' clamps are inactive for it): at most one is s
            const int o4[4] = {t.off, t.off + 1, t.off + W, t.off + W + 1};
            float wk = 0.f;
            bool hit = false;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((t.ok >> k) & 1u) && o4[k] == sidx) { wk = t.w[k]; hit = true; }
            if (!hit) continue;
            const float* __restrict__ g = g0 + (size_t)h * W + w;
#pragma unroll
            for (int u = 0; u < WAB_CCH; ++u)
                if (u < nc) acc[u] = acc[u] + wk * g[(size_t)u * HW];
        }
    }
    float* __restrict__ o = gsrc + ((size_t)a * p.C + c0) * HW + sidx;
#pragma unroll
    for (int u = 0; u < WAB_CCH; ++u)
        if (u < nc) o[(size_t)u * HW] = acc[u];
}

// The window of one row (host).  Returns null, or why the backward does not take the row.
static const char* warp_window(const double* row, int H, int W, double* out) {
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return "H, W >= 1 and H * W <= 2^30";
    for (int k = 0; k < 6; ++k)
        if (!isfinite(row[k])) return "an entry of the row is not finite";
    const double rw = (double)W / (double)H, rh = (double)H / (double)W;
    const double a00 = row[0], a01 = row[1] * rw, a10 = row[3] * rh, a11 = row[4];
    const double det = a00 * a11 - a01 * a10;
    if (!(fabs(det) >= 1e-9)) return "the row is singular (|det A| < 1e-9)";
    const double i00 = a11 / det, i01 = -a01 / det, i10 = -a10 / det, i11 = a00 / det;
    const double rx = fabs(i00) + fabs(i01), ry = fabs(i10) + fabs(i11);
    if (!(rx <= HEAL_WARP_BWD_MAX_REACH && ry <= HEAL_WARP_BWD_MAX_REACH)) return "the reach exceeds HEAL_WARP_BWD_MAX_REACH";
    // p(d) = A d + b from ix = ((gx + 1) W - 1) / 2 with base(w, W) = (2 w + 1 - W) / W
    const double bx = a00 * (0.5 - 0.5 * W) + a01 * (0.5 - 0.5 * H) + (row[2] + 1.0) * 0.5 * W - 0.5;
    const double by = a10 * (0.5 - 0.5 * W) + a11 * (0.5 - 0.5 * H) + (row[5] + 1.0) * 0.5 * H - 0.5;
    const double margin = 0.01 + ldexp((double)(H > W ? H : W), -20);
    out[0] = i00; out[1] = i01; out[2] = i10; out[3] = i11;
    out[4] = bx; out[5] = by; out[6] = rx + margin; out[7] = ry + margin;
    return nullptr;
}

}  // namespace heal

using namespace heal;

extern "C" int heal_warp_affine_forward(const float* src, int n, int C, int H, int W, const double* affine_host,
                                        const double* affine_dev, int grid_f64, float* out, void* stream) {
    HEAL_REQUIRE(n >= 1 && n <= WF_MAXA, "warp_affine_forward: n must be in [1,%d] (got %d)", WF_MAXA, n);
    HEAL_REQUIRE(C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= (1ll << 30), "warp_affine_forward: bad shape (%d, %d, %d)", C, H, W);
    HEAL_REQUIRE(src && out, "warp_affine_forward: null pointer");
    WarpAffineParams p;
    if (fill_affine_rows(p.rows, "warp_affine_forward", affine_host, affine_dev, n, grid_f64)) return 1;
    p.n = n; p.C = C; p.H = H; p.W = W; p.cchunks = ceil_div(C, WAF_CCH);
    HEAL_REQUIRE((long long)n * p.cchunks <= 65535, "warp_affine_forward: n * ceil(C / %d) must not exceed 65535", WAF_CCH);
    HEAL_REQUIRE(ceil_div(H, WAF_TH) <= 65535, "warp_affine_forward: H must not exceed %d", 65535 * WAF_TH);
    dim3 grid(ceil_div(W, WAF_TW), ceil_div(H, WAF_TH), n * p.cchunks);
    HEAL_LAUNCH_EV(k_warp_affine_forward, grid, dim3(256), 0, (hipStream_t)stream, src, p, out);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" int heal_warp_affine_backward_supported(const double* affine_host, int n, int H, int W) {
    if (n < 1 || n > WF_MAXA || affine_host == nullptr) return 0;
    double win[8];
    for (int a = 0; a < n; ++a)
        if (warp_window(affine_host + a * 6, H, W, win)) return 0;
    return 1;
}

extern "C" int heal_warp_affine_window(const double* row, int H, int W, double* out) {
    HEAL_REQUIRE(row && out, "warp_affine_window: null pointer");
    const char* why = warp_window(row, H, W, out);
    HEAL_REQUIRE(why == nullptr, "warp_affine_window: %s", why);
    return 0;
}

extern "C" int heal_warp_affine_backward(const float* grad_out, int n, int C, int H, int W, const double* affine_host, int grid_f64,
                                         float* grad_src, void* stream) {
    HEAL_REQUIRE(n >= 1 && n <= WF_MAXA, "warp_affine_backward: n must be in [1,%d] (got %d)", WF_MAXA, n);
    HEAL_REQUIRE(C >= 1, "warp_affine_backward: bad channel count %d", C);
    HEAL_REQUIRE(grad_out && grad_src, "warp_affine_backward: null pointer");
    HEAL_REQUIRE(affine_host != nullptr, "warp_affine_backward: the rows must come from the host");
    WarpAffineBwdParams p;
    p.n = n; p.C = C; p.H = H; p.W = W; p.cchunks = ceil_div(C, WAB_CCH);
    HEAL_REQUIRE((long long)n * p.cchunks <= 65535, "warp_affine_backward: n * ceil(C / %d) must not exceed 65535", WAB_CCH);
    HEAL_REQUIRE(H >= 1 && ceil_div(H, WAB_TH) <= 65535, "warp_affine_backward: H must be in [1,%d]", 65535 * WAB_TH);
    for (int a = 0; a < WF_MAXA; ++a) {
        for (int k = 0; k < 6; ++k) p.m[a][k] = 0.0;
        for (int k = 0; k < 8; ++k) p.win[a][k] = 0.0;
    }
    for (int a = 0; a < n; ++a) {
        const char* why = warp_window(affine_host + a * 6, H, W, p.win[a]);
        HEAL_REQUIRE(why == nullptr, "warp_affine_backward: row %d on a %d x %d map is not supported: %s", a, H, W, why);
        for (int k = 0; k < 6; ++k) p.m[a][k] = affine_host[a * 6 + k];
    }
    dim3 grid(ceil_div(W, WAB_TW), ceil_div(H, WAB_TH), n * p.cchunks);
    hipStream_t st = (hipStream_t)stream;
    if (grid_f64) HEAL_LAUNCH_EV(k_warp_affine_backward<double>, grid, dim3(WAB_TW * WAB_TH), 0, st, grad_out, p, grad_src);
    else HEAL_LAUNCH_EV(k_warp_affine_backward<float>, grid, dim3(WAB_TW * WAB_TH), 0, st, grad_out, p, grad_src);
    HEAL_LAUNCH_CHECK();
    return 0;
}
