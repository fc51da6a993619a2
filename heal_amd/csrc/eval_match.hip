// AP evaluation on the device: pairwise footprint IoU + the greedy TP / FP match of every IoU threshold, one launch pair.
//
// Reference arithmetic:
//   opencood/utils/eval_utils.py:40-91 (caluclate_tp_fp: detections in descending score, IoU against the ground-truth boxes
//   STILL UNMATCHED, max < thresh -> FP, else TP and the argmax box is popped); the IoU inside it is
//   opencood/utils/common_utils.py:230-270 (convert_format: corners 0..3, x / y; compute_iou: shapely intersection / union in
//   fp64 -> fp32) -- here quad_iou_lds, the clip K8's NMS uses, so that AP is scored with the arithmetic that produced the boxes.
// The reference copies both box sets to the host, rebuilds polygons and runs an O(N*M) Python -> GEOS loop once per threshold.
// Here:
//   k_eval_iou     one thread per (detection, ground-truth) pair of the LIVE counts (read on the device): the fp32 IoU matrix
//                  [n_cap][m_pad] in the workspace (NaN of a zero-area pair -> 0) and, per row, the maximum of every 64-column
//                  slice (one wave each)
//   k_eval_match   ONE block.  All 8 waves rank the scores by counting (descending score, equal scores by ascending index) and
//                  reduce the row maxima; then wave t walks the ranks for threshold t -- the greedy chains of different
//                  thresholds are independent -- with its alive set in registers (m_pad / 64 consecutive boxes per lane), the
//                  next row prefetched (its index is known from the order) and one 64-lane max + ballot per step: lanes hold
//                  consecutive boxes, so the first lane at the maximum holds the first maximum in ground-truth order.  A row
//                  whose maximum over ALL boxes is below the threshold is FP without entering the chain (exact: the alive
//                  maximum cannot exceed it).  Results are staged in LDS and written coalesced; the append form moves the
//                  cursor last.  No atomics: repeated launches are bit-equal.
#include "quad_iou.h"
#include "../../include/heal_amd.h"

namespace heal {

constexpr int EVAL_MAX_N = HEAL_EVAL_MAX_DET;
constexpr int EVAL_MAX_M = HEAL_EVAL_MAX_GT;
constexpr int EVAL_MAX_THR = HEAL_EVAL_MAX_THR;
constexpr int EVAL_THREADS = 64 * EVAL_MAX_THR;

struct EvalThr { float v[EVAL_MAX_THR]; };

__device__ __forceinline__ int live_count(const int32_t* dev, int cap) {
    if (dev == nullptr) return cap;
    const int v = *dev;
    return v < 0 ? 0 : (v > cap ? cap : v);
}

// footprint of box i: corners 0..3, x and y (stride 3 floats in the [.,8,3] form, 2 in the [.,4,2] form)
__device__ __forceinline__ void load_footprint(const float* __restrict__ boxes, int floats_per_box, int i, float* q) {
    const float* b = boxes + (size_t)i * floats_per_box;
    const int cs = floats_per_box == 24 ? 3 : 2;
#pragma unroll
    for (int c = 0; c < 4; ++c) { q[2 * c] = b[c * cs]; q[2 * c + 1] = b[c * cs + 1]; }
}

__global__ __launch_bounds__(256) void k_eval_iou(const float* __restrict__ det, int det_fpb, int n_cap, const int32_t* __restrict__ n_dev,
                                                 const float* __restrict__ gt, int gt_fpb, int m_cap, const int32_t* __restrict__ m_dev,
                                                 int m_pad, float* __restrict__ iou, float* __restrict__ rowpart) {
    extern __shared__ __attribute__((aligned(16))) double s_poly[];   // [32][256]
    const int n = live_count(n_dev, n_cap), m = live_count(m_dev, m_cap);
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / m_pad, j = t - i * m_pad;                       // m_pad is a multiple of 64: a wave stays in one row
    if (i >= n) return;
    float v = -1.0f;                                                  // columns past the live count: below every IoU
    if (j < m) {
        float qa[8], qb[8];
        load_footprint(det, det_fpb, i, qa);
        load_footprint(gt, gt_fpb, j, qb);
        v = quad_iou_lds<256>(qa, qb, s_poly + threadIdx.x);
        if (!(v == v)) v = 0.0f;                                      // zero-area pair: 0 / 0
        iou[(size_t)i * m_pad + j] = v;
    }
    float mx = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) rowpart[(size_t)i * (m_pad >> 6) + (j >> 6)] = mx;
}

// total order of the ranking: larger score first; -0 == +0 (as in the reference's comparison); equal scores by index
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int KPL>   // ground-truth boxes per lane = m_pad / 64
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_match(const float* __restrict__ score, int n_cap, const int32_t* __restrict__ n_dev,
                                                            int m_cap, const int32_t* __restrict__ m_dev, EvalThr thr, int n_thr,
                                                            const float* __restrict__ iou, const float* __restrict__ rowpart,
                                                            int32_t* __restrict__ out_order, uint8_t* __restrict__ out_tp,
                                                            int32_t* __restrict__ out_gt_index, float* __restrict__ out_score_sorted,
                                                            int out_stride, int32_t* cursor_dev, int32_t* gt_total_dev,
                                                            int32_t* overflow_dev) {
    constexpr int M_PAD = 64 * KPL;
    __shared__ uint32_t s_key[EVAL_MAX_N];
    __shared__ int s_order[EVAL_MAX_N];
    __shared__ float s_rowmax[EVAL_MAX_N];
    __shared__ uint8_t s_tp[EVAL_MAX_THR][EVAL_MAX_N];
    __shared__ short s_gi[EVAL_MAX_THR][EVAL_MAX_N];

    const int tid = threadIdx.x;
    const int n = live_count(n_dev, n_cap), m = live_count(m_dev, m_cap);
    int base = 0;
    if (cursor_dev != nullptr) {
        base = *cursor_dev;                                           // read by every thread before thread 0 moves it (barriers below)
        if (base < 0 || base > out_stride || n > out_stride - base) {
            if (tid == 0) *overflow_dev = 1;                          // sticky: nothing else is written, the cursor stays
            return;
        }
    }

    for (int i = tid; i < n; i += EVAL_THREADS) {
        s_key[i] = score_key(score[i]);
        float mx = rowpart[(size_t)i * KPL];
#pragma unroll
        for (int k = 1; k < KPL; ++k) mx = fmaxf(mx, rowpart[(size_t)i * KPL + k]);
        s_rowmax[i] = mx;
    }
    __syncthreads();
    for (int i = tid; i < n; i += EVAL_THREADS) {
        const uint32_t ki = s_key[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = s_key[j];
            rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
        }
        s_order[rank] = i;                                            // the order is total: every rank is taken exactly once
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    if (wave < n_thr) {
        const float th = thr.v[wave];
        bool alive[KPL];
#pragma unroll
        for (int k = 0; k < KPL; ++k) alive[k] = lane * KPL + k < m;
        float cur[KPL], nxt[KPL];
#pragma unroll
        for (int k = 0; k < KPL; ++k) cur[k] = nxt[k] = 0.0f;
        auto load_row = [&](int r, float* v) {                         // wave-uniform branch; a shortcut row is never read
            const int i = s_order[r];
            if (!(s_rowmax[i] < th)) {
                const float* p = iou + (size_t)i * M_PAD + lane * KPL;
                // one 4 / 8 / 16-byte load; columns past m hold whatever the workspace held: masked below
                if constexpr (KPL == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else if constexpr (KPL == 2) {
                    const float2 q = *reinterpret_cast<const float2*>(p);
                    v[0] = q.x; v[1] = q.y;
                } else {
                    v[0] = p[0];
                }
            }
        };
        if (n > 0) load_row(0, cur);
        for (int r = 0; r < n; ++r) {
            if (r + 1 < n) load_row(r + 1, nxt);
            const int i = s_order[r];
            int hit = -1;
            if (!(s_rowmax[i] < th)) {
                float best = -1.0f;
                int bk = 0;
#pragma unroll
                for (int k = 0; k < KPL; ++k) {
                    const float v = alive[k] ? cur[k] : -1.0f;
                    if (v > best) { best = v; bk = k; }               // strict: the first maximum of the lane's boxes
                }
                float mx = best;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                if (mx >= 0.0f && !(mx < th)) {                        // a box is left and the maximum reaches the threshold
                    const unsigned long long at = __ballot(best == mx);
                    const int first = __ffsll((long long)at) - 1;     // lanes hold consecutive boxes: the first maximum overall
                    const int k_first = __shfl(bk, first, 64);
                    hit = first * KPL + k_first;
                    if (lane == first) {
#pragma unroll
                        for (int k = 0; k < KPL; ++k) if (k == bk) alive[k] = false;
                    }
                }
            }
            if (lane == 0) {
                s_tp[wave][r] = hit >= 0 ? 1 : 0;
                s_gi[wave][r] = (short)hit;
            }
#pragma unroll
            for (int k = 0; k < KPL; ++k) cur[k] = nxt[k];
        }
    }
    __syncthreads();

    for (int r = tid; r < n; r += EVAL_THREADS) {
        const int i = s_order[r];
        out_order[base + r] = i;
        out_score_sorted[base + r] = score[i];
    }
    for (int e = tid; e < n_thr * n; e += EVAL_THREADS) {
        const int t = e / n, r = e - t * n;
        out_tp[(size_t)t * out_stride + base + r] = s_tp[t][r];
        if (out_gt_index != nullptr) out_gt_index[(size_t)t * out_stride + base + r] = (int)s_gi[t][r];
    }
    if (cursor_dev != nullptr && tid == 0) {
        *cursor_dev = base + n;
        *gt_total_dev += m;
    }
}

static int eval_m_pad(int m_cap) { return m_cap <= 64 ? 64 : (m_cap <= 128 ? 128 : 256); }

}  // namespace heal

using namespace heal;

extern "C" size_t heal_eval_match_workspace(int n_cap, int m_cap) {
    if (n_cap < 1) n_cap = 1;
    if (m_cap < 0 || m_cap > EVAL_MAX_M) m_cap = EVAL_MAX_M;
    const int m_pad = eval_m_pad(m_cap);
    return align_up((size_t)n_cap * m_pad * sizeof(float)) + align_up((size_t)n_cap * (m_pad / 64) * sizeof(float));
}

extern "C" int heal_eval_match(const float* det, int det_floats_per_box, int n, const int32_t* n_dev,
                               const float* det_score,
                               const float* gt, int gt_floats_per_box, int m, const int32_t* m_dev,
                               const float* thr_host, int n_thr,
                               int32_t* out_order, uint8_t* out_tp, int32_t* out_gt_index, float* out_score_sorted,
                               int out_stride, int32_t* cursor_dev, int32_t* gt_total_dev, int32_t* overflow_dev,
                               void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(n >= 0 && n <= EVAL_MAX_N, "heal_eval_match: n = %d (capacity 0..%d detections)", n, EVAL_MAX_N);
    HEAL_REQUIRE(m >= 0 && m <= EVAL_MAX_M, "heal_eval_match: m = %d (capacity 0..%d ground-truth boxes)", m, EVAL_MAX_M);
    HEAL_REQUIRE(thr_host != nullptr && n_thr >= 1 && n_thr <= EVAL_MAX_THR, "heal_eval_match: n_thr = %d (1..%d thresholds)", n_thr,
                 EVAL_MAX_THR);
    HEAL_REQUIRE((det_floats_per_box == 24 || det_floats_per_box == 8) && (gt_floats_per_box == 24 || gt_floats_per_box == 8),
                 "heal_eval_match: boxes are [.,8,3] (24 floats) or [.,4,2] (8 floats), got %d / %d", det_floats_per_box,
                 gt_floats_per_box);
    HEAL_REQUIRE(n == 0 || (det != nullptr && det_score != nullptr), "heal_eval_match: det / det_score is NULL with n = %d", n);
    HEAL_REQUIRE(m == 0 || gt != nullptr, "heal_eval_match: gt is NULL with m = %d", m);
    const bool append = cursor_dev != nullptr;
    if (append)
        HEAL_REQUIRE(gt_total_dev != nullptr && overflow_dev != nullptr,
                     "heal_eval_match: the append form needs gt_total_dev and overflow_dev next to cursor_dev");
    else
        HEAL_REQUIRE(out_stride >= n, "heal_eval_match: out_stride = %d is below the capacity n = %d", out_stride, n);
    if (n == 0 && !append) return 0;                                  // nothing to write, nothing to advance
    HEAL_REQUIRE(out_stride >= 0 && (n == 0 || (out_order != nullptr && out_tp != nullptr && out_score_sorted != nullptr)),
                 "heal_eval_match: out_order / out_tp / out_score_sorted is NULL");
    const int m_pad = eval_m_pad(m);
    Arena a(ws, ws_bytes);
    float* iou = a.take<float>((size_t)(n < 1 ? 1 : n) * m_pad);
    float* rowpart = a.take<float>((size_t)(n < 1 ? 1 : n) * (m_pad / 64));
    HEAL_REQUIRE(a.ok(), "heal_eval_match: workspace too small (%zu bytes, need %zu)", ws_bytes, a.off);
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        static bool attr_set = false;
        if (!attr_set) {
            HEAL_HIP(hipFuncSetAttribute((const void*)k_eval_iou, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 256 * 8));
            attr_set = true;
        }
        k_eval_iou<<<ceil_div(n * m_pad, 256), 256, 32 * 256 * 8, s>>>(det, det_floats_per_box, n, n_dev, gt, gt_floats_per_box, m, m_dev,
                                                                      m_pad, iou, rowpart);
        HEAL_LAUNCH_CHECK();
    }
    EvalThr thr;
    for (int t = 0; t < EVAL_MAX_THR; ++t) thr.v[t] = t < n_thr ? thr_host[t] : 0.0f;
#define HEAL_EVAL_LAUNCH(KPL)                                                                                                  \
    k_eval_match<KPL><<<1, EVAL_THREADS, 0, s>>>(det_score, n, n_dev, m, m_dev, thr, n_thr, iou, rowpart, out_order, out_tp,   \
                                                 out_gt_index, out_score_sorted, out_stride, cursor_dev, gt_total_dev, overflow_dev)
    if (m_pad == 64) HEAL_EVAL_LAUNCH(1);
    else if (m_pad == 128) HEAL_EVAL_LAUNCH(2);
    else HEAL_EVAL_LAUNCH(4);
#undef HEAL_EVAL_LAUNCH
    HEAL_LAUNCH_CHECK();
    return 0;
}
