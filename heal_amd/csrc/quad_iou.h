// fp64 convex quad IoU shared by K8 (k_nms_mask, k_quad_iou: decode_nms.hip) and the AP matcher (eval_match.hip): one
// arithmetic for the NMS and for the evaluation that scores its output.
#pragma once
#include "common.h"

namespace heal {

// ---- fp64 convex quad IoU (same operation order as oracle/oracle_ref.c) ---------------------------
__device__ __forceinline__ double poly_area(const double* p, int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        a += p[2 * i] * p[2 * j + 1] - p[2 * j] * p[2 * i + 1];
    }
    return 0.5 * a;
}

__device__ __forceinline__ void make_ccw(double* q, double& area) {
    area = poly_area(q, 4);
    if (area < 0.0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double tx = q[2 * i], ty = q[2 * i + 1];
            q[2 * i] = q[2 * (3 - i)]; q[2 * i + 1] = q[2 * (3 - i) + 1];
            q[2 * (3 - i)] = tx; q[2 * (3 - i) + 1] = ty;
        }
        area = -area;
    }
}

// The same clip with the two polygon buffers in LDS.  A thread-private `double buf[32]` indexed by the running vertex count lives
// in SCRATCH memory: every vertex of every edge pass is then a dependent store -> load round trip to L2 (k_nms_mask: 30 us for
// two clips per thread).  Layout: element e (= 2 * vertex + coordinate, < 16: clipping a convex quad by four half planes
// leaves at most 8 vertices) of thread t at buf[e * NT + t] -- consecutive lanes, consecutive words, whatever e each lane is at.
template <int NT>
__device__ __forceinline__ int clip_edge_lds(const double* subj, int ns, double ax, double ay, double bx, double by, double* out) {
    int no = 0;
    const double ex = bx - ax, ey = by - ay;
    for (int i = 0; i < ns; ++i) {
        const int j = (i + 1 == ns) ? 0 : i + 1;
        const double px = subj[(2 * i) * NT], py = subj[(2 * i + 1) * NT];
        const double qx = subj[(2 * j) * NT], qy = subj[(2 * j + 1) * NT];
        const double dp = ex * (py - ay) - ey * (px - ax);
        const double dq = ex * (qy - ay) - ey * (qx - ax);
        const bool pin = dp >= 0.0, qin = dq >= 0.0;
        if (pin) {
            if (no < 8) { out[(2 * no) * NT] = px; out[(2 * no + 1) * NT] = py; }
            ++no;
        }
        if (pin != qin) {
            const double t = dp / (dp - dq);
            if (no < 8) { out[(2 * no) * NT] = px + t * (qx - px); out[(2 * no + 1) * NT] = py + t * (qy - py); }
            ++no;
        }
    }
    return no < 8 ? no : 8;
}

template <int NT>
__device__ __forceinline__ float quad_iou_lds(const float* qa, const float* qb, double* lds /* this thread's column of [32][NT] */) {
    double a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = (double)qa[i]; b[i] = (double)qb[i]; }
    double sa, sb;
    make_ccw(a, sa);
    make_ccw(b, sb);
    double* cur = lds;
    double* nxt = lds + 16 * NT;
#pragma unroll
    for (int i = 0; i < 8; ++i) cur[i * NT] = a[i];
    int n = 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int f = (e + 1) & 3;
        if (n > 0) {
            n = clip_edge_lds<NT>(cur, n, b[2 * e], b[2 * e + 1], b[2 * f], b[2 * f + 1], nxt);
            double* t = cur; cur = nxt; nxt = t;
        }
    }
    double inter = 0.0;
    if (n >= 3) {
        for (int i = 0; i < n; ++i) {
            const int j = (i + 1 == n) ? 0 : i + 1;
            inter += cur[(2 * i) * NT] * cur[(2 * j + 1) * NT] - cur[(2 * j) * NT] * cur[(2 * i + 1) * NT];
        }
        inter = 0.5 * inter;
    }
    if (inter < 0.0) inter = 0.0;
    const double uni = sa + sb - inter;
    return (float)(inter / uni);
}

}  // namespace heal
