// PG -- CoAlign's agent-object pose graph (box alignment) for a batch of samples: clustering of every agent's boxes into
// landmarks and the whole Levenberg-Marquardt solve in one workgroup per sample (include/heal_amd_pose.h).
//
// Reference: box_alignment_relative_sample_np (opencood/models/sub_modules/box_align_v2.py:105-400); the optimiser g2o runs there
// is replaced by the solve below.  heal_amd/opencood/models/sub_modules/pose_graph_optim.py is the same algorithm in numpy and
// the place where cost, damping and stopping rule are written out; the two are kept step for step alike.
//
//   k_pg_prepare   one thread per box: corner_to_center in the agent's frame (the measurement), the 6-DoF projection into the world
//                  frame and corner_to_center again (centre, yaw), the certainties exp(-log sigma^2) -> a 16-double row per box.
//   k_pg_solve     one 256-thread workgroup per sample.
//                  clustering: the seed loop is sequential and uniform over the block; each seed's row of the distance matrix is
//                  evaluated across the lanes (4 boxes per thread at HEAL_POSE_MAX_BOXES) against the bit set of unassigned boxes;
//                  ballots and per-wave counts give every new member its place in the edge list, in ascending box order.
//                  solve: per iteration one thread per landmark linearises its edges (3x3 block, right-hand side, one coupling
//                  block per agent -> workspace); the Schur complement onto the 3 (N - 1) agent unknowns is summed per matrix
//                  entry over the landmarks in index order; Cholesky of the <= 21 x 21 system (right-hand side carried as an extra
//                  row) and the back substitution run in LDS; each landmark back-substitutes its own update and evaluates its
//                  edges at the trial point; the block-wide sums are fixed trees.
// No floating-point atomic, no dependence on the batch around a sample: results are bit-equal across launches and compositions.
// Every loop is bounded by a count that does not depend on the data converging (seeds <= boxes, iterations <= max_iterations,
// trials <= PG_MAX_TRIALS); every branch around a barrier is uniform over the block (taken on values all threads read from LDS
// after a barrier, or carry in registers computed from such values).
#include "common.h"
#include "../../include/heal_amd_pose.h"

namespace heal {

constexpr int PG_THREADS = 256;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_MAXB = HEAL_POSE_MAX_BOXES;
constexpr int PG_MAXL = PG_MAXB / 2;              // a landmark holds at least two boxes
constexpr int PG_MAXA = HEAL_POSE_MAX_AGENTS;
constexpr int PG_KPT = PG_MAXB / PG_THREADS;      // boxes per thread in the neighbour test
constexpr int PG_NMAX = 3 * (PG_MAXA - 1);        // agent unknowns
constexpr int PG_ROW = 16;                        // doubles per box in the table
constexpr int PG_LROW = PG_MAXA * 18 + 18;        // doubles per landmark in the workspace
constexpr int PG_MAX_TRIALS = 10;
constexpr double PG_TAU = 1e-5, PG_POLISH = 1e-13, PG_STEP_FLOOR = 1e-14;
constexpr double PG_PI = 3.141592653589793, PG_DEG = 0.017453292519943295, PG_RAD = 57.29577951308232;
constexpr double PG_ANCHOR_DIAG2 = 1.6 * 1.6 + 3.9 * 3.9;
constexpr double PG_MAX_DIST = 10000.0, PG_UNSURE = 100.0;
static_assert(PG_MAXB % PG_THREADS == 0 && PG_MAXL == 2 * PG_THREADS, "the sums below take two landmarks per thread");

// box table row
enum { T_MX = 0, T_MY, T_MYAW, T_CZ, T_SZ, T_W0, T_W1, T_W2, T_WX, T_WY, T_WZ, T_WYAW, T_AA, T_FINITE };
// landmark workspace row: [agent][18] = A(6 sym) b(3) W(9), then
enum { L_HLL = PG_MAXA * 18, L_BL = L_HLL + 6, L_MINV = L_BL + 3, L_YL = L_MINV + 6 };
// landmark flags
enum { F_SE2 = 1, F_ACTIVE = 2, F_VARIES = 4, F_DOUBLED = 8 };

__device__ __forceinline__ double pg_wrap(double t) { return t - 2.0 * PG_PI * ceil((t - PG_PI) / (2.0 * PG_PI)); }
__device__ __forceinline__ bool pg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// corner_to_center (box_utils.py:25-84) of one box: centre = mean of corners 0, 3, 5, 6; yaw = plain mean of four arctan2
__device__ __forceinline__ void pg_center(const double (&c)[8][3], double& x, double& y, double& z, double& yaw) {
    x = (((c[0][0] + c[3][0]) + c[5][0]) + c[6][0]) / 4.0;
    y = (((c[0][1] + c[3][1]) + c[5][1]) + c[6][1]) / 4.0;
    z = (((c[0][2] + c[3][2]) + c[5][2]) + c[6][2]) / 4.0;
    yaw = (((atan2(c[1][1] - c[2][1], c[1][0] - c[2][0]) + atan2(c[0][1] - c[3][1], c[0][0] - c[3][0])) +
            atan2(c[5][1] - c[6][1], c[5][0] - c[6][0])) + atan2(c[4][1] - c[7][1], c[4][0] - c[7][0])) / 4.0;
}

__global__ __launch_bounds__(256) void k_pg_prepare(const double* __restrict__ corners, const int32_t* __restrict__ box_offsets,
                                                    const double* __restrict__ pose, const double* __restrict__ log_sigma2,
                                                    int total_agents, int total_boxes, int normalize,
                                                    double* __restrict__ table) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total_boxes) return;
    double* row = table + (size_t)j * PG_ROW;
    // the agent that owns box j: the last a with box_offsets[a] <= j (offsets that are not monotone are caught by k_pg_solve)
    int lo = 0, hi = total_agents;                      // invariant: the answer lies in [lo, hi)
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if (box_offsets[mid] <= j) lo = mid; else hi = mid;
    }
    const double* p = pose + (size_t)lo * 6;
    double c[8][3];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            c[k][d] = corners[(size_t)j * 24 + k * 3 + d];
            fin = fin && pg_finite(c[k][d]);
        }
#pragma unroll
    for (int d = 0; d < 6; ++d) fin = fin && pg_finite(p[d]);
    double mx, my, mz, myaw;
    pg_center(c, mx, my, mz, myaw);
    // pose_to_tfm (transformation_utils.py:94-162), 6-DoF, degrees, CARLA convention
    const double cy = cos(p[4] * PG_DEG), sy = sin(p[4] * PG_DEG), cr = cos(p[3] * PG_DEG), sr = sin(p[3] * PG_DEG);
    const double cp = cos(p[5] * PG_DEG), sp = sin(p[5] * PG_DEG);
    const double r00 = cp * cy, r01 = cy * sp * sr - sy * cr, r02 = -cy * sp * cr - sy * sr;
    const double r10 = sy * cp, r11 = sy * sp * sr + cy * cr, r12 = -sy * sp * cr + cy * sr;
    const double r20 = sp, r21 = -cp * sr, r22 = cp * cr;
    double w[8][3];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[k][0] = ((r00 * c[k][0] + r01 * c[k][1]) + r02 * c[k][2]) + p[0];
        w[k][1] = ((r10 * c[k][0] + r11 * c[k][1]) + r12 * c[k][2]) + p[1];
        w[k][2] = ((r20 * c[k][0] + r21 * c[k][1]) + r22 * c[k][2]) + p[2];
    }
    double wx, wy, wz, wyaw;
    pg_center(w, wx, wy, wz, wyaw);
    double c0 = 1.0, c1 = 1.0, c2 = 1.0;
    if (log_sigma2 != nullptr) {
        c0 = exp(-log_sigma2[(size_t)j * 3 + 0]) / PG_ANCHOR_DIAG2;
        c1 = exp(-log_sigma2[(size_t)j * 3 + 1]) / PG_ANCHOR_DIAG2;
        c2 = exp(-log_sigma2[(size_t)j * 3 + 2]);
        if (normalize) { c0 = sqrt(c0); c1 = sqrt(c1); c2 = sqrt(c2); }
        fin = fin && pg_finite(c0) && pg_finite(c1) && pg_finite(c2);
    }
    row[T_MX] = mx; row[T_MY] = my; row[T_MYAW] = myaw; row[T_CZ] = cos(myaw); row[T_SZ] = sin(myaw);
    row[T_W0] = c0; row[T_W1] = c1; row[T_W2] = c2;
    row[T_WX] = wx; row[T_WY] = wy; row[T_WZ] = wz; row[T_WYAW] = wyaw;
    row[T_AA] = (wx * wx + wy * wy) + wz * wz;
    row[T_FINITE] = fin && pg_finite(myaw) && pg_finite(wyaw) && pg_finite(row[T_AA]) ? 1.0 : 0.0;
    row[14] = 0.0; row[15] = 0.0;
}

// One edge at (xi = agent pose with its cos / sin, xj = landmark): the error and the two Jacobians (pose_graph_optim.linearize).
struct PgEdge { double zx, zy, zyaw, cz, sz, w0, w1, w2; };

__device__ __forceinline__ PgEdge pg_load_edge(const double* __restrict__ row, int flags) {
    PgEdge m;
    const double s = (flags & F_DOUBLED) ? 2.0 : 1.0;
    m.zx = row[T_MX]; m.zy = row[T_MY];
    m.w0 = row[T_W0] * s; m.w1 = row[T_W1] * s;
    if (flags & F_SE2) { m.zyaw = pg_wrap(row[T_MYAW]); m.cz = row[T_CZ]; m.sz = row[T_SZ]; m.w2 = row[T_W2] * s; }
    else { m.zyaw = 0.0; m.cz = 1.0; m.sz = 0.0; m.w2 = 0.0; }
    return m;
}

__device__ __forceinline__ void pg_error(const double* xi, double ci, double si, const double* xj, const PgEdge& m, double (&e)[3],
                                         double& d0, double& d1) {
    const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
    d0 = ci * dx + si * dy;
    d1 = -si * dx + ci * dy;
    const double u0 = d0 - m.zx, u1 = d1 - m.zy;
    e[0] = m.cz * u0 + m.sz * u1;
    e[1] = -m.sz * u0 + m.cz * u1;
    e[2] = m.w2 != 0.0 ? pg_wrap(xj[2] - xi[2] - m.zyaw) : 0.0;
}

__device__ __forceinline__ double pg_chi(const double (&e)[3], const PgEdge& m) {
    return (m.w0 * e[0] * e[0] + m.w1 * e[1] * e[1]) + m.w2 * e[2] * e[2];
}

// sym 3x3 as [00, 01, 02, 11, 12, 22]
__device__ __forceinline__ int pg_sym(int r, int c) {
    if (r > c) { const int t = r; r = c; c = t; }
    return r == 0 ? c : (r == 1 ? 2 + c : 5);
}

// two block-wide sums over PG_MAXL slots each (a, b in LDS; every slot written, zeros beyond the live ones): a fixed tree
__device__ __forceinline__ void pg_reduce2(double* a, double* b, int tid, double& ra, double& rb) {
    __syncthreads();
    for (int s = PG_MAXL / 2; s >= 1; s >>= 1) {
        if (tid < s) { a[tid] += a[tid + s]; b[tid] += b[tid + s]; }
        __syncthreads();
    }
    ra = a[0]; rb = b[0];
    __syncthreads();
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_solve(
    const double* __restrict__ table, const int32_t* __restrict__ box_offsets, const int32_t* __restrict__ agent_offsets,
    const double* __restrict__ pose, int has_unc, int total_agents, int total_boxes, int options, double thres, double yaw_var_thres,
    int max_iterations, double* __restrict__ lws, int lws_rows, double* __restrict__ refined, int32_t* __restrict__ cluster_out,
    double* __restrict__ stats) {
    // ---- LDS -------------------------------------------------------------------------------------------------------------
    __shared__ double s_u[4 * PG_MAXB];                 // clustering: wc[3 * MAXB], aa[MAXB]; solve: xl, xlt [3 * MAXL], red [2 * MAXL]
    __shared__ int s_cluster[PG_MAXB];
    __shared__ unsigned short s_edge_box[PG_MAXB];      // edge list: local box index, grouped by landmark, seed first
    __shared__ unsigned short s_lm_start[PG_MAXL + 1];
    __shared__ unsigned char s_edge_on[PG_MAXB];
    __shared__ unsigned char s_agent_of[PG_MAXB];
    __shared__ unsigned char s_lm_flags[PG_MAXL];
    __shared__ unsigned char s_lm_mask[PG_MAXL];        // agents (bit a) with an active edge into the landmark
    __shared__ unsigned int s_free[PG_MAXB / 32];       // bit set of unassigned boxes
    __shared__ double s_S[(PG_NMAX + 1) * PG_NMAX];     // Schur system (lower triangle); row nu_dim = right-hand side
    __shared__ double s_ldiag[PG_NMAX], s_yv[PG_NMAX], s_xv[PG_NMAX];
    __shared__ double s_xa[PG_MAXA * 3], s_xat[PG_MAXA * 3], s_x0[PG_MAXA * 3], s_da[PG_MAXA * 3];
    __shared__ double s_haa[PG_MAXA * 6], s_ba[PG_MAXA * 3];
    __shared__ int s_off[PG_MAXA + 1];
    __shared__ int s_wcount[PG_KPT * PG_WAVES];
    __shared__ int s_ints[8];                           // 0 bad input, 1 any neighbour, 2 yaw-varying landmarks, 3 active edges,
                                                        // 4 agents with an active edge (mask), 5 solve failed
    __shared__ unsigned long long s_stepmax;

    double* s_wc = s_u;
    double* s_aa = s_u + 3 * PG_MAXB;
    double* s_xl = s_u;
    double* s_xlt = s_u + 3 * PG_MAXL;
    double* s_red = s_u + 6 * PG_MAXL;
    double* s_red2 = s_u + 7 * PG_MAXL;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int smp = blockIdx.x;
    int a0 = agent_offsets[smp], a1 = agent_offsets[smp + 1];
    const bool agents_ok = a0 >= 0 && a1 >= a0 && a1 <= total_agents;
    if (!agents_ok) {                                    // no valid place to write poses: only the status
        if (tid == 0 && stats) {
            for (int k = 0; k < HEAL_POSE_STATS; ++k) stats[(size_t)smp * HEAL_POSE_STATS + k] = 0.0;
            stats[(size_t)smp * HEAL_POSE_STATS + HEAL_POSE_STAT_STATUS] = HEAL_POSE_STATUS_NONFINITE;
        }
        return;
    }
    const int N = a1 - a0;
    if (tid < 8) s_ints[tid] = 0;
    if (tid == 0) s_stepmax = 0ull;
    if (tid <= PG_MAXA) s_off[tid] = tid <= N && tid <= PG_MAXA && N <= PG_MAXA ? box_offsets[a0 + tid] : 0;
    __syncthreads();
    bool shape_ok = N >= 1 && N <= PG_MAXA;
    int b0 = 0, n = 0;
    if (shape_ok) {
        b0 = s_off[0];
        n = s_off[N] - b0;
        shape_ok = b0 >= 0 && n >= 0 && n <= PG_MAXB && b0 + n <= total_boxes;
        for (int a = 0; a < N; ++a) shape_ok = shape_ok && s_off[a + 1] >= s_off[a];
    }
    if (!shape_ok) n = 0;
    const int NB = N >= 1 && N <= PG_MAXA ? N : 0;       // agents whose poses may be read and written

    // ---- inputs: the agent of every box, finiteness, start poses ----------------------------------------------------------
    for (int j = tid; j < n; j += PG_THREADS) {
        int a = 0;
        for (int k = 1; k < N; ++k) a += (b0 + j >= s_off[k]) ? 1 : 0;
        s_agent_of[j] = (unsigned char)a;
        s_cluster[j] = -1;
        const double* row = table + (size_t)(b0 + j) * PG_ROW;
        s_wc[3 * j + 0] = row[T_WX]; s_wc[3 * j + 1] = row[T_WY]; s_wc[3 * j + 2] = row[T_WZ];
        s_aa[j] = row[T_AA];
        if (row[T_FINITE] != 1.0) atomicOr(&s_ints[0], 1);
    }
    if (tid < PG_MAXB / 32) {
        const int lo = tid * 32;
        s_free[tid] = n >= lo + 32 ? 0xffffffffu : (n > lo ? ((1u << (n - lo)) - 1u) : 0u);
    }
    if (tid < NB) {
        const double* p = pose + (size_t)(a0 + tid) * 6;
        bool fin = true;
        for (int d = 0; d < 6; ++d) fin = fin && pg_finite(p[d]);
        if (!fin) atomicOr(&s_ints[0], 1);
        s_x0[3 * tid + 0] = p[0]; s_x0[3 * tid + 1] = p[1]; s_x0[3 * tid + 2] = pg_wrap(p[4] * PG_DEG);
        s_xa[3 * tid + 0] = p[0]; s_xa[3 * tid + 1] = p[1]; s_xa[3 * tid + 2] = s_x0[3 * tid + 2];
    }
    __syncthreads();
    const bool bad_input = !shape_ok || s_ints[0] != 0;

    int nl = 0, ne = 0;                                  // landmarks, edge-list length: uniform over the block
    int status = HEAL_POSE_STATUS_NO_EDGES, iterations = 0, total_trials = 0;
    double chi = 0.0, chi_initial = 0.0, lam = 0.0;
    bool give_noisy = bad_input;
    if (bad_input) status = HEAL_POSE_STATUS_NONFINITE;

    // ---- clustering (box_align_v2.py:208-291) ------------------------------------------------------------------------------
    if (!bad_input) {
        for (int seed = 0; seed < n; ++seed) {           // <= n seeds; a seed that is taken costs one LDS read
            if (!((s_free[seed >> 5] >> (seed & 31)) & 1u)) continue;
            const double sx = s_wc[3 * seed], sy = s_wc[3 * seed + 1], sz = s_wc[3 * seed + 2], saa = s_aa[seed];
            const int sa = s_agent_of[seed];
            bool nb[PG_KPT];
            bool any = false;
#pragma unroll
            for (int k = 0; k < PG_KPT; ++k) {
                const int j = k * PG_THREADS + tid;
                bool near = false, open = false;
                if (j < n) {
                    // all_pair_l2 (:83-100): sqrt(|a|^2 + |b|^2 - 2 a.b); a NaN compares false; one agent's own pairs are MAX_DIST
                    const double two_ab = ((2.0 * sx) * s_wc[3 * j] + (2.0 * sy) * s_wc[3 * j + 1]) + (2.0 * sz) * s_wc[3 * j + 2];
                    double d = sqrt((saa + s_aa[j]) - two_ab);
                    if (s_agent_of[j] == sa) d = PG_MAX_DIST;
                    near = d < thres;
                    open = (s_free[j >> 5] >> (j & 31)) & 1u;
                }
                any = any || near;
                nb[k] = near && open;
                const unsigned long long bal = __ballot(nb[k]);
                if (lane == 0) s_wcount[k * PG_WAVES + wave] = __popcll(bal);
            }
            if (any) atomicOr(&s_ints[1], 1);
            __syncthreads();
            int total = 0;                               // all members; base_k: those ahead of this thread's wave in round k
            int base_k[PG_KPT];
#pragma unroll
            for (int k = 0; k < PG_KPT; ++k)
                for (int w = 0; w < PG_WAVES; ++w) {
                    if (w == 0) base_k[k] = total;
                    const int c = s_wcount[k * PG_WAVES + w];
                    if (w < wave) base_k[k] += c;
                    total += c;
                }
            const bool any_nb = s_ints[1] != 0;
            __syncthreads();                             // everybody has read the counts and the flag
            if (tid == 0) s_ints[1] = 0;
            if (total == 0) {
                if (any_nb && tid == 0) s_free[seed >> 5] &= ~(1u << (seed & 31));   // every neighbour is taken: the seed leaves
                __syncthreads();
                continue;
            }
            // a new landmark: the seed, then its unassigned neighbours in ascending box order
#pragma unroll
            for (int k = 0; k < PG_KPT; ++k) {
                const unsigned long long bal = __ballot(nb[k]);
                if (nb[k]) {
                    const int j = k * PG_THREADS + tid;
                    const int pos = ne + 1 + base_k[k] + __popcll(bal & ((1ull << lane) - 1ull));
                    s_edge_box[pos] = (unsigned short)j;       // pos <= ne + total < n: the members are distinct unassigned boxes
                    s_cluster[j] = nl;
                    atomicAnd(&s_free[j >> 5], ~(1u << (j & 31)));
                }
            }
            if (tid == 0) {
                s_edge_box[ne] = (unsigned short)seed;
                s_cluster[seed] = nl;
                atomicAnd(&s_free[seed >> 5], ~(1u << (seed & 31)));
                s_lm_start[nl] = (unsigned short)ne;
            }
            ne += 1 + total;
            nl += 1;
            __syncthreads();
        }
        if (tid == 0) s_lm_start[nl] = (unsigned short)ne;
        __syncthreads();
    }
    if (cluster_out != nullptr)
        for (int j = tid; j < n; j += PG_THREADS) cluster_out[b0 + j] = bad_input ? -1 : s_cluster[j];
    __syncthreads();                                     // the clustering arrays in s_u are dead from here

    // ---- landmarks: yaw variance, kind, start value, edges (:253-291, :306-388) ---------------------------------------------
    const bool opt_se2 = options & HEAL_POSE_LANDMARK_SE2, opt_adaptive = options & HEAL_POSE_ADAPTIVE_LANDMARK;
    if (!bad_input) {
        for (int l = tid; l < nl; l += PG_THREADS) {
            const int e0 = s_lm_start[l], e1 = s_lm_start[l + 1];
            double sum = 0.0;
            for (int p = e0; p < e1; ++p) sum += table[(size_t)(b0 + s_edge_box[p]) * PG_ROW + T_WYAW];
            const double mean = sum / (double)(e1 - e0);
            double var = 0.0;
            for (int p = e0; p < e1; ++p) {
                const double d = table[(size_t)(b0 + s_edge_box[p]) * PG_ROW + T_WYAW] - mean;
                var += d * d;
            }
            var = var / (double)(e1 - e0);
            const bool varies = var > yaw_var_thres;
            int f = F_ACTIVE;
            if (varies) f |= F_VARIES;
            if (opt_se2 && !(opt_adaptive && varies)) f |= F_SE2;
            if (opt_se2 && opt_adaptive && varies && has_unc) f |= F_DOUBLED;
            if ((options & HEAL_POSE_DROP_HARD_BOXES) && varies) f &= ~F_ACTIVE;
            const double* srow = table + (size_t)(b0 + s_edge_box[e0]) * PG_ROW;
            s_xl[3 * l + 0] = srow[T_WX]; s_xl[3 * l + 1] = srow[T_WY];
            s_xl[3 * l + 2] = (f & F_SE2) ? pg_wrap(srow[T_WYAW]) : 0.0;
            int mask = 0, cnt = 0;
            for (int p = e0; p < e1; ++p) {
                const double* row = table + (size_t)(b0 + s_edge_box[p]) * PG_ROW;
                const double sc = (f & F_DOUBLED) ? 2.0 : 1.0;
                const double csum = (row[T_W0] * sc + row[T_W1] * sc) + row[T_W2] * sc;
                const bool unsure = has_unc && (options & HEAL_POSE_DROP_UNSURE_EDGE) && csum < PG_UNSURE;
                const bool on = (f & F_ACTIVE) && !unsure;
                s_edge_on[p] = on ? 1 : 0;
                if (on) { mask |= 1 << s_agent_of[s_edge_box[p]]; ++cnt; }
            }
            s_lm_flags[l] = (unsigned char)f;
            s_lm_mask[l] = (unsigned char)mask;
            if (varies) atomicAdd(&s_ints[2], 1);
            if (cnt) { atomicAdd(&s_ints[3], cnt); atomicOr(&s_ints[4], mask); }
        }
        __syncthreads();
        if (options & HEAL_POSE_ABANDON_HARD_CASES)
            if (nl <= 3 || 2 * s_ints[2] >= nl) { status = HEAL_POSE_STATUS_ABANDONED; give_noisy = true; }
    }
    const int n_edges = bad_input || status == HEAL_POSE_STATUS_ABANDONED ? 0 : s_ints[3];
    const int agent_mask = s_ints[4];
    const int nu_dim = 3 * (N - 1);                      // agent unknowns (agent 0 is fixed)
    double* lrow0 = lws + (size_t)(b0 / 2) * PG_LROW;    // this sample's landmark rows: b0 / 2 + nl <= lws_rows (nl <= n / 2)
    const bool run = !give_noisy && n_edges > 0 && (size_t)(b0 / 2) + (size_t)nl <= (size_t)lws_rows;

    // ---- Levenberg-Marquardt ------------------------------------------------------------------------------------------------
    if (run) {
        if (max_iterations > HEAL_POSE_MAX_ITERATIONS) max_iterations = HEAL_POSE_MAX_ITERATIONS;
        status = HEAL_POSE_STATUS_MAX_ITERATIONS;
        double nu = 2.0, last_step = -1.0;
        for (int it = 0; it < max_iterations; ++it) {
            // -- linearise: one thread per landmark --------------------------------------------------------------------------
            for (int q = 0; q < 2; ++q) {
                const int l = q * PG_THREADS + tid;
                double chi_l = 0.0, dmax = 0.0;
                if (l < nl && s_lm_mask[l]) {
                    const int f = s_lm_flags[l], mask = s_lm_mask[l];
                    const int e0 = s_lm_start[l], e1 = s_lm_start[l + 1];
                    double* lr = lrow0 + (size_t)l * PG_LROW;
                    const double xj[3] = {s_xl[3 * l], s_xl[3 * l + 1], s_xl[3 * l + 2]};
                    double hll[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
                    for (int a = 0; a < N; ++a) {
                        if (!((mask >> a) & 1)) continue;
                        const double xi[3] = {s_xa[3 * a], s_xa[3 * a + 1], s_xa[3 * a + 2]};
                        const double ci = cos(xi[2]), si = sin(xi[2]);
                        double A[6] = {0, 0, 0, 0, 0, 0}, ba[3] = {0, 0, 0}, W[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                        for (int p = e0; p < e1; ++p) {
                            const int j = s_edge_box[p];
                            if (!s_edge_on[p] || s_agent_of[j] != a) continue;
                            const PgEdge m = pg_load_edge(table + (size_t)(b0 + j) * PG_ROW, f);
                            double e[3], d0, d1;
                            pg_error(xi, ci, si, xj, m, e, d0, d1);
                            chi_l += pg_chi(e, m);
                            const double w[3] = {m.w0, m.w1, m.w2};
                            // Ji = Z [[-ci, -si, d1], [si, -ci, -d0], [0, 0, -1]],  Jj = Z [[ci, si, 0], [-si, ci, 0], [0, 0, 1]],
                            // Z = [[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]]
                            const double Ji[3][3] = {{m.cz * (-ci) + m.sz * si, m.cz * (-si) + m.sz * (-ci), m.cz * d1 + m.sz * (-d0)},
                                                     {-m.sz * (-ci) + m.cz * si, -m.sz * (-si) + m.cz * (-ci), -m.sz * d1 + m.cz * (-d0)},
                                                     {0.0, 0.0, -1.0}};
                            const double Jj[3][3] = {{m.cz * ci + m.sz * (-si), m.cz * si + m.sz * ci, 0.0},
                                                     {-m.sz * ci + m.cz * (-si), -m.sz * si + m.cz * ci, 0.0},
                                                     {0.0, 0.0, 1.0}};
#pragma unroll
                            for (int r = 0; r < 3; ++r)
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    double hj = 0.0, hi = 0.0, wv = 0.0;
#pragma unroll
                                    for (int k = 0; k < 3; ++k) {
                                        hj += Jj[k][r] * w[k] * Jj[k][c];
                                        hi += Ji[k][r] * w[k] * Ji[k][c];
                                        wv += Ji[k][r] * w[k] * Jj[k][c];
                                    }
                                    if (c >= r) { hll[pg_sym(r, c)] += hj; A[pg_sym(r, c)] += hi; }
                                    W[r * 3 + c] += wv;
                                }
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                double gj = 0.0, gi = 0.0;
#pragma unroll
                                for (int k = 0; k < 3; ++k) { gj += Jj[k][r] * w[k] * e[k]; gi += Ji[k][r] * w[k] * e[k]; }
                                bl[r] -= gj;
                                ba[r] -= gi;
                            }
                        }
                        if (a > 0) {
                            double* blk = lr + a * 18;
#pragma unroll
                            for (int k = 0; k < 6; ++k) blk[k] = A[k];
#pragma unroll
                            for (int k = 0; k < 3; ++k) blk[6 + k] = ba[k];
#pragma unroll
                            for (int k = 0; k < 9; ++k) blk[9 + k] = W[k];
                        }
                    }
                    if (!(f & F_SE2)) { hll[2] = 0.0; hll[4] = 0.0; hll[5] = 0.0; bl[2] = 0.0; }
#pragma unroll
                    for (int k = 0; k < 6; ++k) lr[L_HLL + k] = hll[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) lr[L_BL + k] = bl[k];
                    dmax = fmax(fmax(hll[0], hll[3]), hll[5]);
                }
                s_red[l] = chi_l;
                s_red2[l] = dmax;
            }
            __syncthreads();                             // the landmark rows (global) and the two arrays are written
            // -- the agents' own blocks: entry (a, c) summed over the landmarks in index order ---------------------------------
            if (tid < PG_MAXA * 9) {
                const int a = tid / 9, c = tid % 9;
                double acc = 0.0;
                if (a >= 1 && a < N)
                    for (int l = 0; l < nl; ++l)
                        if ((s_lm_mask[l] >> a) & 1) acc += lrow0[(size_t)l * PG_LROW + a * 18 + c];
                if (c < 6) s_haa[a * 6 + c] = acc; else s_ba[a * 3 + (c - 6)] = acc;
            }
            if (it == 0) {                               // lambda_0 = tau max diag(H): the landmarks' part as a max tree
                __syncthreads();
                for (int s = PG_MAXL / 2; s >= 1; s >>= 1) {
                    if (tid < s) s_red2[tid] = fmax(s_red2[tid], s_red2[tid + s]);
                    __syncthreads();
                }
            }
            double chi_now, unused;
            {
                const double keep = s_red2[0];
                __syncthreads();
                if (tid == 0) s_red2[0] = 0.0;           // the sum tree below adds it to nothing that is read
                __syncthreads();
                pg_reduce2(s_red, s_red2, tid, chi_now, unused);
                if (it == 0) {
                    double dm = keep;
                    for (int a = 1; a < N; ++a) dm = fmax(dm, fmax(fmax(s_haa[a * 6 + 0], s_haa[a * 6 + 3]), s_haa[a * 6 + 5]));
                    lam = PG_TAU * dm;
                    chi_initial = chi_now;
                }
            }
            chi = chi_now;
            if (!pg_finite(chi)) { status = HEAL_POSE_STATUS_NONFINITE; give_noisy = true; break; }
            iterations = it + 1;
            double rho = 0.0, step = 0.0;
            int trials = 0;
            bool polished = false;
            while (true) {                               // <= PG_MAX_TRIALS rounds
                // -- the landmarks' damped blocks: inverse and Minv bl ---------------------------------------------------------
                if (tid == 0) { s_ints[5] = 0; s_stepmax = 0ull; }
                __syncthreads();                         // the reset comes before this round's first failure flag
                for (int q = 0; q < 2; ++q) {
                    const int l = q * PG_THREADS + tid;
                    if (l < nl && s_lm_mask[l]) {
                        double* lr = lrow0 + (size_t)l * PG_LROW;
                        const bool se2 = s_lm_flags[l] & F_SE2;
                        const double m00 = lr[L_HLL + 0] + lam, m01 = lr[L_HLL + 1], m11 = lr[L_HLL + 3] + lam;
                        const double m02 = se2 ? lr[L_HLL + 2] : 0.0, m12 = se2 ? lr[L_HLL + 4] : 0.0;
                        const double m22 = se2 ? lr[L_HLL + 5] + lam : 1.0;
                        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
                        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
                        const double det = (m00 * c00 + m01 * c01) + m02 * c02;
                        const double id = 1.0 / det;
                        double mi[6] = {c00 * id, c01 * id, c02 * id, c11 * id, c12 * id, c22 * id};
                        if (!se2) { mi[2] = 0.0; mi[4] = 0.0; mi[5] = 0.0; }
                        const double b0l = lr[L_BL], b1l = lr[L_BL + 1], b2l = lr[L_BL + 2];
#pragma unroll
                        for (int k = 0; k < 6; ++k) lr[L_MINV + k] = mi[k];
                        lr[L_YL + 0] = (mi[0] * b0l + mi[1] * b1l) + mi[2] * b2l;
                        lr[L_YL + 1] = (mi[1] * b0l + mi[3] * b1l) + mi[4] * b2l;
                        lr[L_YL + 2] = (mi[2] * b0l + mi[4] * b1l) + mi[5] * b2l;
                        if (!(det > 0.0) || !pg_finite(id)) atomicOr(&s_ints[5], 1);
                    }
                }
                __syncthreads();
                // -- Schur complement, entry by entry, landmarks in index order; row nu_dim is the right-hand side -------------
                for (int idx = tid; idx < (nu_dim + 1) * nu_dim; idx += PG_THREADS) {
                    const int i = idx / nu_dim, j = idx % nu_dim;
                    const int b = j / 3 + 1, qd = j % 3;
                    double v = 0.0;
                    if (i == nu_dim) {
                        v = s_ba[b * 3 + qd];
                        for (int l = 0; l < nl; ++l)
                            if ((s_lm_mask[l] >> b) & 1) {
                                const double* lr = lrow0 + (size_t)l * PG_LROW;
                                const double* Wb = lr + b * 18 + 9 + qd * 3;
                                v -= (Wb[0] * lr[L_YL] + Wb[1] * lr[L_YL + 1]) + Wb[2] * lr[L_YL + 2];
                            }
                    } else if (j <= i) {
                        const int a = i / 3 + 1, pd = i % 3;
                        if (a == b) {
                            v = s_haa[a * 6 + pg_sym(pd, qd)] + (pd == qd ? lam : 0.0);
                            if (!((agent_mask >> a) & 1)) v = pd == qd ? 1.0 : 0.0;     // an agent without an active edge: unit block
                        }
                        for (int l = 0; l < nl; ++l) {
                            const int mk = s_lm_mask[l];
                            if (((mk >> a) & 1) && ((mk >> b) & 1)) {
                                const double* lr = lrow0 + (size_t)l * PG_LROW;
                                const double* Wa = lr + a * 18 + 9 + pd * 3;
                                const double* Wb = lr + b * 18 + 9 + qd * 3;
                                const double* mi = lr + L_MINV;
                                const double t0 = (mi[0] * Wb[0] + mi[1] * Wb[1]) + mi[2] * Wb[2];
                                const double t1 = (mi[1] * Wb[0] + mi[3] * Wb[1]) + mi[4] * Wb[2];
                                const double t2 = (mi[2] * Wb[0] + mi[4] * Wb[1]) + mi[5] * Wb[2];
                                v -= (Wa[0] * t0 + Wa[1] * t1) + Wa[2] * t2;
                            }
                        }
                    }
                    s_S[i * PG_NMAX + j] = v;
                }
                __syncthreads();
                bool ok = s_ints[5] == 0;
                // -- Cholesky, the right-hand side carried as row nu_dim (its entries become the forward substitution) ---------
                for (int k = 0; k < nu_dim; ++k) {
                    const double d = s_S[k * PG_NMAX + k];
                    if (!(d > 0.0) || !pg_finite(d)) ok = false;       // uniform: every thread reads the same word
                    const double r = sqrt(ok ? d : 1.0);
                    __syncthreads();                                     // everybody has read the pivot
                    if (tid == 0) s_ldiag[k] = r;
                    if (tid > k && tid <= nu_dim) s_S[tid * PG_NMAX + k] /= r;
                    __syncthreads();
                    for (int idx = tid; idx < (nu_dim + 1) * nu_dim; idx += PG_THREADS) {
                        const int i = idx / nu_dim, j = idx % nu_dim;
                        if (j > k && i >= j) s_S[i * PG_NMAX + j] -= s_S[i * PG_NMAX + k] * s_S[j * PG_NMAX + k];
                    }
                    __syncthreads();
                }
                if (tid < nu_dim) s_yv[tid] = s_S[nu_dim * PG_NMAX + tid];
                __syncthreads();
                // -- back substitution L^T x = y, column by column -------------------------------------------------------------
                for (int k = nu_dim - 1; k >= 0; --k) {
                    const double xk = s_yv[k] / s_ldiag[k];
                    if (tid == 0) s_xv[k] = xk;
                    if (tid < k) s_yv[tid] -= s_S[k * PG_NMAX + tid] * xk;
                    __syncthreads();
                }
                // -- the agents' trial poses -----------------------------------------------------------------------------------
                if (tid < N) {
                    double d[3] = {0.0, 0.0, 0.0};
                    if (tid > 0) { d[0] = s_xv[3 * (tid - 1)]; d[1] = s_xv[3 * (tid - 1) + 1]; d[2] = s_xv[3 * (tid - 1) + 2]; }
                    if (!(pg_finite(d[0]) && pg_finite(d[1]) && pg_finite(d[2]))) atomicOr(&s_ints[5], 1);
                    s_da[3 * tid] = d[0]; s_da[3 * tid + 1] = d[1]; s_da[3 * tid + 2] = d[2];
                    s_xat[3 * tid] = s_xa[3 * tid] + d[0];
                    s_xat[3 * tid + 1] = s_xa[3 * tid + 1] + d[1];
                    s_xat[3 * tid + 2] = tid > 0 ? pg_wrap(s_xa[3 * tid + 2] + d[2]) : s_xa[3 * tid + 2];
                    atomicMax(&s_stepmax, (unsigned long long)__double_as_longlong(fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2]))));
                }
                __syncthreads();
                // -- the landmarks' updates, the predicted decrease and the cost at the trial point ----------------------------
                for (int q = 0; q < 2; ++q) {
                    const int l = q * PG_THREADS + tid;
                    double chi_l = 0.0, pred_l = 0.0;
                    if (l < nl && s_lm_mask[l]) {
                        const int f = s_lm_flags[l], mask = s_lm_mask[l];
                        const double* lr = lrow0 + (size_t)l * PG_LROW;
                        double v[3] = {0.0, 0.0, 0.0};
                        for (int a = 1; a < N; ++a)
                            if ((mask >> a) & 1) {
                                const double* Wa = lr + a * 18 + 9;
#pragma unroll
                                for (int r = 0; r < 3; ++r)
                                    v[r] += (Wa[r] * s_da[3 * a] + Wa[3 + r] * s_da[3 * a + 1]) + Wa[6 + r] * s_da[3 * a + 2];
                            }
                        const double* mi = lr + L_MINV;
                        double dl[3];
                        dl[0] = lr[L_YL + 0] - ((mi[0] * v[0] + mi[1] * v[1]) + mi[2] * v[2]);
                        dl[1] = lr[L_YL + 1] - ((mi[1] * v[0] + mi[3] * v[1]) + mi[4] * v[2]);
                        dl[2] = (f & F_SE2) ? lr[L_YL + 2] - ((mi[2] * v[0] + mi[4] * v[1]) + mi[5] * v[2]) : 0.0;
                        if (!(pg_finite(dl[0]) && pg_finite(dl[1]) && pg_finite(dl[2]))) atomicOr(&s_ints[5], 1);
                        const double xj[3] = {s_xl[3 * l] + dl[0], s_xl[3 * l + 1] + dl[1],
                                              (f & F_SE2) ? pg_wrap(s_xl[3 * l + 2] + dl[2]) : 0.0};
                        s_xlt[3 * l] = xj[0]; s_xlt[3 * l + 1] = xj[1]; s_xlt[3 * l + 2] = xj[2];
                        pred_l = (dl[0] * (lam * dl[0] + lr[L_BL]) + dl[1] * (lam * dl[1] + lr[L_BL + 1])) +
                                 dl[2] * (lam * dl[2] + lr[L_BL + 2]);
                        atomicMax(&s_stepmax,
                                  (unsigned long long)__double_as_longlong(fmax(fmax(fabs(dl[0]), fabs(dl[1])), fabs(dl[2]))));
                        const int e0 = s_lm_start[l], e1 = s_lm_start[l + 1];
                        for (int a = 0; a < N; ++a) {
                            if (!((mask >> a) & 1)) continue;
                            const double xi[3] = {s_xat[3 * a], s_xat[3 * a + 1], s_xat[3 * a + 2]};
                            const double ci = cos(xi[2]), si = sin(xi[2]);
                            for (int p = e0; p < e1; ++p) {
                                const int j = s_edge_box[p];
                                if (!s_edge_on[p] || s_agent_of[j] != a) continue;
                                const PgEdge m = pg_load_edge(table + (size_t)(b0 + j) * PG_ROW, f);
                                double e[3], d0, d1;
                                pg_error(xi, ci, si, xj, m, e, d0, d1);
                                chi_l += pg_chi(e, m);
                            }
                        }
                    }
                    s_red[l] = chi_l;
                    s_red2[l] = pred_l;
                }
                double chi_t, pred;
                pg_reduce2(s_red, s_red2, tid, chi_t, pred);
                for (int a = 1; a < N; ++a)
#pragma unroll
                    for (int r = 0; r < 3; ++r) pred += s_da[3 * a + r] * (lam * s_da[3 * a + r] + s_ba[3 * a + r]);
                ok = ok && s_ints[5] == 0;
                step = __longlong_as_double((long long)s_stepmax);
                __syncthreads();                         // s_ints[5] and s_stepmax are reset at the top of the next round
                ++total_trials;
                bool accept = false;
                if (ok && pred <= PG_POLISH * chi) {     // below the cost's resolution: taken unseen (pose_graph_optim.py)
                    accept = true;
                    polished = true;
                    chi = fmin(chi, chi_t);
                } else {
                    if (ok) rho = (chi - chi_t) / (pred + 1e-3); else rho = -1.0;
                    if (ok && rho > 0.0 && pg_finite(chi_t)) {
                        double alpha = 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0);
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lam *= fmax(1.0 / 3.0, alpha);
                        nu = 2.0;
                        chi = chi_t;
                        accept = true;
                    } else {
                        lam *= nu;
                        nu *= 2.0;
                    }
                }
                if (accept) {
                    if (tid < 3 * N) s_xa[tid] = s_xat[tid];
                    for (int k = tid; k < 3 * nl; k += PG_THREADS)
                        if (s_lm_mask[k / 3]) s_xl[k] = s_xlt[k];
                    __syncthreads();
                }
                ++trials;
                if (polished) break;
                if (!(rho < 0.0 && trials < PG_MAX_TRIALS && pg_finite(lam))) break;
            }
            if (polished) {
                if (step <= PG_STEP_FLOOR || (last_step >= 0.0 && step > 0.5 * last_step)) {
                    status = HEAL_POSE_STATUS_CONVERGED;
                    break;
                }
                last_step = step;
                continue;
            }
            last_step = -1.0;
            if (trials == PG_MAX_TRIALS || rho == 0.0 || !pg_finite(lam)) { status = HEAL_POSE_STATUS_CONVERGED; break; }
        }
    }

    // ---- results -------------------------------------------------------------------------------------------------------------
    __syncthreads();
    if (tid < NB) {
        const double* p = pose + (size_t)(a0 + tid) * 6;
        double* out = refined + (size_t)(a0 + tid) * 3;
        const bool moved = s_xa[3 * tid] != s_x0[3 * tid] || s_xa[3 * tid + 1] != s_x0[3 * tid + 1] ||
                           s_xa[3 * tid + 2] != s_x0[3 * tid + 2];
        if (give_noisy || (!moved && p[4] > -180.0 && p[4] <= 180.0)) {
            out[0] = p[0]; out[1] = p[1]; out[2] = p[4];
        } else {
            out[0] = s_xa[3 * tid]; out[1] = s_xa[3 * tid + 1]; out[2] = s_xa[3 * tid + 2] * PG_RAD;
        }
    }
    if (tid == 0 && stats != nullptr) {
        double* st = stats + (size_t)smp * HEAL_POSE_STATS;
        st[HEAL_POSE_STAT_LANDMARKS] = (double)nl;
        st[HEAL_POSE_STAT_EDGES] = (double)n_edges;
        st[HEAL_POSE_STAT_ITERATIONS] = (double)iterations;
        st[HEAL_POSE_STAT_STATUS] = (double)status;
        st[HEAL_POSE_STAT_CHI2_INITIAL] = chi_initial;
        st[HEAL_POSE_STAT_CHI2_FINAL] = chi;
        st[HEAL_POSE_STAT_LAMBDA] = lam;
        st[HEAL_POSE_STAT_TRIALS] = (double)total_trials;
    }
}

static size_t pg_table_bytes(int total_boxes) { return align_up((size_t)(total_boxes > 0 ? total_boxes : 1) * PG_ROW * sizeof(double)); }
static size_t pg_lws_rows(int total_boxes) { return (size_t)total_boxes / 2 + 1; }

}  // namespace heal

using namespace heal;

extern "C" int heal_pose_graph_supported(int max_agents_per_sample, int max_boxes_per_sample) {
    return max_agents_per_sample >= 1 && max_agents_per_sample <= HEAL_POSE_MAX_AGENTS && max_boxes_per_sample >= 0 &&
                   max_boxes_per_sample <= HEAL_POSE_MAX_BOXES ? 1 : 0;
}

extern "C" size_t heal_pose_graph_workspace(int samples, int total_agents, int total_boxes) {
    if (samples < 1 || samples > 65535 || total_agents < samples || total_agents > samples * HEAL_POSE_MAX_AGENTS) return 0;
    if (total_boxes < 0 || (long long)total_boxes > (long long)samples * HEAL_POSE_MAX_BOXES) return 0;
    return pg_table_bytes(total_boxes) + align_up(pg_lws_rows(total_boxes) * PG_LROW * sizeof(double));
}

extern "C" int heal_pose_graph_align(const double* corners, const int32_t* box_offsets, const int32_t* agent_offsets,
                                     const double* lidar_pose, const double* log_sigma2, int samples, int total_agents,
                                     int total_boxes, int max_agents, int max_boxes, int options, double thres,
                                     double yaw_var_thres, int max_iterations, double* refined, int32_t* cluster_of_box,
                                     double* stats, void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(heal_pose_graph_supported(max_agents, max_boxes),
                 "pose_graph_align: a sample of %d agents and %d boxes is out of range (at most %d agents and %d boxes per sample)",
                 max_agents, max_boxes, HEAL_POSE_MAX_AGENTS, HEAL_POSE_MAX_BOXES);
    const size_t need = heal_pose_graph_workspace(samples, total_agents, total_boxes);
    HEAL_REQUIRE(need != 0, "pose_graph_align: unsupported batch (%d samples, %d agents, %d boxes)", samples, total_agents, total_boxes);
    HEAL_REQUIRE(box_offsets && agent_offsets && lidar_pose && refined && (corners || total_boxes == 0), "pose_graph_align: null argument");
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws & 255) == 0,
                 "pose_graph_align: the workspace must be 256-byte aligned and hold %zu bytes (got %zu)", need, ws_bytes);
    HEAL_REQUIRE((options & ~63) == 0 && thres == thres && yaw_var_thres == yaw_var_thres, "pose_graph_align: bad options");
    if (max_iterations < 0) max_iterations = 0;
    double* table = (double*)ws;
    double* lws = (double*)((char*)ws + pg_table_bytes(total_boxes));
    hipStream_t s = (hipStream_t)stream;
    if (total_boxes > 0) {
        hipLaunchKernelGGL(k_pg_prepare, dim3((unsigned)ceil_div(total_boxes, 256)), dim3(256), 0, s, corners, box_offsets, lidar_pose,
                           log_sigma2, total_agents, total_boxes, (options & HEAL_POSE_NORMALIZE_UNCERTAINTY) ? 1 : 0, table);
        HEAL_LAUNCH_CHECK();
    }
    HEAL_LAUNCH_EV(k_pg_solve, dim3((unsigned)samples), dim3(PG_THREADS), 0, s, (const double*)table, box_offsets, agent_offsets,
                   lidar_pose, log_sigma2 != nullptr ? 1 : 0, total_agents, total_boxes, options, thres, yaw_var_thres, max_iterations,
                   lws, (int)pg_lws_rows(total_boxes), refined, cluster_of_box, stats);
    HEAL_LAUNCH_CHECK();
    return 0;
}
