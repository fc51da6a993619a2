// CM -- Where2comm's communication mask: Communication.forward for every scene of a batch and the per-level max-pooling of
// Where2comm.forward in one pass over the confidence maps.  Arithmetic and reference line numbers: include/heal_amd_comm.h.
//
// The reference runs, per scene, sigmoid, max over anchors, a 1-channel Conv2d, ones_like / zeros_like / where, a sum, a clone and a
// strided assignment, then one max_pool2d per further level: a dozen launches per scene that each stream a map of a few floats per
// pixel.  Here:
//   k_comm_mask    one block per 32 x 32 tile of one agent.  The tile and its halo of c = sigmoid(max_a psm[a]) are staged in LDS once
//                  (zero outside the map: the convolution's padding); every thread filters four pixels from LDS (lanes along x: the
//                  k x k window of a wave's 32-pixel rows is conflict-free), thresholds, applies the even-agent override and leaves
//                  the level-0 ones in a second LDS tile, from which every further level's cells are reduced directly.  The tile is
//                  aligned to 32 = 4 x 2^(HEAL_WARP_MAX_LEVELS - 1), so a pooling square never straddles two blocks and no level
//                  waits for another.  The tile of a scene's first agent also leaves its count of ones (before the override) in the
//                  workspace.
//   k_comm_rate    one block: count[b] = the tiles' integers in tile order, rate = the fp32 chain of the reference.
#include <stdlib.h>
#include "common.h"
#include "../../include/heal_amd_comm.h"

namespace heal {

constexpr int CM_T = 32;                               // level-0 tile edge
constexpr int CM_THREADS = 256;
constexpr int CM_R = (HEAL_COMM_MAX_K - 1) / 2;        // largest halo
constexpr int CM_PITCH = CM_T + 2 * CM_R;              // 40 floats: rows of the staged tile
static_assert(CM_T % (1 << (HEAL_WARP_MAX_LEVELS - 1)) == 0, "a pooling square must not straddle two tiles");

struct CmParams {
    const float* psm;
    const float* weight;    // [k, k] on the device, or null: no smoothing
    const float* bias;      // [1] on the device
    float* mask[HEAL_WARP_MAX_LEVELS];
    int* tile_count;        // [B, tiles]: ones of the first agent's tile, before the override
    int A, H, W, k, n_levels, tiles_x, tiles;
    float thre;
    uint32_t agent[HEAL_COMM_MAX_AGENTS];   // scene << 16 | index within the scene
};

__global__ __launch_bounds__(CM_THREADS) void k_comm_mask(const CmParams P) {
    __shared__ float s_c[CM_PITCH * CM_PITCH];
    __shared__ float s_w[HEAL_COMM_MAX_K * HEAL_COMM_MAX_K + 1];
    __shared__ unsigned char s_m[CM_T * CM_T];
    __shared__ int s_cnt[CM_THREADS / HEAL_WAVE];
    const int n = blockIdx.y, tile = blockIdx.x;
    const int x0 = (tile % P.tiles_x) * CM_T, y0 = (tile / P.tiles_x) * CM_T;
    const bool smooth = P.weight != nullptr;
    const int k = smooth ? P.k : 1, r = (k - 1) / 2, side = CM_T + 2 * r;
    const int H = P.H, W = P.W;
    const size_t HW = (size_t)H * W;

    if (smooth && (int)threadIdx.x <= k * k) s_w[threadIdx.x] = (int)threadIdx.x < k * k ? P.weight[threadIdx.x] : P.bias[0];
    const float* src = P.psm + (size_t)n * P.A * HW;
    for (int i = threadIdx.x; i < side * side; i += CM_THREADS) {
        const int ly = i / side, lx = i - ly * side;
        const int y = y0 - r + ly, x = x0 - r + lx;
        float c = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t o = (size_t)y * W + x;
            float v = src[o];
            for (int a = 1; a < P.A; ++a) v = fmaxf(v, src[a * HW + o]);
            c = 1.f / (1.f + expf(-v));
        }
        s_c[ly * CM_PITCH + lx] = c;
    }
    __syncthreads();

    const uint32_t who = P.agent[n];
    const int scene = who >> 16, idx = who & 0xffffu;
    const bool forced = (idx & 1) == 0;
    const int tx = threadIdx.x & (CM_T - 1), ty = threadIdx.x / CM_T;     // 8 rows of 32 pixels per pass
    int ones = 0;
#pragma unroll
    for (int p = 0; p < CM_T / (CM_THREADS / CM_T); ++p) {
        const int py = ty + p * (CM_THREADS / CM_T);
        float s;
        if (smooth) {
            s = s_w[k * k];
            for (int dy = 0; dy < k; ++dy)
                for (int dx = 0; dx < k; ++dx) s += s_w[dy * k + dx] * s_c[(py + dy) * CM_PITCH + tx + dx];
        } else {
            s = s_c[py * CM_PITCH + tx];
        }
        const bool in = y0 + py < H && x0 + tx < W;
        const bool m = s > P.thre;
        ones += (in && m) ? 1 : 0;
        const unsigned char mo = (m || forced) ? 1 : 0;
        s_m[py * CM_T + tx] = mo;
        if (in) P.mask[0][(size_t)n * HW + (size_t)(y0 + py) * W + x0 + tx] = mo ? 1.f : 0.f;
    }
    ones = wave_sum_i(ones);
    if (lane_id() == 0) s_cnt[threadIdx.x / HEAL_WAVE] = ones;
    __syncthreads();
    if (idx == 0 && threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < CM_THREADS / HEAL_WAVE; ++i) t += s_cnt[i];
        P.tile_count[(size_t)scene * P.tiles + tile] = t;
    }

    for (int l = 1; l < P.n_levels; ++l) {
        const int Hl = H >> l, Wl = W >> l, e = CM_T >> l, q = 1 << l;      // e x e cells of q x q pixels in this tile
        if (Hl == 0 || Wl == 0) break;
        for (int i = threadIdx.x; i < e * e; i += CM_THREADS) {
            const int cy = i / e, cx = i - cy * e;
            const int gy = (y0 >> l) + cy, gx = (x0 >> l) + cx;
            if (gy >= Hl || gx >= Wl) continue;          // a cell of the last partial row / column: floor mode drops it
            unsigned char v = 0;
            for (int dy = 0; dy < q; ++dy)
                for (int dx = 0; dx < q; ++dx) v |= s_m[(cy * q + dy) * CM_T + cx * q + dx];
            P.mask[l][((size_t)n * Hl + gy) * Wl + gx] = v ? 1.f : 0.f;
        }
    }
}

__global__ __launch_bounds__(CM_THREADS) void k_comm_rate(const int* __restrict__ tile_count, int tiles, int B, float hw,
                                                          int* __restrict__ count, float* __restrict__ rate) {
    for (int b = threadIdx.x; b < B; b += CM_THREADS) {
        int t = 0;
        for (int i = 0; i < tiles; ++i) t += tile_count[(size_t)b * tiles + i];
        count[b] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int b = 0; b < B; ++b) sum += (float)count[b] / hw;
        rate[0] = sum / (float)B;
    }
}

static long long cm_tiles(int H, int W) { return (long long)ceil_div(W, CM_T) * ceil_div(H, CM_T); }

}  // namespace heal

using namespace heal;

extern "C" int heal_comm_fused_enabled(void) {
    const char* v = getenv("HEAL_COMM_FUSED");
    if (v == nullptr || v[0] == 0 || (v[0] == '1' && v[1] == 0)) return 1;
    return (v[0] == '0' && v[1] == 0) ? 0 : -1;
}

extern "C" int heal_comm_mask_supported(int n_total, int B, int A, int H, int W, int k, int n_levels) {
    if (B < 1 || n_total < B || n_total > HEAL_COMM_MAX_AGENTS || A < 1 || H < 1 || W < 1) return 0;
    if ((long long)H * W >= (1ll << 31)) return 0;
    if ((double)n_total * A * (double)H * W >= 4.6e18) return 0;
    if (k < 1 || k > HEAL_COMM_MAX_K || k % 2 == 0) return 0;
    if (n_levels < 1 || n_levels > HEAL_WARP_MAX_LEVELS) return 0;
    return 1;
}

extern "C" size_t heal_comm_mask_workspace(int B, int H, int W) {
    if (B < 1 || B > HEAL_COMM_MAX_AGENTS || H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
    return align_up((size_t)B * (size_t)cm_tiles(H, W) * sizeof(int));
}

extern "C" int heal_comm_mask(const float* psm, int n_total, int A, int H, int W, const int32_t* record_len_host, int B,
                              const float* weight, const float* bias, int k, float thre, int n_levels, float* const* mask_host,
                              int32_t* count, float* rate, void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(weight == nullptr || (k >= 1 && k <= HEAL_COMM_MAX_K && k % 2 == 1),
                 "comm_mask: k must be odd and in [1, %d] (got %d)", HEAL_COMM_MAX_K, k);
    HEAL_REQUIRE(heal_comm_mask_supported(n_total, B, A, H, W, weight ? k : 1, n_levels),
                 "comm_mask: unsupported problem (n_total %d, B %d, A %d, H %d, W %d, k %d, levels %d)", n_total, B, A, H, W, k,
                 n_levels);
    HEAL_REQUIRE(psm && record_len_host && mask_host && count && rate, "comm_mask: null argument");
    HEAL_REQUIRE(weight == nullptr || bias != nullptr, "comm_mask: a filter weight without a bias");
    CmParams Q;              // the agents' scene table travels by value: nothing is copied to the device
    Q.psm = psm; Q.weight = weight; Q.bias = bias;
    Q.A = A; Q.H = H; Q.W = W; Q.k = k; Q.n_levels = n_levels; Q.thre = thre;
    Q.tiles_x = ceil_div(W, CM_T);
    Q.tiles = (int)cm_tiles(H, W);
    int at = 0;
    for (int b = 0; b < B; ++b) {
        HEAL_REQUIRE(record_len_host[b] >= 1 && at + (long long)record_len_host[b] <= n_total,
                     "comm_mask: record_len[%d] = %d does not fit n_total = %d", b, record_len_host[b], n_total);
        for (int i = 0; i < record_len_host[b]; ++i) Q.agent[at++] = ((uint32_t)b << 16) | (uint32_t)i;
    }
    HEAL_REQUIRE(at == n_total, "comm_mask: record_len sums to %d, psm has %d agents", at, n_total);
    for (int a = at; a < HEAL_COMM_MAX_AGENTS; ++a) Q.agent[a] = 0;
    for (int l = 0; l < HEAL_WARP_MAX_LEVELS; ++l) {
        const bool used = l < n_levels && (H >> l) >= 1 && (W >> l) >= 1;
        Q.mask[l] = used ? mask_host[l] : nullptr;
        HEAL_REQUIRE(!used || Q.mask[l], "comm_mask: mask of level %d is NULL", l);
    }
    const size_t need = heal_comm_mask_workspace(B, H, W);
    HEAL_REQUIRE(ws && ws_bytes >= need, "comm_mask: workspace too small (%zu < %zu)", ws_bytes, need);
    Q.tile_count = (int*)ws;
    hipStream_t st = (hipStream_t)stream;
    const LaunchEvents ev = take_launch_events();
    HEAL_LAUNCH_EV2(k_comm_mask, dim3((unsigned)Q.tiles, (unsigned)n_total), dim3(CM_THREADS), 0, st, ev.start, (hipEvent_t) nullptr, Q);
    HEAL_LAUNCH_CHECK();
    HEAL_LAUNCH_EV2(k_comm_rate, dim3(1), dim3(CM_THREADS), 0, st, (hipEvent_t) nullptr, ev.stop, (const int*)Q.tile_count, Q.tiles, B,
                    (float)((long long)H * W), count, rate);
    HEAL_LAUNCH_CHECK();
    return 0;
}
