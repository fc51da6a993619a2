// CP -- the anchor-free centre head: CenterPointLoss (target assignment + Gaussian focal term + L1 term, forward and gradients)
// and generate_predicted_boxes.  Arithmetic, reference line numbers and the reduction order: include/heal_amd_center.h.
//
// The reference criterion copies the boxes to the host and runs ~30 tiny tensor operations per object, builds a numpy Gaussian per
// object and copies it back, then composes the two terms from a dozen full-map operators.  Here:
//   k_cp_targets   one block per sample: n_b, the per-object fp32 chain (heat-map cell, radius, anno_box), the object table and the
//                  count of distinct positive cells (an O(n^2) comparison in LDS) into the workspace
//   k_cp_pixels    lanes along the pixels of the NCHW maps as in det_loss.hip: a wave owns 64 consecutive pixels of one sample, the
//                  block's four waves share the sample's object table in LDS.  A lane walks the table behind a tile-level
//                  bounding-box cull, takes the maximum of the Gaussians that cover its pixel (never stored unless asked for) and,
//                  where an object's centre IS its pixel, adds that slot's L1 term and gradient -- in slot order, so pixels shared
//                  by several slots need neither a scatter nor an atomic.  Writes grad_cls, grad_bbox and two fp64 partials.
//   k_cp_finish    one block: the two normalisers and the fixed-order fp64 sums of the partials
//   k_cp_boxes     bbox_preds [B, 8, H, W] -> reg_preds [B, H*W, 7], the rows of a 64-pixel tile turned in LDS so that both sides
//                  are contiguous accesses
#include "common.h"
#include "../../include/heal_amd_center.h"

namespace heal {

constexpr int CP_TILE = 64;
constexpr int CP_WAVES = 4;
constexpr int CP_MAX_OBJS = HEAL_CENTER_MAX_OBJS;

struct CpGeom {
    float r0, r1, r2, vx, vy, vz, factor;
    float one_minus, one_plus, b3c, c3c, a3x4, a3x2;   // (1 - o), (1 + o), -2 o, (o - 1), 16 o, 8 o: python floats rounded to fp32
    int min_radius, H, W;
};

struct CpTerms {
    float cw[8];            // code_weights as the fp32 tensor of :326
    float cls_weight, loc_weight;
    float clamp_lo, clamp_hi, avg_eps;
};

// sum over the block's 256 threads; every thread must call it
__device__ __forceinline__ int cp_block_sum(int v, int* s4) {
    v = wave_sum_i(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// center_point_loss.py:526-555 on fp32 tensors: the python floats meet the tensors as fp32 scalars
__device__ __forceinline__ float cp_gaussian_radius(float height, float width, const CpGeom& g) {
    const float b1 = height + width;
    const float c1 = ((width * height) * g.one_minus) / g.one_plus;
    const float sq1 = sqrtf(b1 * b1 - 4.0f * c1);
    const float r1 = (b1 + sq1) / 2.0f;
    const float b2 = 2.0f * (height + width);
    const float c2 = (g.one_minus * width) * height;
    const float sq2 = sqrtf(b2 * b2 - 16.0f * c2);
    const float r2 = (b2 + sq2) / 8.0f;
    const float b3 = g.b3c * (height + width);
    const float c3 = (g.c3c * width) * height;
    const float sq3 = sqrtf(b3 * b3 - g.a3x4 * c3);
    const float r3 = (b3 + sq3) / g.a3x2;
    return fminf(fminf(r1, r2), r3);
}

// counts [3][B]: distinct positive cells, kept slots, slots in use (min(n_b, max_objs)) of every sample
__global__ __launch_bounds__(256) void k_cp_targets(const float* __restrict__ boxes, const int* __restrict__ mask, int Mmax,
                                                    int max_objs, CpGeom g, int* __restrict__ counts, int4* __restrict__ table,
                                                    float* __restrict__ anno_ws, float* __restrict__ anno_out,
                                                    long long* __restrict__ inds_out, unsigned char* __restrict__ masks_out) {
    __shared__ int s_ind[CP_MAX_OBJS];
    __shared__ int s4[4];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
    int c = 0;
    for (int i = tid; i < Mmax; i += 256) c += mask[(size_t)b * Mmax + i];
    const int n_b = cp_block_sum(c, s4);
    const int n_used = max(min(min(n_b, max_objs), Mmax), 0);
    for (int k = tid; k < max_objs; k += 256) {
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int x = 0, y = 0, radius = 0, kept = 0;
        if (k < n_used) {
            const float* __restrict__ v = boxes + ((size_t)b * Mmax + k) * 7;
            const float coor_x = ((v[0] - g.r0) / g.vx) / g.factor;
            const float coor_y = ((v[1] - g.r1) / g.vy) / g.factor;
            const float coor_z = ((v[2] - g.r2) / g.vz) / g.factor;
            const float h = (v[3] / g.vx) / g.factor, w = (v[4] / g.vy) / g.factor, l = (v[5] / g.vz) / g.factor;
            // a centre beyond +-2^30 cells (or NaN) is outside any map; the cast below must not see it
            if (h > 0.f && w > 0.f && fabsf(coor_x) < 1073741824.f && fabsf(coor_y) < 1073741824.f) {
                const float rf = cp_gaussian_radius(h, w, g);
                const int ri = rf < 536870912.f ? (int)rf : 536870912;                   // int(): toward zero (2 r + 1 stays an int)
                const int cx = (int)coor_x, cy = (int)coor_y;                             // .to(torch.int32): toward zero
                if (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) {
                    kept = 1;
                    x = cx;
                    y = cy;
                    radius = max(g.min_radius, ri);
                    a[0] = coor_x - (float)cx;
                    a[1] = coor_y - (float)cy;
                    a[2] = coor_z;
                    a[3] = h;
                    a[4] = w;
                    a[5] = l;
                    a[6] = (float)sin((double)v[6]);
                    a[7] = (float)cos((double)v[6]);
                }
            }
        }
        s_ind[k] = kept ? y * g.W + x : -1;
        const size_t slot = (size_t)b * max_objs + k;
        table[slot] = make_int4(x, y, radius, kept);
#pragma unroll
        for (int i = 0; i < 8; ++i) anno_ws[slot * 8 + i] = a[i];
        if (anno_out != nullptr) {
#pragma unroll
            for (int i = 0; i < 8; ++i) anno_out[slot * 8 + i] = a[i];
        }
        if (inds_out != nullptr) inds_out[slot] = kept ? (long long)y * g.W + x : 0ll;
        if (masks_out != nullptr) masks_out[slot] = (unsigned char)kept;
    }
    __syncthreads();
    int cells = 0, kept_slots = 0;
    for (int k = tid; k < n_used; k += 256) {
        const int mine = s_ind[k];
        if (mine < 0) continue;
        ++kept_slots;
        bool first = true;
        for (int j = 0; j < k; ++j) first = first && s_ind[j] != mine;
        cells += first ? 1 : 0;
    }
    cells = cp_block_sum(cells, s4);
    kept_slots = cp_block_sum(kept_slots, s4);
    if (tid == 0) {
        counts[b] = cells;
        counts[B + b] = kept_slots;
        counts[2 * B + b] = n_used;
    }
}

__device__ __forceinline__ double cp_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (ceil(tiles / CP_WAVES), B); partials [2][B * tiles] (cls, reg), not yet normalised
__global__ __launch_bounds__(256) void k_cp_pixels(const float* __restrict__ cls, const float* __restrict__ bbox,
                                                   const int* __restrict__ counts, const int4* __restrict__ table,
                                                   const float* __restrict__ anno, int HW, int W, int tiles, int max_objs,
                                                   CpTerms prm, float* __restrict__ gcls, float* __restrict__ gbbox,
                                                   float* __restrict__ heatmap, double* __restrict__ partials) {
    __shared__ int4 s_obj[CP_MAX_OBJS];
    const int b = blockIdx.y, B = gridDim.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_used = min(counts[2 * B + b], max_objs);
    for (int i = threadIdx.x; i < n_used; i += 256) s_obj[i] = table[(size_t)b * max_objs + i];
    int n_pos = 0, n_kept = 0;                            // the two normalisers: integer sums over the batch, exact in any order
    for (int i = lane; i < B; i += 64) {
        n_pos += counts[i];
        n_kept += counts[B + i];
    }
    n_pos = wave_sum_i(n_pos);
    n_kept = wave_sum_i(n_kept);
    __syncthreads();
    const int tile = blockIdx.x * CP_WAVES + wave;
    if (tile >= tiles) return;                            // wave-uniform; nothing is shared after the barrier
    const int pix = tile * CP_TILE + lane;
    const bool live = pix < HW;                           // the tail of a sample is masked, never read or written
    const int px = pix % W, py = pix / W;
    // the cells of this tile: rows y0..y1, and within a single row the columns x0..x1
    const int first = tile * CP_TILE, last = min(first + CP_TILE, HW) - 1;
    const int y0 = first / W, y1 = last / W;
    const int x0 = y0 == y1 ? first % W : 0, x1 = y0 == y1 ? last % W : W - 1;
    const float s_cls = prm.cls_weight / (float)max(n_pos, 1);                 // :281-283 backwards: weight, then / avg_factor
    const float s_reg = prm.loc_weight / ((float)n_kept + prm.avg_eps);        // :329-331
    const size_t map0 = (size_t)b * HW + (size_t)pix;
    float heat = 0.f;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    double reg_sum = 0.0;
    for (int k = 0; k < n_used; ++k) {
        const int4 o = s_obj[k];                          // one LDS broadcast
        const int r = o.z;
        if (o.w == 0 || o.y + r < y0 || o.y - r > y1 || o.x + r < x0 || o.x - r > x1) continue;   // wave-uniform
        const int dx = px - o.x, dy = py - o.y;
        if (!live || abs(dx) > r || abs(dy) > r) continue;
        const double sigma = (double)(2 * r + 1) / 6.0;
        const double d2 = (double)dx * dx + (double)dy * dy;
        heat = fmaxf(heat, (float)exp(-d2 / (2.0 * sigma * sigma)));
        if (dx == 0 && dy == 0) {                         // slot k's own pixel: its L1 term, in slot order
            const float* __restrict__ a = anno + ((size_t)b * max_objs + k) * 8;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float d = bbox[((size_t)b * 8 + c) * HW + (size_t)pix] - a[c];
                reg_sum += (double)(fabsf(d) * prm.cw[c]);
                const float sign = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f);
                g[c] = g[c] + sign * (s_reg * prm.cw[c]);
            }
        }
    }
    double cls_sum = 0.0;
    if (live) {
        const float x = cls[map0];
        const float ps = (float)(1.0 / (1.0 + exp(-(double)x)));               // sigmoid, rounded once to fp32
        const float p = fminf(fmaxf(ps, prm.clamp_lo), prm.clamp_hi);
        const bool clamped = ps < prm.clamp_lo || ps > prm.clamp_hi;
        const float q = 1.0f - p;                                               // the fp32 number the reference goes on with
        const double pd = (double)p, qd = (double)q;
        double dldp;
        if (heat == 1.0f) {
            const double lp = log(pd);
            cls_sum = -lp * (qd * qd);
            dldp = 2.0 * qd * lp - (qd * qd) / pd;
        } else {
            const double m = (double)(1.0f - heat), nw = (m * m) * (m * m), lq = log(qd);
            cls_sum = -lq * (pd * pd) * nw;
            dldp = ((pd * pd) / qd - 2.0 * pd * lq) * nw;
        }
        if (gcls != nullptr) gcls[map0] = clamped ? 0.f : (float)(dldp * (pd * qd) * (double)s_cls);
        if (gbbox != nullptr) {
#pragma unroll
            for (int c = 0; c < 8; ++c) gbbox[((size_t)b * 8 + c) * HW + (size_t)pix] = g[c];
        }
        if (heatmap != nullptr) heatmap[map0] = heat;
    }
    cls_sum = cp_wave_sum_d(cls_sum);
    reg_sum = cp_wave_sum_d(reg_sum);
    if (lane == 0) {
        const size_t total = (size_t)B * tiles, at = (size_t)b * tiles + tile;
        partials[at] = cls_sum;
        partials[total + at] = reg_sum;
    }
}

// terms[t] <- scale_t * sum_i partials[t][i]: thread j adds partials j, j + 256, ... in fp64, then a fixed LDS tree
__global__ __launch_bounds__(256) void k_cp_finish(const double* __restrict__ partials, long long n_partials,
                                                   const int* __restrict__ counts, int B, CpTerms prm, float* __restrict__ terms) {
    __shared__ double acc[256];
    __shared__ int s4[4];
    int n_pos = 0, n_kept = 0;
    for (int i = threadIdx.x; i < B; i += 256) {
        n_pos += counts[i];
        n_kept += counts[B + i];
    }
    n_pos = cp_block_sum(n_pos, s4);
    n_kept = cp_block_sum(n_kept, s4);
    const double scale[2] = {(double)prm.cls_weight / (double)(float)max(n_pos, 1),
                             (double)prm.loc_weight / (double)((float)n_kept + prm.avg_eps)};
    for (int t = 0; t < 2; ++t) {
        double v = 0.0;
        for (long long i = threadIdx.x; i < n_partials; i += 256) v += partials[(size_t)t * n_partials + i];
        acc[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) terms[t] = (float)(acc[0] * scale[t]);
        __syncthreads();
    }
}

struct CpBoxGeom { float r0, r1, r2, vx, vy, vz, factor; };

// grid (ceil(H * W / 256), B): a wave turns its 64 rows of 7 in LDS
__global__ __launch_bounds__(256) void k_cp_boxes(const float* __restrict__ bbox, int HW, int W, CpBoxGeom g,
                                                  float* __restrict__ out) {
    __shared__ float s_rows[CP_WAVES][CP_TILE * 7];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = ((int)blockIdx.x * CP_WAVES + wave) * CP_TILE, pix = first + lane;
    if (pix < HW) {
        float c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = bbox[((size_t)b * 8 + i) * HW + (size_t)pix];
        float* row = &s_rows[wave][lane * 7];
        row[0] = (((float)(pix % W) + c[0]) * g.factor) * g.vx + g.r0;
        row[1] = (((float)(pix / W) + c[1]) * g.factor) * g.vy + g.r1;
        row[2] = (c[2] * g.factor) * g.vz + g.r2;
        row[3] = (c[3] * g.factor) * g.vx;
        row[4] = (c[4] * g.factor) * g.vy;
        row[5] = (c[5] * g.factor) * g.vz;
        row[6] = atan2f(c[6], c[7]);
    }
    __syncthreads();
    const int n = min(CP_TILE, HW - first) * 7;             // <= 0 for a wave beyond the map
    float* __restrict__ dst = out + ((size_t)b * HW + (size_t)first) * 7;
    for (int i = lane; i < n; i += 64) dst[i] = s_rows[wave][i];
}

static bool cp_shape_ok(int B, int H, int W, int max_objs, long long* tiles) {
    if (B < 1 || B > HEAL_CENTER_MAX_BATCH || H < 1 || W < 1 || max_objs < 1 || max_objs > CP_MAX_OBJS) return false;
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL - CP_TILE) return false;
    const long long t = (hw + CP_TILE - 1) / CP_TILE;
    if ((long long)B * t > 0x7fffffffLL - CP_WAVES) return false;
    *tiles = t;
    return true;
}

}  // namespace heal

using namespace heal;

extern "C" int heal_center_loss_supported(int B, int Mmax, int H, int W, const double* cav_lidar_range, const double* voxel_size,
                                          int out_size_factor, int max_objs) {
    long long tiles;
    if (cav_lidar_range == nullptr || voxel_size == nullptr || Mmax < 1 || out_size_factor < 1) return 0;
    if (!cp_shape_ok(B, H, W, max_objs, &tiles)) return 0;
    long long grid[2];
    for (int i = 0; i < 2; ++i) {
        if (!(voxel_size[i] > 0.0)) return 0;
        const double cells = nearbyint((cav_lidar_range[3 + i] - cav_lidar_range[i]) / voxel_size[i]);   // np.round: half to even
        if (!(cells >= 1.0 && cells < 2147483648.0)) return 0;
        grid[i] = (long long)cells;
    }
    if (!(voxel_size[2] > 0.0)) return 0;
    return (grid[0] / out_size_factor == W && grid[1] / out_size_factor == H) ? 1 : 0;
}

extern "C" size_t heal_center_loss_workspace(int B, int H, int W, int max_objs) {
    long long tiles;
    if (!cp_shape_ok(B, H, W, max_objs, &tiles)) return 0;
    const size_t slots = (size_t)B * max_objs;
    return align_up((size_t)3 * B * sizeof(int)) + align_up(slots * sizeof(int4)) + align_up(slots * 8 * sizeof(float)) +
           align_up((size_t)2 * B * tiles * sizeof(double));
}

extern "C" int heal_center_loss(const float* cls_preds, const float* bbox_preds, const float* object_bbx_center,
                                const int32_t* object_bbx_mask, int B, int Mmax, int H, int W, const double* cav_lidar_range,
                                const double* voxel_size, int out_size_factor, int max_objs, int min_radius,
                                double gaussian_overlap, const double* code_weights, double cls_weight, double loc_weight,
                                float* terms, float* grad_cls, float* grad_bbox, float* heatmap, float* anno_boxes, int64_t* inds,
                                uint8_t* masks, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    HEAL_REQUIRE(cls_preds && bbox_preds && object_bbx_center && object_bbx_mask && cav_lidar_range && voxel_size && code_weights &&
                 terms, "center_loss: the maps, the boxes, the mask, the host arrays and terms must be set");
    HEAL_REQUIRE(heal_center_loss_supported(B, Mmax, H, W, cav_lidar_range, voxel_size, out_size_factor, max_objs),
                 "center_loss: B=%d Mmax=%d H=%d W=%d max_objs=%d (1..%d) out_size_factor=%d is out of range or (H, W) is not the "
                 "feature map of the range and voxel size (heal_center_loss_supported)", B, Mmax, H, W, max_objs, CP_MAX_OBJS,
                 out_size_factor);
    long long tiles_ll = 0;
    cp_shape_ok(B, H, W, max_objs, &tiles_ll);
    const size_t need = heal_center_loss_workspace(B, H, W, max_objs);
    HEAL_REQUIRE(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws & 255) == 0,
                 "center_loss: workspace of %zu bytes, need %zu, 256-B aligned (heal_center_loss_workspace)", ws_bytes, need);
    Arena arena(ws, ws_bytes);
    const size_t slots = (size_t)B * max_objs;
    int* counts = arena.take<int>((size_t)3 * B);
    int4* table = arena.take<int4>(slots);
    float* anno = arena.take<float>(slots * 8);
    double* partials = arena.take<double>((size_t)2 * B * tiles_ll);
    CpGeom g;
    g.r0 = (float)cav_lidar_range[0]; g.r1 = (float)cav_lidar_range[1]; g.r2 = (float)cav_lidar_range[2];
    g.vx = (float)voxel_size[0]; g.vy = (float)voxel_size[1]; g.vz = (float)voxel_size[2];
    g.factor = (float)out_size_factor;
    g.one_minus = (float)(1.0 - gaussian_overlap);
    g.one_plus = (float)(1.0 + gaussian_overlap);
    g.b3c = (float)(-2.0 * gaussian_overlap);
    g.c3c = (float)(gaussian_overlap - 1.0);
    g.a3x4 = (float)(4.0 * (4.0 * gaussian_overlap));
    g.a3x2 = (float)(2.0 * (4.0 * gaussian_overlap));
    g.min_radius = min_radius; g.H = H; g.W = W;
    CpTerms prm;
    for (int i = 0; i < 8; ++i) prm.cw[i] = (float)code_weights[i];
    prm.cls_weight = (float)cls_weight;
    prm.loc_weight = (float)loc_weight;
    prm.clamp_lo = (float)1e-4;
    prm.clamp_hi = (float)(1.0 - 1e-4);
    prm.avg_eps = (float)1e-4;
    const int HW = H * W, tiles = (int)tiles_ll;
    const LaunchEvents ev = take_launch_events();
    HEAL_LAUNCH_EV2(k_cp_targets, dim3(B), dim3(256), 0, s, ev.start, nullptr, object_bbx_center, (const int*)object_bbx_mask, Mmax,
                    max_objs, g, counts, table, anno, anno_boxes, (long long*)inds, (unsigned char*)masks);
    HEAL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cp_pixels, dim3(ceil_div(tiles, CP_WAVES), B), dim3(256), 0, s, cls_preds, bbox_preds, (const int*)counts,
                       (const int4*)table, (const float*)anno, HW, W, tiles, max_objs, prm, grad_cls, grad_bbox, heatmap, partials);
    HEAL_LAUNCH_CHECK();
    HEAL_LAUNCH_EV2(k_cp_finish, dim3(1), dim3(256), 0, s, nullptr, ev.stop, (const double*)partials, (long long)B * tiles,
                    (const int*)counts, B, prm, terms);
    HEAL_LAUNCH_CHECK();
    return 0;
}

extern "C" int heal_center_boxes(const float* bbox_preds, int B, int H, int W, const double* cav_lidar_range,
                                 const double* voxel_size, int out_size_factor, float* reg_preds, void* stream) {
    HEAL_REQUIRE(bbox_preds && reg_preds && cav_lidar_range && voxel_size, "center_boxes: null pointer");
    HEAL_REQUIRE(B >= 1 && B <= HEAL_CENTER_MAX_BATCH && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - 256,
                 "center_boxes: bad shape B=%d (1..%d) H=%d W=%d", B, HEAL_CENTER_MAX_BATCH, H, W);
    CpBoxGeom g;
    g.r0 = (float)cav_lidar_range[0]; g.r1 = (float)cav_lidar_range[1]; g.r2 = (float)cav_lidar_range[2];
    g.vx = (float)voxel_size[0]; g.vy = (float)voxel_size[1]; g.vz = (float)voxel_size[2];
    g.factor = (float)out_size_factor;
    const int HW = H * W;
    HEAL_LAUNCH_EV(k_cp_boxes, dim3(ceil_div(HW, CP_TILE * CP_WAVES), B), dim3(256), 0, (hipStream_t)stream, bbox_preds, HW, W, g,
                   reg_preds);
    HEAL_LAUNCH_CHECK();
    return 0;
}
