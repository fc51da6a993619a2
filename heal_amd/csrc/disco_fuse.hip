// DiscoNet fusion: warp every agent into the ego frame, one logit per (agent, pixel) from a four-layer 1x1 MLP over
// cat(warped neighbour, unwarped ego), softmax over agents, weighted sum -- one launch per scene.
//
// Reference arithmetic (one scene of n agents):
//   opencood/models/fuse_modules/fusion_in_one.py:153-201  DiscoFusion.forward
//       nbr_j  = warp_affine_simple(feats, t[0, :n])[j]                       (torch_transformation_utils.py:323-332)
//       l_j    = PixelWeightLayer(cat(nbr_j, x_0))                             [1, H, W] per agent
//       w      = softmax_j(l_j);   out = sum_j w_j nbr_j
//   PixelWeightLayer (DiscoNet / CoAlign lineage): ReLU(bn(conv1x1)) 2C -> 128 -> 32 -> 8, then ReLU(conv1x1 8 -> 1).
// The torch composition writes and re-reads the warped stack [n, C, H, W] and the concatenation [n, 2C, H, W]; here neither exists.
//
// Identities (DiscoNet): inference BatchNorm is folded into the convolution before it by the caller; layer 1 splits by
// input half, conv1_1(cat(nbr_j, x_0)) = W1n nbr_j + E0 with E0 = W1e x_0 + b1 the same for every agent (computed once per scene
// by heal_conv1x1 and passed in); one agent has weight exactly 1.
//
// A block of 4 waves is a tile of 16 x 4 ego pixels.
//   Phase 1, per agent j:
//     1. the bilinearly warped values of 32 channels x 64 pixels go global -> registers -> LDS, pixel-fastest (the B operand of
//        v_mfma_f32_16x16x4_f32); the next chunk's taps and A fragments are in flight while this chunk's MFMAs run;
//     2. layer 1 [128 x C] . [C x 64]: wave w owns rows 32 w .. 32 w + 31 (2 m-tiles x 4 n-tiles of accumulators), A fragments
//        straight from L2 in fragment order (ops.mfma_a_fragments); + E0, ReLU -> LDS;
//     3. layer 2 [32 x 128] . [128 x 64] on the matrix cores: wave w owns the 16 pixels of n-tile w; + b2, ReLU -> LDS;
//     4. layers 3 and 4 (8 x 32 and 1 x 8: 264 FMAs per pixel) by wave 0, lane = pixel, weights through scalar loads; the logit
//        goes to LDS (and to `scores` when given).
//   Phase 2: softmax over the n logits of the thread's pixel (max, exp, sum, divide -- torch's order), then the warped maps are
//     gathered AGAIN (from L2: the same block read the same footprint microseconds earlier) and accumulated with the final
//     weights in agent order, thread = pixel x channel quarter.
// Out-of-range samples are zeros and take part in the softmax, as in the reference.  fp32 throughout; no atomics.
#include "common.h"
#include "warp_taps.h"
#include "../../include/heal_amd.h"

namespace heal {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DF_TW = 16, DF_TH = 4, DF_TP = DF_TW * DF_TH;   // ego pixel tile of a block
constexpr int DF_KC = 32;                                     // channels per staging chunk (8 per wave)
constexpr int DF_LD = DF_TP + 16;                             // LDS row stride: the four k-rows of a B fragment 16 banks apart
constexpr int DF_M1 = 128, DF_M2 = 32, DF_M3 = 8;             // PixelWeightLayer widths

struct DiscoParams {
    const float* feats;     // [n, C, H, W]
    const float* e0;        // [128, H, W]: W1e x_0 + b1
    const float* w1n;       // [8, C / 4, 64]: the neighbour half of the folded conv1_1 in A-fragment order
    const float* w2f;       // [2, 32, 64]: folded conv1_2 in A-fragment order
    const float *b2, *w3, *b3, *w4, *b4;      // [32], [8, 32], [8], [8], [1]
    float* out;             // [C, H, W]
    float* scores;          // [n, H, W] post-ReLU logits, or null
    AffineRows rows;
    int C, H, W;
};

template <int NA>
__global__ __launch_bounds__(256, 2) void k_disco_fuse(const DiscoParams P) {
    __shared__ float s_x[DF_KC][DF_LD];
    __shared__ float s_h1[DF_M1][DF_LD];
    __shared__ float s_h2[DF_M2][DF_LD];
    __shared__ float s_logit[WF_MAXA][DF_TP];
    const Block3 bk = xcd_block();
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6, lk = l >> 4, ln = l & 15;
    const int tx0 = bk.x * DF_TW, ty0 = bk.y * DF_TH;
    const int w = tx0 + ln, h = ty0 + lk;          // gather roles: lane = pixel of the tile, wave = channel slice
    const bool live = w < P.W && h < P.H;          // no early return: the block meets at barriers
    const int C = P.C, HW = P.H * P.W, pix = h * P.W + w;
    const int ksteps = C >> 2, nchunks = (C + DF_KC - 1) / DF_KC;

    if (NA > 1 || P.scores != nullptr) {
#pragma unroll 1
        for (int a = 0; a < NA; ++a) {
            // E0 and the conv1_2 fragments are the same for every agent; hoisted out of this loop (which the compiler does on its
            // own) they hold 96 registers for the whole of phase 1: 340 instead of 201, one wave per SIMD instead of two (measured,
            // 5 agents at 256 x 256: 1185 us hoisted, 1002 us re-read per agent from L1 / L2).  The empty asm (no instruction)
            // makes the pointers opaque per iteration.
            const float* e0p = P.e0;
            const float* w2p = P.w2f;
            asm volatile("" : "+s"(e0p), "+s"(w2p));
            int off[4];
            float wt[4];
            pixel_taps(P.rows, a, h, w, P.H, P.W, live, off, wt);
            // the four waves hold the same 64 pixels: the test is block-uniform, the barriers inside are met by every wave
            const bool any = __ballot((wt[0] != 0.f) | (wt[1] != 0.f) | (wt[2] != 0.f) | (wt[3] != 0.f)) != 0ull;
            f32x4 acc[2][4];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (any) {      // an agent that reaches no pixel of the tile is a zero operand: layer 1 is E0 alone
                const float* __restrict__ src_a = P.feats + (size_t)a * C * HW;
                // Software pipeline: the NEXT chunk's taps (raw words) and A fragments are requested before this chunk's MFMAs and
                // combined / used one iteration later, so no MFMA waits on a load issued in its own iteration (with the A fragments
                // loaded inside the k-step loop, an L2 round trip stood in front of every 8 MFMAs: 392 instead of 306 us for 5
                // agents at 128 x 128).
                float raw[8][4];
                float a_cur[2][DF_KC / 4], a_nxt[2][DF_KC / 4];
                auto load_raw = [&](int c) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float* __restrict__ src = src_a + (size_t)min(c * DF_KC + wave * 8 + u, C - 1) * HW;
#pragma unroll
                        for (int k = 0; k < 4; ++k) raw[u][k] = src[off[k]];
                    }
                };
                auto load_a = [&](int c, float (&af)[2][DF_KC / 4]) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int ks = 0; ks < DF_KC / 4; ++ks) {
                            const int kg = c * (DF_KC / 4) + ks;      // past the last k-step: a zero fragment (the B rows are zero too)
                            af[mt][ks] = kg < ksteps ? P.w1n[((size_t)(wave * 2 + mt) * ksteps + kg) * 64 + l] : 0.f;
                        }
                };
                load_raw(0);
                load_a(0, a_cur);
                for (int c = 0; c < nchunks; ++c) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {      // sample(): nw, ne, sw, se accumulated in that order
                        float v = raw[u][0] * wt[0];
                        v += raw[u][1] * wt[1];
                        v += raw[u][2] * wt[2];
                        v += raw[u][3] * wt[3];
                        s_x[wave * 8 + u][l] = c * DF_KC + wave * 8 + u < C ? v : 0.f;
                    }
                    lds_barrier();
                    if (c + 1 < nchunks) {
                        load_raw(c + 1);
                        load_a(c + 1, a_nxt);
                    }
                    __builtin_amdgcn_sched_barrier(0);      // keep the prefetch ABOVE this chunk's MFMAs
#pragma unroll
                    for (int ks = 0; ks < DF_KC / 4; ++ks) {
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const float b = s_x[ks * 4 + lk][nt * 16 + ln];
                            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[0][ks], b, acc[0][nt], 0, 0, 0);
                            acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[1][ks], b, acc[1][nt], 0, 0, 0);
                        }
                    }
                    lds_barrier();
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int ks = 0; ks < DF_KC / 4; ++ks) a_cur[mt][ks] = a_nxt[mt][ks];
                }
            }
            // folded conv1_2 in fragment order, 8 k-steps at a time: the first batch is requested here, before the epilogue's barrier
            float a2c[2][8], a2n[2][8];
            auto load_a2 = [&](int q, float (&af)[2][8]) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) af[mt][ks] = w2p[(size_t)(mt * (DF_M1 / 4) + q * 8 + ks) * 64 + l];
            };
            load_a2(0, a2c);
            // layer 1 epilogue: D[row = lk * 4 + r][col = ln] per (mt, nt); n-tile nt is row nt of the pixel tile
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const bool in = ty0 + nt < P.H && tx0 + ln < P.W;
                    const int p_g = in ? (ty0 + nt) * P.W + tx0 + ln : 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = wave * 32 + mt * 16 + lk * 4 + r;
                        const float e = in ? e0p[(size_t)row * HW + p_g] : 0.f;
                        s_h1[row][nt * 16 + ln] = fmaxf(acc[mt][nt][r] + e, 0.f);
                    }
                }
            lds_barrier();
            // layer 2: wave = n-tile, both m-tiles, two accumulation chains per tile
            f32x4 c2[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) { c2[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; c2[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int q = 0; q < DF_M1 / 32; ++q) {
                if (q + 1 < DF_M1 / 32) load_a2(q + 1, a2n);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const float b = s_h1[(q * 8 + ks) * 4 + lk][wave * 16 + ln];
                    c2[0][ks & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2c[0][ks], b, c2[0][ks & 1], 0, 0, 0);
                    c2[1][ks & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2c[1][ks], b, c2[1][ks & 1], 0, 0, 0);
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) a2c[mt][ks] = a2n[mt][ks];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mt * 16 + lk * 4 + r;
                    s_h2[row][wave * 16 + ln] = fmaxf((c2[mt][0][r] + c2[mt][1][r]) + P.b2[row], 0.f);
                }
            lds_barrier();
            // layers 3 and 4: wave 0, lane = pixel.  The other waves go on to the next agent; s_h2 is not written again before a
            // barrier that wave 0 joins after these reads.
            if (wave == 0) {
                float logit = P.b4[0];
#pragma unroll
                for (int o = 0; o < DF_M3; ++o) {
                    float s = P.b3[o];
#pragma unroll
                    for (int k = 0; k < DF_M2; ++k) s = fmaf(P.w3[o * DF_M2 + k], s_h2[k][l], s);
                    logit = fmaf(P.w4[o], fmaxf(s, 0.f), logit);
                }
                logit = fmaxf(logit, 0.f);
                s_logit[a][l] = logit;
                if (P.scores != nullptr && live) P.scores[(size_t)a * HW + pix] = logit;
            }
        }
        lds_barrier();
    }

    // ---- phase 2: softmax over agents, weighted sum in agent order ----------------------------------------------------------------
    float prob[NA];
    if (NA == 1) {
        prob[0] = 1.f;      // the softmax of one logit
    } else {
#pragma unroll
        for (int a = 0; a < NA; ++a) prob[a] = s_logit[a][l];
        softmax_agents(prob);
    }
    int off[NA][4];
    float wt[NA][4];
    unsigned reach = 0;      // bit a: some lane of this wave samples agent a inside its map
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        pixel_taps(P.rows, a, h, w, P.H, P.W, live, off[a], wt[a]);
        const bool any = (wt[a][0] != 0.f) | (wt[a][1] != 0.f) | (wt[a][2] != 0.f) | (wt[a][3] != 0.f);
        reach |= __ballot(any) ? (1u << a) : 0u;
    }
    const int cper = (C + 3) / 4;
    const int c_lo = wave * cper, c_hi = min(c_lo + cper, C);
#pragma unroll 2
    for (int c = c_lo; c < c_hi; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < NA; ++a)
            if ((reach >> a) & 1u) acc += prob[a] * tap4(P.feats + ((size_t)a * C + c) * HW, off[a], wt[a]);
        if (live) P.out[(size_t)c * HW + pix] = acc;
    }
}

}  // namespace heal

using namespace heal;

extern "C" int heal_disco_fuse(const float* feats, int n_agents, int channels, int H, int W, const double* affine_host,
                               const double* affine_dev, int grid_f64, const float* e0, const float* w1n_frag,
                               const float* w2_frag, const float* b2, const float* w3, const float* b3, const float* w4,
                               const float* b4, float* out, float* scores, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && n_agents <= WF_MAXA, "disco_fuse: n_agents must be in [1,%d] (got %d)", WF_MAXA, n_agents);
    HEAL_REQUIRE(channels >= 4 && channels % 4 == 0, "disco_fuse: channels must be a positive multiple of 4 (got %d)", channels);
    HEAL_REQUIRE(H >= 1 && W >= 1, "disco_fuse: bad shape");
    HEAL_REQUIRE((long long)n_agents * channels * H * W < (1ll << 31) && (long long)DF_M1 * H * W < (1ll << 31),
                 "disco_fuse: more than 2^31 elements");
    HEAL_REQUIRE(feats && out, "disco_fuse: null feats / out");
    DiscoParams P;
    if (fill_affine_rows(P.rows, "disco_fuse", affine_host, affine_dev, n_agents, grid_f64)) return 1;
    HEAL_REQUIRE((n_agents == 1 && scores == nullptr) || (e0 && w1n_frag && w2_frag && b2 && w3 && b3 && w4 && b4),
                 "disco_fuse: null PixelWeightLayer operand");
    P.feats = feats; P.e0 = e0; P.w1n = w1n_frag; P.w2f = w2_frag; P.b2 = b2; P.w3 = w3; P.b3 = b3; P.w4 = w4; P.b4 = b4;
    P.out = out; P.scores = scores;
    P.C = channels; P.H = H; P.W = W;
    const dim3 grid(ceil_div(W, DF_TW), ceil_div(H, DF_TH));
    hipStream_t st = (hipStream_t)stream;
    HEAL_FOR_AGENTS(n_agents, "disco_fuse", HEAL_LAUNCH_EV(k_disco_fuse<NA>, grid, dim3(256), 0, st, P));
    HEAL_LAUNCH_CHECK();
    return 0;
}
