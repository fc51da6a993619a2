// V2VNet message passing (opencood/models/fuse_modules/fusion_in_one.py:203-318, sub_modules/convgru.py:7-72) on the fp32
// matrix cores.  Per ego i of a scene with N agents, one launch computes the masked aggregation of the messages
//     msg_ij = (W_n * nbr_ij + E_i) * mask_ij,      E_i = W_e * x_i + b    (msg_cnn(cat(nbr_ij, x_i)) split by input half)
//     mean:  agg_i = (sum_j mask_ij (W_n * nbr_ij) + (sum_j mask_ij) E_i) / N
//     max:   agg_i = max_j mask_ij (W_n * nbr_ij + E_i)
// (+ x_i when gru_flag is false), where nbr_ij is agent j warped into ego i's frame.  The ego term E_i is one convolution per
// ego (the caller's stacked 256 -> 768 convolution of x_i); this kernel does the N neighbour convolutions.
//
// Implicit GEMM of heal_conv3x3 (conv3x3.hip, k_conv3x3; the same A-fragment layout, ops.conv3x3_fragments) with the agent
// loop inside the block: an output tile of 64 channels x (TH x 16) pixels runs the K loop of agent j into a per-agent
// accumulator, multiplies it by that agent's mask in the spatial domain (MFMA's D layout puts one pixel and four channels in a
// lane: one mask value per lane and n-tile) and folds it into the running sum / maximum.  The K loop over (agent, chunk) is
// flat, so the register prefetch of the next chunk crosses agent boundaries without a bubble.
//   * Why not the Winograd F(2x2,3x3) kernel: the mask is per PIXEL, so it does not commute with the output transform
//     A^T . A; every agent would need its own output transform through LDS (the Winograd epilogue's four LDS passes, per agent)
//     instead of 16 multiply-adds per lane.
//   * Agent split (nsplit > 1): the sum over j is linear and max is associative, so block (tile, ego, split s) may reduce the
//     agent range [s * aps, (s + 1) * aps) alone and write a partial to ws[s][ego][Cout][HW] (mean: sum_j mask (W_n * nbr),
//     max: the partial maximum with E added); k_v2v_reduce combines the splits in split order (deterministic) and applies the
//     rest.  This fills the chip when one ego's 4 Cout blocks x tiles are fewer than the CUs (the last iteration: ego 0 only).
// Arithmetic: fp32 MFMA (an fmaf chain per output), fp32 mask products and sums in agent order; no reduced precision.
#include "common.h"
#include "../../include/heal_amd.h"

namespace heal {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int VM_KC = 8;                    // input channels per chunk
constexpr int VM_KS = VM_KC / 4;            // MFMA k-steps per chunk
constexpr int VM_WCHUNK = 9 * VM_KS * 4 * 64;
constexpr int VM_MAX_AGENTS = HEAL_V2V_MAX_AGENTS;

template <int TH>
struct VmGeom {
    static constexpr int TW = 16;
    static constexpr int NT = TH / 4;
    static constexpr int PH = TH + 2, PW = TW + 2, PE = PH * PW;
    static constexpr int CS = (PE + 15) / 32 * 32 + 16;     // == 16 (mod 32): conflict-free B reads (conv3x3.hip)
    static constexpr int NP = (VM_KC * PE + 255) / 256;
    static constexpr int NW = (VM_WCHUNK / 4 + 255) / 256;
};

struct VmArgs {
    const float* xs;      // [n_ego, N, Cin, H, W] warped neighbour maps
    const float* mask;    // [n_ego, N, H, W]
    const float* e;       // E_i: ego stride e_stride floats, channel stride H*W
    long long e_stride;
    const float* wfrag;   // W_n in conv3x3 fragment order
    const float* res;     // [n_ego, Cout, H, W] or null
    float* out;           // [n_ego, Cout, H, W] (nsplit == 1) | partials [nsplit, n_ego, Cout, H, W]
    int n_agents, n_ego, cin, nchunks, cout, H, W, tiles_x, nsplit, aps;
};

template <int TH, bool MAX>
__global__ __launch_bounds__(256) void k_v2v_message(VmArgs a) {
    using G = VmGeom<TH>;
    constexpr int NT = G::NT, PW = G::PW, PE = G::PE, CS = G::CS, NP = G::NP, NW = G::NW;
    __shared__ __attribute__((aligned(16))) float sW[VM_WCHUNK];
    __shared__ float sP[VM_KC * CS];

    const Block3 bk = xcd_block();       // x: Cout block, y: tile, z: ego * nsplit + split
    const int mb = bk.x, ego = bk.z / a.nsplit, split = bk.z - ego * a.nsplit;
    const int ty = bk.y / a.tiles_x, tx = bk.y - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * G::TW;
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int lk = l >> 4, ln = l & 15;
    const int H = a.H, W = a.W, Cin = a.cin, nchunks = a.nchunks, Cout = a.cout;
    const size_t HW = (size_t)H * W;
    const int j0 = split * a.aps, j1 = min(j0 + a.aps, a.n_agents);
    const float* __restrict__ xego = a.xs + (size_t)ego * a.n_agents * Cin * HW;
    const float* __restrict__ mego = a.mask + (size_t)ego * a.n_agents * HW;
    const float4* __restrict__ wsrc = reinterpret_cast<const float4*>(a.wfrag + (size_t)mb * nchunks * VM_WCHUNK);

    int p_off[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int ci = e / PE, rem = e - ci * PE, py = rem / PW, px = rem - py * PW;
        const int gy = oy0 - 1 + py, gx = ox0 - 1 + px;
        const bool ok = e < VM_KC * PE && gy >= 0 && gy < H && gx >= 0 && gx < W;
        p_off[j] = ok ? gy * W + gx : -1;
    }
    float pst[NP];
    float4 wst[NW];
    auto load_chunk = [&](int jj, int c) {
        const float* __restrict__ xin = xego + (size_t)jj * Cin * HW;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int ch = c * VM_KC + (threadIdx.x + 256 * j) / PE;
            pst[j] = (p_off[j] >= 0 && ch < Cin) ? xin[(size_t)ch * HW + p_off[j]] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = threadIdx.x + 256 * j;
            wst[j] = i < VM_WCHUNK / 4 ? wsrc[(size_t)c * (VM_WCHUNK / 4) + i] : float4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int e = threadIdx.x + 256 * j, ci = e / PE;
            if (e < VM_KC * PE) sP[ci * CS + (e - ci * PE)] = pst[j];
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < VM_WCHUNK / 4) reinterpret_cast<float4*>(sW)[i] = wst[j];
        }
    };

    // this lane's pixels (one per n-tile; clamped addresses for loads, the store tests the bounds)
    const int ox = ox0 + ln;
    size_t pix[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) pix[nt] = (size_t)min(oy0 + wave * NT + nt, H - 1) * W + min(ox, W - 1);

    constexpr bool is_max = MAX;      // a template flag: as a runtime flag the compiler keeps both folds live (+100 VGPRs)
    const float* __restrict__ eego = a.e + (size_t)ego * a.e_stride;
    // E_i at this lane's outputs: read where it is used (at each agent's end for max, in the epilogue for mean), not held
    // through the K loop (32 | 64 registers)
    auto load_e = [&](float (&ev)[4][NT][4]) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    ev[mt][nt][r] = eego[(size_t)min(mb * 64 + mt * 16 + lk * 4 + r, Cout - 1) * HW + pix[nt]];
    };

    f32x4 acc[4][NT], tot[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float t0 = is_max ? -INFINITY : 0.f;
            tot[mt][nt] = f32x4{t0, t0, t0, t0};
        }
    float msum[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) msum[nt] = 0.f;

    const float* __restrict__ bbase = sP + lk * CS + (wave * NT) * PW + ln;
    load_chunk(j0, 0);           // the host leaves no split empty: j0 < j1
    store_chunk();
    __syncthreads();
    for (int jj = j0; jj < j1; ++jj) {
        float mk[NT];            // this agent's mask at the lane's pixels: in flight under its K loop
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) mk[nt] = mego[(size_t)jj * HW + pix[nt]];
        for (int c = 0; c < nchunks; ++c) {
            // the next chunk in (agent, chunk) order: the register prefetch crosses agent boundaries
            const bool more = c + 1 < nchunks || jj + 1 < j1;
            if (more) load_chunk(c + 1 < nchunks ? jj : jj + 1, c + 1 < nchunks ? c + 1 : 0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
                for (int ks = 0; ks < VM_KS; ++ks) {
                    float av[4], bv[NT];
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) av[mt] = sW[((tap * VM_KS + ks) * 4 + mt) * 64 + l];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = bbase[ks * 4 * CS + (nt + dy) * PW + dx];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
                }
            }
            if (more) {
                __syncthreads();
                store_chunk();
                __syncthreads();
            }
        }
        // agent done: mask in the spatial domain, fold into the sum / maximum, restart the accumulator
        float ev[4][NT][4];
        if (is_max) load_e(ev);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            msum[nt] = msum[nt] + mk[nt];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (is_max) tot[mt][nt][r] = fmaxf(tot[mt][nt][r], mk[nt] * (acc[mt][nt][r] + ev[mt][nt][r]));
                    else tot[mt][nt][r] = tot[mt][nt][r] + mk[nt] * acc[mt][nt][r];
                }
                acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }

    const bool partial = a.nsplit > 1;
    float* __restrict__ yout = a.out + ((size_t)split * a.n_ego * (partial ? 1 : 0) + ego) * Cout * HW;
    const float* __restrict__ rin = (!partial && a.res) ? a.res + (size_t)ego * Cout * HW : nullptr;
    const float n_div = (float)a.n_agents;
    float ev[4][NT][4];
    if (!partial && !is_max) load_e(ev);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int oy = oy0 + wave * NT + nt;
        if (oy >= H || ox >= W) continue;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = mb * 64 + mt * 16 + lk * 4 + r;
                if (co >= Cout) continue;
                float v = tot[mt][nt][r];
                if (!partial) {
                    if (!is_max) v = (v + msum[nt] * ev[mt][nt][r]) / n_div;
                    if (rin) v = rin[(size_t)co * HW + pix[nt]] + v;
                }
                yout[(size_t)co * HW + pix[nt]] = v;
            }
        }
    }
}

// Combines the splits of the agent loop: mean -> (sum_s part[s] + (sum_j mask_j) E) / N, max -> max_s part[s]; then + res.
__global__ __launch_bounds__(256) void k_v2v_reduce(const float* __restrict__ part, const float* __restrict__ mask,
                                                    const float* __restrict__ e, long long e_stride,
                                                    const float* __restrict__ res, int n_agents, int n_ego, int cout,
                                                    long long HW, int mode, int nsplit, float* __restrict__ out) {
    const long long per_ego = (long long)cout * HW, total = per_ego * n_ego;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long ego = i / per_ego, rem = i - ego * per_ego, co = rem / HW, p = rem - co * HW;
        float v = part[i];
        for (int s = 1; s < nsplit; ++s) {
            const float q = part[(long long)s * total + i];
            v = mode == 1 ? fmaxf(v, q) : v + q;
        }
        if (mode != 1) {
            float ms = 0.f;
            for (int j = 0; j < n_agents; ++j) ms = ms + mask[(ego * n_agents + j) * HW + p];
            v = (v + ms * e[ego * e_stride + co * HW + p]) / (float)n_agents;
        }
        if (res) v = res[i] + v;
        out[i] = v;
    }
}

// Zero-state ConvGRU cell (convgru.py:52-72 with h_cur = 0): h = sigmoid(u) * tanh(c), u / c = channels [0, C) / [C, 2C) of
// the gate convolution (+ the same channels of `add`, the x_i part of the stacked convolution, when given).
__global__ __launch_bounds__(256) void k_gru_zero_state(const float* __restrict__ gates, long long g_stride,
                                                        const float* __restrict__ add, long long a_stride, int n, int C,
                                                        long long HW, float* __restrict__ h) {
    const long long per = (long long)C * HW, total = per * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long img = i / per, k = i - img * per;
        float u = gates[img * g_stride + k], c = gates[img * g_stride + per + k];
        if (add) {
            u = u + add[img * a_stride + k];
            c = c + add[img * a_stride + per + k];
        }
        h[i] = (1.f / (1.f + expf(-u))) * tanhf(c);
    }
}

}  // namespace heal

using namespace heal;

extern "C" size_t heal_v2v_message_workspace(int n_ego, int cout, int H, int W, int nsplit) {
    return nsplit > 1 ? (size_t)nsplit * n_ego * cout * H * W * sizeof(float) : 0;
}

extern "C" int heal_v2v_message(const float* xs, const float* mask, const float* e, long long e_stride, const float* w_frag,
                                const float* residual, int n_ego, int n_agents, int cin, int cout, int H, int W, int mode,
                                int nsplit, int tile_h, float* out, void* ws, size_t ws_bytes, void* stream) {
    HEAL_REQUIRE(n_ego >= 1 && n_agents >= 1 && n_agents <= VM_MAX_AGENTS && cin >= 1 && cout >= 1 && H >= 1 && W >= 1,
                 "v2v_message: bad shape (n_ego %d, n_agents %d in [1, %d], cin %d, cout %d, %dx%d)", n_ego, n_agents,
                 VM_MAX_AGENTS, cin, cout, H, W);
    HEAL_REQUIRE(xs && mask && e && w_frag && out, "v2v_message: null pointer");
    HEAL_REQUIRE(((uintptr_t)w_frag & 15) == 0, "v2v_message: weight fragments must be 16-B aligned");
    HEAL_REQUIRE(mode == 0 || mode == 1, "v2v_message: mode must be 0 (mean) or 1 (max)");
    HEAL_REQUIRE(tile_h == 4 || tile_h == 8 || tile_h == 16, "v2v_message: tile_h must be 4, 8 or 16");
    HEAL_REQUIRE(e_stride >= (long long)cout * H * W, "v2v_message: E's ego stride is shorter than Cout * H * W");
    HEAL_REQUIRE(nsplit >= 1 && nsplit <= n_agents, "v2v_message: nsplit must be in [1, n_agents]");
    const int aps = ceil_div(n_agents, nsplit);
    HEAL_REQUIRE((nsplit - 1) * aps < n_agents, "v2v_message: %d splits of %d agents leave an empty split", nsplit, n_agents);
    if (nsplit > 1)
        HEAL_REQUIRE(ws && ws_bytes >= heal_v2v_message_workspace(n_ego, cout, H, W, nsplit) && ((uintptr_t)ws & 15) == 0,
                     "v2v_message: workspace too small or misaligned");
    const int tiles_x = ceil_div(W, 16), tiles_y = ceil_div(H, tile_h), mblocks = ceil_div(cout, 64);
    HEAL_REQUIRE((long long)tiles_x * tiles_y <= 65535 && (long long)n_ego * nsplit <= 65535,
                 "v2v_message: map too large for the launch grid");
    VmArgs a{xs, mask, e, e_stride, w_frag, residual, nsplit > 1 ? (float*)ws : out, n_agents, n_ego, cin,
             ceil_div(cin, VM_KC), cout, H, W, tiles_x, nsplit, aps};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(mblocks, tiles_x * tiles_y, n_ego * nsplit);
    LaunchEvents ev = take_launch_events();
    hipEvent_t ev_mid = nsplit > 1 ? (hipEvent_t) nullptr : ev.stop;
#define HEAL_VM(TH_, MAX_) HEAL_LAUNCH_EV2((k_v2v_message<TH_, MAX_>), grid, dim3(256), 0, s, ev.start, ev_mid, a)
    if (tile_h == 16) { if (mode == 1) HEAL_VM(16, true); else HEAL_VM(16, false); }
    else if (tile_h == 8) { if (mode == 1) HEAL_VM(8, true); else HEAL_VM(8, false); }
    else { if (mode == 1) HEAL_VM(4, true); else HEAL_VM(4, false); }
#undef HEAL_VM
    HEAL_LAUNCH_CHECK();
    if (nsplit > 1) {
        const long long total = (long long)n_ego * cout * H * W;
        const int blocks = (int)std::min<long long>(ceil_div64(total, 256), 8192);
        HEAL_LAUNCH_EV2(k_v2v_reduce, dim3(blocks), dim3(256), 0, s, (hipEvent_t) nullptr, ev.stop, (const float*)ws, mask, e,
                        e_stride, residual, n_agents, n_ego, cout, (long long)H * W, mode, nsplit, out);
        HEAL_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int heal_gru_zero_state(const float* gates, long long gates_stride, const float* add, long long add_stride, int n,
                                   int channels, int H, int W, float* h, void* stream) {
    HEAL_REQUIRE(n >= 1 && channels >= 1 && H >= 1 && W >= 1, "gru_zero_state: bad shape");
    HEAL_REQUIRE(gates && h, "gru_zero_state: null pointer");
    const long long per = (long long)channels * H * W;
    HEAL_REQUIRE(gates_stride >= 2 * per && (!add || add_stride >= 2 * per),
                 "gru_zero_state: image strides must hold 2 * channels * H * W floats");
    const int blocks = (int)std::min<long long>(ceil_div64(per * n, 256), 8192);
    HEAL_LAUNCH_EV(k_gru_zero_state, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gates, gates_stride, add, add_stride, n,
                   channels, (long long)H * W, h);
    HEAL_LAUNCH_CHECK();
    return 0;
}
