// Fused masked agent-window attention of CoBEVT's swap fusion (opencood/models/fuse_modules/swap_fusion_modules.py:11-152,
// Attention inside SwapFusionBlockMask; fusion_in_one.py:374-430): for every group of L x ws x ws tokens and every head
//     O = softmax(scale * Q K^T + bias[h] + key_mask) V,      Q, K, V [T = 16 L, d]
// where a group is the (l, w1, w2) tokens of one ws x ws tile of every agent (window mode: pixel (x ws + w1, y ws + w2)) or of a
// dilated grid (grid mode: pixel (w1 H / ws + x, w2 W / ws + y)), in the reference's agent-major token order (l w1 w2).  Keys of
// agents >= n_valid are masked to -inf by the reference (Regroup's padding); queries are not masked.
//
// The transposed MFMA scheme and its blocks are in attn_tiles.h: S^T = K Q^T with K of the group in LDS and Q from global, the
// scores of one query in one lane column, the unnormalised probabilities used as they lie as the B operand of O^T = V^T P^T.
// With ws = 4 a 16-key MFMA tile is exactly one agent's 16 keys: a masked agent is a whole key tile that is neither loaded nor
// multiplied, which is exactly the -inf semantics (exp(-inf) = 0) -- and leaves whatever its K / V hold out of the result.
// One block per (group, head) with one wave per agent: wave l owns the 16 queries of agent l.
#include "attn_tiles.h"
#include "../../include/heal_amd.h"

namespace heal {

constexpr int SWAP_WS = 4;           // window size: 16 tokens per agent and group (AgentGroupTokens)
constexpr int SWAP_MAX_AGENTS = HEAL_AGENT_WINDOW_MAX_AGENTS;

template <int L, int D>
__global__ __launch_bounds__(64 * L) void k_agent_window_attn(
    const float* __restrict__ qkv /*[L,H,W,3,m,D]*/, const float* __restrict__ bias /*[m,T,T] or null*/, int n_valid, int H,
    int W, int m, int grid_mode, float scale, float* __restrict__ out /*[L,H,W,m*D]*/) {
    constexpr int WS = SWAP_WS, T = 16 * L, NB = D / 16;
    constexpr int STR = D + 4;                           // row stride (words) of the LDS tiles (attn_tiles.h)
    __shared__ __attribute__((aligned(16))) float sK[T * STR];
    __shared__ __attribute__((aligned(16))) float sV[T * STR];
    const int ngy = W / WS;
    const int gx = blockIdx.x / ngy, gy = blockIdx.x - gx * ngy, h = blockIdx.y;
    const AgentGroupTokens tok{gx, gy, grid_mode, H, W};
    const int MD = m * D;
    const size_t C3 = (size_t)3 * MD;
    const float* base = qkv + (size_t)h * D;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lk = lane >> 4, ln = lane & 15;
    // Q of this wave's agent, requested together with K / V
    float4 qf[NB];
    const size_t qpix = tok(wave * 16 + ln);
    load_frag<D>(base + qpix * C3, lk, qf);
    // K and V of the valid agents only (the masked key tiles are never read)
    stage_rows<D, 64 * L>(tok, n_valid * 16, base + MD, C3, base + 2 * MD, C3, sK, sV);
    __syncthreads();
    f32x4 s[L];
    float mx, inv;
    query_scores<L, D>(sK, qf, bias ? bias + ((size_t)h * T + wave * 16 + ln) * T + lk * 4 : nullptr, scale, n_valid, lk, ln, s, mx, inv);
    // ---- O^T = V^T P^T over the valid key tiles: B = the (unnormalised) probabilities as they lie ------------------------------------
    f32x4 o[NB];
    zero_tiles(o);
#pragma unroll
    for (int cb = 0; cb < L; ++cb)
        if (cb < n_valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r) col_accumulate<D>(sV, cb, r, lk, ln, s[cb][r], o);
        }
    store_tiles(out + qpix * MD + (size_t)h * D + lk * 4, o, inv);
}

// out[p, c] = (1 / L) sum_l x[l, p, c]: the agent mean of CoBEVT's mlp_head (Reduce('b m d h w -> b d h w', 'mean'), padded agents
// included), summed in agent order.  One float4 per thread.
__global__ void k_agent_mean(const float4* __restrict__ x, int n_agents, size_t n4, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 a = x[i];
    for (int l = 1; l < n_agents; ++l) {
        const float4 v = x[(size_t)l * n4 + i];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    const float s = 1.f / (float)n_agents;
    out[i] = make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

}  // namespace heal

using namespace heal;

extern "C" int heal_agent_window_attention(const float* qkv, const float* bias, int n_agents, int n_valid, int H, int W,
                                           int heads, int dim_head, int window, int mode, float scale, float* out, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && n_agents <= SWAP_MAX_AGENTS, "agent_window_attention: n_agents %d outside 1..%d", n_agents,
                 SWAP_MAX_AGENTS);
    HEAL_REQUIRE(n_valid >= 1 && n_valid <= n_agents, "agent_window_attention: n_valid %d outside 1..%d", n_valid, n_agents);
    HEAL_REQUIRE(window == SWAP_WS, "agent_window_attention: window %d is not instantiated (4 only)", window);
    HEAL_REQUIRE(mode == 0 || mode == 1, "agent_window_attention: mode must be 0 (window) or 1 (grid)");
    HEAL_REQUIRE(heads >= 1 && heads <= 65535 && H >= window && W >= window, "agent_window_attention: bad shape");
    HEAL_REQUIRE(H % window == 0 && W % window == 0, "agent_window_attention: H, W must be multiples of the window size");
    HEAL_REQUIRE(qkv && out, "agent_window_attention: null pointer");
    HEAL_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)bias & 15) == 0,
                 "agent_window_attention: pointers must be 16-B aligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((H / window) * (W / window), heads);
#define HEAL_AWA(L_, D_)                                                                                                  \
    if (n_agents == L_ && dim_head == D_) {                                                                               \
        k_agent_window_attn<L_, D_><<<grid, 64 * L_, 0, s>>>(qkv, bias, n_valid, H, W, heads, mode, scale, out);          \
        HEAL_LAUNCH_CHECK();                                                                                              \
        return 0;                                                                                                         \
    }
    HEAL_AWA(1, 32) HEAL_AWA(2, 32) HEAL_AWA(3, 32) HEAL_AWA(4, 32) HEAL_AWA(5, 32) HEAL_AWA(6, 32) HEAL_AWA(7, 32) HEAL_AWA(8, 32)
#undef HEAL_AWA
    return set_error("agent_window_attention: dim_head %d is not instantiated (32 only)", dim_head);
}

extern "C" int heal_agent_mean(const float* x, int n_agents, long long n_elems, float* out, void* stream) {
    HEAL_REQUIRE(n_agents >= 1 && n_elems >= 0 && n_elems % 4 == 0, "agent_mean: bad shape");
    HEAL_REQUIRE(x && out && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "agent_mean: null or misaligned pointer");
    if (n_elems == 0) return 0;
    const size_t n4 = (size_t)n_elems / 4;
    k_agent_mean<<<(unsigned)((n4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const float4*>(x), n_agents, n4,
                                                                              reinterpret_cast<float4*>(out));
    HEAL_LAUNCH_CHECK();
    return 0;
}
