// Shared host/device helpers for libheal_amd (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdarg.h>

#define HEAL_WAVE 64

namespace heal {

// thread-local last error text, exposed through heal_last_error()
char* err_buf();
int set_error(const char* fmt, ...);

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Bump allocator over the caller-provided workspace.
struct Arena {
    char* base; size_t cap; size_t off;
    Arena(void* p, size_t n) : base((char*)p), cap(n), off(0) {}
    template <typename T> T* take(size_t count) {
        size_t bytes = align_up(count * sizeof(T));
        T* r = (T*)(base + off);
        off += bytes;
        return r;
    }
    bool ok() const { return off <= cap && (base != nullptr || off == 0); }
};

#define HEAL_HIP(expr)                                                                      \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess)                                                              \
            return heal::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                   __FILE__, __LINE__);                                     \
    } while (0)

#define HEAL_REQUIRE(cond, ...)                       \
    do {                                              \
        if (!(cond)) return heal::set_error(__VA_ARGS__); \
    } while (0)

#define HEAL_LAUNCH_CHECK() HEAL_HIP(hipGetLastError())

// Debug switches that SKIP WORK (HEAL_K4_DBG, HEAL_K5_DBG, HEAL_SP_DBG: timing anatomy only, outputs invalid) are read ONCE per process and
// announced on stderr when set, so that a stray variable cannot corrupt results silently and costs nothing per launch.
int debug_env_once(const char* name);
#define HEAL_DEBUG_ENV(name) ([]() -> int { static const int v__ = heal::debug_env_once(name); return v__; }())

// fill_bytes: the library's ONLY way of initialising device memory (a kernel, prims.hip).  hipMemsetAsync is not used anywhere: captured
// into a HIP graph it becomes a memset NODE, and in round 4 K1's 0xFF table fill came back from such a node with byte 0 of every
// 16 B cleared (workspace dump in profiles/r05_k1_memset_node_dump.txt; DESIGN 5 "memory fault") -- the runtime's fill goes through
// a pattern buffer that is not private to the node.  A kernel node carries its pattern in its own arguments.
// dst and bytes must be multiples of 4; `byte` is replicated.  Returns 0 / sets the error text.
int fill_bytes(void* dst, int byte, size_t bytes, hipStream_t s);
// 4-byte device-to-device copy as a kernel (dst <- *src, or 0 when src is null); same reason
int copy_word(int* dst, const int* src, hipStream_t s);
#define HEAL_FILL(dst, byte, bytes, s)                      \
    do {                                                    \
        if (heal::fill_bytes((dst), (byte), (bytes), (s))) return 1; \
    } while (0)

// Measurement hook (heal_next_launch_events): a thread-local pair of events armed by the caller and consumed by the next launch
// that supports it (HEAL_LAUNCH_EV).  hipExtLaunchKernelGGL stamps the events with the kernel's OWN begin / end, the interval a
// rocprofv3 kernel trace reports; an event pair recorded around a launch also holds the dispatch and marker latencies (3-5 us,
// a quarter of a 13-us kernel).
struct LaunchEvents { hipEvent_t start, stop; };
LaunchEvents take_launch_events();
#define HEAL_LAUNCH_EV(kernel, grid, block, lds, stream, ...)                                                        \
    do {                                                                                                             \
        const heal::LaunchEvents ev__ = heal::take_launch_events();                                                  \
        if (ev__.start && ev__.stop)                                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, ev__.start, ev__.stop, 0, __VA_ARGS__); \
        else                                                                                                         \
            hipLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, __VA_ARGS__);                      \
    } while (0)

// the same with explicit events (either may be null): the first kernel of a two-kernel operator takes `start`, the last `stop`
#define HEAL_LAUNCH_EV2(kernel, grid, block, lds, stream, ev_start, ev_stop, ...)                                    \
    do {                                                                                                             \
        if ((ev_start) || (ev_stop))                                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, ev_start, ev_stop, 0, __VA_ARGS__); \
        else                                                                                                         \
            hipLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, __VA_ARGS__);                      \
    } while (0)

// Per-image OUTPUT region of interest of a launch (heal_conv1x1_roi, heal_grouped_small_conv3x3_roi; include/heal_amd_roi.h): box
// (y0, y1, x0, x1) in output pixels for each image, passed BY VALUE as a kernel argument -- no device memory, so a captured graph
// holds the boxes as constants.  A block whose output tile holds no pixel of its image's box returns before its first load and writes
// nothing; the test runs on block-uniform values in the prologue, before any barrier, so every wave of a block takes the same path.
// (heal_conv1x1_box_roi: the tiles enumerate the box itself, roi_align4 below; a tile behind its last pixel returns in the same place.)
// The kernels take the table as a template choice (`bool ROI`, default false): the plain instantiation -- what the old entry points
// launch -- receives the empty NoRoi instead and compiles to the code it always was (no test, no larger argument block).
constexpr int ROI_MAX_IMAGES = 8;   // == HEAL_WARP_MAX_AGENTS (checked where the header is included)
struct RoiTable {
    int n;
    unsigned perm;   // see roi_spread
    int by_box;      // k_conv1x1: the tiles enumerate the (aligned) boxes, not the images (roi_align4)
    int box[ROI_MAX_IMAGES][4];
};
inline RoiTable no_roi() { RoiTable r; r.n = 0; r.perm = 1; r.by_box = 0; return r; }
struct NoRoi {};
template <bool ROI> struct RoiArg { using type = NoRoi; };
template <> struct RoiArg<true> { using type = RoiTable; };
// Workgroups go to the 8 XCDs round-robin and xcd_block() hands every XCD one CONTIGUOUS range of the logical block order, image index
// slowest: the tiles a ROI skips (whole images' borders) would all fall to a few XCDs, which then idle while the others set the kernel's
// time.  A pointwise ROI launch therefore walks its G (tile, image) pairs in the order L -> L * perm mod G, perm coprime to G and near
// G / phi: every contiguous range of L holds an even sample of all images and all tile positions.  Blocks that share a pair (the Cout
// chunks of a pixel tile) stay together.  perm == 1: identity.  (The 3x3 ROI launch, whose neighbouring tiles share halo pixels, turns
// the image index with the super-group instead: gconv_small.hip.)
inline unsigned roi_spread(unsigned G) {
    if (G < 16 || G >= 65536) return 1;            // (L * perm stays below 2^32)
    auto gcd = [](unsigned a, unsigned b) { while (b) { const unsigned t = a % b; a = b; b = t; } return a; };
    unsigned p = (unsigned)(G * 0.6180339887) | 1u;
    while (p < G && gcd(p, G) != 1) p += 2;
    return p < G ? p : 1;
}
// host side of the two entry points: checks the boxes (inside the Ho x Wo output map; y1 <= y0 or x1 <= x0 is an EMPTY box, the whole image is
// skipped) and fills the table.  Returns nullptr, or the message of the failed check.
inline const char* roi_from_host(const int32_t* roi_host, int n, int Ho, int Wo, RoiTable* out) {
    if (!roi_host) return "null ROI table";
    if (n > ROI_MAX_IMAGES) return "more images than ROI table rows (HEAL_WARP_MAX_AGENTS)";
    out->n = n;
    for (int i = 0; i < ROI_MAX_IMAGES; ++i)
        for (int k = 0; k < 4; ++k) out->box[i][k] = i < n ? roi_host[4 * i + k] : 0;
    for (int i = 0; i < n; ++i) {
        const int* b = out->box[i];
        if (b[0] < 0 || b[1] > Ho || b[2] < 0 || b[3] > Wo || b[1] < 0 || b[0] > Ho || b[3] < 0 || b[2] > Wo)
            return "ROI box outside the output map";
    }
    return nullptr;
}
// The box rule of heal_conv1x1_box_roi (Wo % 4 == 0): a launch's 64-pixel tiles enumerate each image's ALIGNED box -- its rows, its columns
// rounded outward to multiples of 4 (inside the map, since Wo % 4 == 0) -- row by row, so every float4 of the kernel lies in one row of
// the box and stays 16-B aligned.  An empty box becomes all zeros: no pixel, every tile of the image leaves.
inline void roi_align4(RoiTable* r) {
    r->by_box = 1;
    for (int i = 0; i < r->n; ++i) {
        int* b = r->box[i];
        if (b[0] >= b[1] || b[2] >= b[3]) { b[0] = b[1] = b[2] = b[3] = 0; continue; }
        b[2] &= ~3;
        b[3] = (b[3] + 3) & ~3;
    }
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ unsigned long long lanemask_lt() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(v, o, 64);
        if (l >= o) v += t;
    }
    return v;
}


// Workgroup barrier for data exchanged through LDS only.  `__syncthreads()` compiles to `s_waitcnt vmcnt(0) lgkmcnt(0);
// s_barrier` (its workgroup-scope fence covers global memory too), which drains every global load in flight and so exposes
// one L2/HBM round trip per barrier in a software-pipelined loop.  This form waits for the wave's LDS operations only; global
// loads issued before it stay in flight across the barrier (the compiler still waits for them before their first use).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- XCD-aware block index -----------------------------------------------------------------------------
// The dispatcher is observed to place block b (x fastest) on XCD b % 8, each XCD with a private 4 MiB L2.
// Tiled kernels whose neighbouring tiles share input (conv halos, rotated bilinear footprints) remap the
// dispatch id so that every XCD works on one CONTIGUOUS range of logical tiles; the shared lines are then
// fetched into one L2 instead of up to eight.  Bijective for any grid size.  A speed choice only.
struct Block3 { unsigned x, y, z; };
__device__ inline Block3 xcd_block() {
    const unsigned gx = gridDim.x, gy = gridDim.y, nb = gx * gy * gridDim.z;
    unsigned b = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned q = nb >> 3, r = nb & 7u, xcd = b & 7u;
    b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    Block3 o;
    o.x = b % gx;
    b /= gx;
    o.y = b % gy;
    o.z = b / gy;
    return o;
}

}  // namespace heal
