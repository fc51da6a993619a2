"""Tensor-level wrappers over the C ABI (include/heal_amd.h).

torch is used for device memory and the current HIP stream only; all arithmetic happens in
libheal_amd.so.  Every function requires CUDA(HIP) tensors and raises otherwise -- there is no CPU
path in the product.
"""
import ctypes

import numpy as np
import torch

from . import _capi, derived, switches
from .derived import derived as _derived

_WS = {}

# The kernels' compile-time limits are `#define HEAL_..._MAX_...` in include/heal_amd.h, each next to the entry point it bounds; the
# constants below that route a call to a kernel or to the torch path are read from there (the .hip files use the same defines).
_limit = _capi.header_define
WARP_MAX_AGENTS, WARP_MAX_LEVELS = _limit("HEAL_WARP_MAX_AGENTS"), _limit("HEAL_WARP_MAX_LEVELS")     # heal_warp_fuse[_levels[_src]]

# Optional per-operator timing with HIP events on the launch stream (bench.py turns it on):
# TIMING = {} enables it; every wrapper then appends (start_event, end_event) under its name.
TIMING = None
# SP_TRACE = [] additionally records, per sparse convolution, what its roofline needs: channel counts, taps,
# the (device) input / output row counts and the neighbour table (-> rule pairs R), with the launch's timing events.
SP_TRACE = None
# LAST_CALLS = {} keeps, per MULTI-LAUNCH operator (K1: memset + 5 kernels, K8: memset + 4 kernels), a closure that repeats its last
# call on the same tensors.  An event pair around such a chain launched from the host mostly times the host (6 launches a ~10 us
# apart); bench.py replays the closure inside a captured graph (graph_period_ms) -- how the chain runs in the timed region.
LAST_CALLS = None


def _remember(name, fn):
    if LAST_CALLS is not None:
        LAST_CALLS[name] = fn


def graph_period_ms(fn, reps=20, iters=10):
    """Device time per call of `fn` (launches only, outputs dropped) as a captured graph runs it: `reps` back-to-back calls captured
    once on the current (non-default) stream, replayed `iters` times; median of replay time / reps."""
    global TIMING, LAST_CALLS
    saved = (TIMING, LAST_CALLS)
    TIMING, LAST_CALLS = None, None          # no events inside a capture
    try:
        st = torch.cuda.current_stream()
        for _ in range(3):
            fn()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for _ in range(reps):
                fn()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            g.replay()
            e1.record(st)
            st.synchronize()
            ts.append(e0.elapsed_time(e1) / reps)
        ts.sort()
        return ts[len(ts) // 2]
    finally:
        TIMING, LAST_CALLS = saved


class _Timed:
    """work: optional (flops, algorithmic bytes) of this launch, accumulated per name for the roofline report.
    kernel_events=True (operators that are ONE kernel whose C entry point supports heal_next_launch_events): the events are
    stamped with the kernel's own begin / end (what a rocprofv3 kernel trace reports) instead of being recorded around the launch,
    which adds the dispatch and marker latencies (3-5 us: a quarter of K4's 13 us)."""

    def __init__(self, name, flops=0.0, nbytes=0.0, kernel_events=False):
        self.name = name
        self.flops = float(flops)
        self.nbytes = float(nbytes)
        self.kernel_events = kernel_events

    def __enter__(self):
        if TIMING is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            st = torch.cuda.current_stream()
            self.e0.record(st)
            if self.kernel_events and not torch.cuda.is_current_stream_capturing():
                self.e1.record(st)          # instantiates the underlying hipEvent_t; the launch re-stamps both
                _capi.call("heal_next_launch_events", ctypes.c_void_p(self.e0.cuda_event), ctypes.c_void_p(self.e1.cuda_event))
            else:
                self.kernel_events = False
        return self

    def __exit__(self, *exc):
        if TIMING is not None:
            if not self.kernel_events:
                self.e1.record(torch.cuda.current_stream())
            else:
                _capi.call("heal_next_launch_events", None, None)   # disarm if the launch never happened (an error above)
            TIMING.setdefault(self.name, []).append((self.e0, self.e1, self.flops, self.nbytes))
        return False


def timing_summary():
    """name -> (calls, mean milliseconds); call after torch.cuda.synchronize()."""
    out = {}
    for name, evs in (TIMING or {}).items():
        ms = [e[0].elapsed_time(e[1]) for e in evs]
        out[name] = (len(ms), sum(ms) / max(len(ms), 1))
    return out


def work_summary():
    """name -> dict(calls, total_ms, flops, bytes) summed over the recorded launches (call after a synchronize)."""
    out = {}
    for name, evs in (TIMING or {}).items():
        out[name] = {"calls": len(evs), "total_ms": sum(e[0].elapsed_time(e[1]) for e in evs),
                     "flops": sum(e[2] for e in evs), "bytes": sum(e[3] for e in evs)}
    return out


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.HealAmdError(f"{name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if t.dtype != dtype:
        raise _capi.HealAmdError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if t.grad_fn is not None and torch.is_grad_enabled():
        # an activation of a recorded autograd graph: the HIP operators have no backward, the result would silently drop out
        # of the graph.  The modules route such calls to their gradient path (bev_blocks.grad_path); reaching this is a bug
        # or an operator without one (sparse 3-D encoder, attention fusions).
        raise _capi.HealAmdError(f"{name} carries autograd history: this HIP operator is inference-only (no backward). "
                                 "Run under torch.no_grad(), or train a configuration whose blocks have a gradient path")
    return t.contiguous()


def _need_bias(bias, cout, who):
    """An optional per-output-channel bias: None, or a f32 cuda tensor of exactly `cout` elements (made contiguous: the kernels
    read bias[co] from a bare pointer, so a strided view or a longer buffer would be misread without an error)."""
    if bias is None:
        return None
    bias = _need(bias, torch.float32, "bias")
    if bias.numel() != cout:
        raise _capi.HealAmdError(f"{who}: bias has {bias.numel()} elements for {cout} output channels")
    return bias


def _need_rows(t, width, name, who):
    """A f32 cuda row matrix [n, width] (made contiguous).  No autograd check: the sparse encoder hands its activations over
    detached, and SparseTensor.features is never part of a recorded graph."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise _capi.HealAmdError(f"{who}: {name} must have dtype torch.float32, got {t.dtype}")
    if t.dim() != 2 or int(t.shape[1]) != width:
        raise _capi.HealAmdError(f"{who}: {name} has shape {tuple(t.shape)}, want [n, {width}]")
    return t.contiguous()


def _need_nbr(nbr, K, who):
    """A neighbour table [n_out, K] int32 on the device (made contiguous): the kernels read it as n_out * K int32 words from a
    bare pointer, so an int64 table or one with another tap count would be misread without an error."""
    if not isinstance(nbr, torch.Tensor) or not nbr.is_cuda:
        raise _capi.HealAmdError(f"{who}: nbr must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if nbr.dtype != torch.int32:
        raise _capi.HealAmdError(f"{who}: nbr must have dtype torch.int32, got {nbr.dtype}")
    if nbr.dim() != 2 or int(nbr.shape[1]) != K:
        raise _capi.HealAmdError(f"{who}: nbr has shape {tuple(nbr.shape)}, want [n_out, {K}] for a {K}-tap weight")
    return nbr.contiguous()


def _need_channels(t, cout, name, who):
    """A per-output-channel f32 vector of exactly `cout` elements (BatchNorm scale / shift of the sparse layers)."""
    t = _need(t, torch.float32, name)
    if t.numel() != cout:
        raise _capi.HealAmdError(f"{who}: {name} has {t.numel()} elements for {cout} output channels")
    return t


def _workspace(key, nbytes, device, zeroed=False):
    """Grow-only per-(op, device) scratch buffer (256-B aligned by the caching allocator).  A buffer that is outgrown is
    RETIRED (derived.retire), not freed: a captured HIP graph may have its address baked in, and handing the memory back to the
    caching allocator would let a later replay scribble over somebody else's tensor.  zeroed=True: scratch with a zero-on-entry /
    zero-on-exit contract (heal_bev_pool_pm), allocated zero-filled ONCE and then owned by the operator, which leaves it clean
    after every call."""
    # one scratch per (operator, device, STREAM): modalities encoded on concurrent streams must not share scratch
    k = (key, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(k)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            derived.retire(buf)
        buf = (torch.zeros if zeroed else torch.empty)(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS[k] = buf
    return buf


# ---- capacity checks of the no-host-sync sparse path ---------------------------------------------------------------------
# Strided sparse layers that run without a host round trip size their outputs by a capacity bound and record
# (device counter, capacity) here.  Whoever synchronises with the host next on the same stream (decode_nms(sync=True),
# ScenePipeline.replay) verifies them, so a frame denser than the bound raises instead of silently dropping sites.
_SPARSE_CHECKS = []


# Sticky form: a captured graph re-creates every n_out counter on each replay, so a check every N replays only sees
# the LAST frame.  The rank-path out_sites kernel also atomicMax-es an overflowing count into this per-device word, which no
# graph ever resets: verify_sparse_capacity() reads it, so an overflow on ANY replayed frame is reported at the next check.
_SPARSE_OVERFLOW = {}


def sparse_overflow_flag(device):
    """int32 [1] on `device`, persistent: max over all strided sparse layers of an n_out that exceeded its capacity (0 = none).
    Allocated at the first (eager) use, i.e. outside any graph capture."""
    key = str(device)
    flag = _SPARSE_OVERFLOW.get(key)
    if flag is None:
        flag = _SPARSE_OVERFLOW[key] = torch.zeros((1,), dtype=torch.int32, device=device)
    return flag


def take_sparse_checks():
    """Hand over (and forget) the pending checks, e.g. to keep those recorded inside a captured graph."""
    global _SPARSE_CHECKS
    out, _SPARSE_CHECKS = _SPARSE_CHECKS, []
    return out


def verify_sparse_capacity(checks=None):
    """Raise if any recorded strided sparse layer produced more active sites than its capacity (synchronises: one small
    D2H copy).  checks=None: verify and clear the pending list."""
    pending = take_sparse_checks() if checks is None else checks
    for key, flag in _SPARSE_OVERFLOW.items():
        worst = int(flag.item())
        if worst:
            flag.zero_()
            raise _capi.HealAmdError(
                f"sparse conv: a strided layer produced {worst} active sites on {key}, more than its capacity in the "
                "no-host-sync mode, on this or an earlier (replayed) frame (sites beyond the capacity were dropped: the result "
                "is invalid).  Feed exact-size voxel inputs or raise the capacity policy (SparseTensor.out_sites)")
    if not pending:
        return
    counts = torch.cat([c.reshape(1) for c, _ in pending]).cpu().tolist()
    for n, (_, cap) in zip(counts, pending):
        if n > cap:
            raise _capi.HealAmdError(
                f"sparse conv: a strided layer produced {n} active sites, more than its capacity {cap} in the no-host-sync "
                "mode (sites beyond the capacity were dropped: the result is invalid).  Feed exact-size voxel inputs or "
                "raise the capacity policy (SparseTensor.out_sites)")


def _host_array(values, ctype):
    arr = (ctype * len(values))(*values)
    return arr


# ------------------------------------------------------------------------------------------------
# K1's per-cell table is self-cleaning: a workspace that a finished call left behind needs no fill.  What persists in it is laid out by
# the table alone (heal_voxelize_layout), so there is ONE workspace per (stream, table slots, table kind) whatever the point count, and
# the scratch behind the table grows with the clouds.  _VOX_CLEAN: the (data_ptr, numel) of the buffers known to be clean.
_VOX_CLEAN = set()


def _vox_cells(lidar_range, voxel_size):
    """Cells of the voxel grid, as the library counts them (round((max - min) / size) per axis in fp64)."""
    c = 1
    for j in range(3):
        c *= int(round((float(np.float32(lidar_range[3 + j])) - float(np.float32(lidar_range[j]))) / float(np.float32(voxel_size[j]))))
    return max(c, 0)


def _vox_chain(name, dev, n, n_agents, max_points, max_voxels, agents_x_cells, *args):
    """Call heal_voxelize / heal_voxelize_batch (`args`: everything in front of ws) on the workspace of its table, with tables_clean
    from the bookkeeping; any failure leaves the workspace 'unknown'."""
    lay = (ctypes.c_size_t * 6)()
    _capi.call("heal_voxelize_layout", n, 1, max_points, agents_x_cells, lay)
    # sized for the next power of two of points (the carve is monotone in points and rows, so the call fits): a buffer is outgrown at
    # most once per doubling, and what _workspace retires on the way stays below the size of the live one
    capacity = max(1024, 1 << max(n - 1, 0).bit_length())
    nbytes = _capi.query("heal_voxelize_batch_workspace", capacity, n_agents, max_points, max_voxels, agents_x_cells)
    ws = _workspace(("voxelize", int(lay[0]), bool(lay[1])), nbytes, dev)
    ident = (ws.data_ptr(), ws.numel())
    clean = ident in _VOX_CLEAN
    if not clean:       # first use of this buffer: forget the one it replaced, if any (retired, it is never called again)
        _VOX_CLEAN.intersection_update({(b.data_ptr(), b.numel()) for b in _WS.values()})
    _VOX_CLEAN.discard(ident)
    with _Timed("voxelize"):
        _capi.call(name, *args, _ptr(ws), ws.numel(), 1 if clean else 0, _stream())
    # A call RECORDED into a graph has not run: if it carries the initial fill (workspace first seen inside a capture), the tables are
    # clean only once that graph has been replayed -- later calls must not rely on it, so the workspace stays 'unknown' (every capture
    # then carries its own fill; the first eager call settles it).
    if clean or not torch.cuda.is_current_stream_capturing():
        _VOX_CLEAN.add(ident)


def voxelize(points, lidar_range, voxel_size, max_points, max_voxels, batch_idx=0, sync=True):
    """K1.  points [N,4] f32 cuda -> (voxels [M,P,4], coords [M,4] (b,z,y,x) i32, num_points [M] i32).

    With sync=True (the SpVoxelPreprocessor contract: exact-size outputs) the voxel count is read
    back and the outputs are sliced; with sync=False the full-capacity buffers and the device
    counter are returned: (voxels, coords, num_points, n_voxels_dev)."""
    points = _need(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] != 4:
        raise _capi.HealAmdError("points must be [N,4]")
    n = int(points.shape[0])
    cap = max(1, min(n, int(max_voxels)))
    dev = points.device
    voxels = torch.empty((cap, max_points, 4), dtype=torch.float32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty((cap,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    rng = _host_array([float(v) for v in lidar_range], ctypes.c_float)
    vs = _host_array([float(v) for v in voxel_size], ctypes.c_float)
    _vox_chain("heal_voxelize", dev, n, 1, int(max_points), int(max_voxels), _vox_cells(lidar_range, voxel_size),
               _ptr(points), n, rng, vs, int(max_points), int(max_voxels), int(batch_idx),
               _ptr(voxels), _ptr(coords), _ptr(num), _ptr(count), None, None)
    if not sync:
        return voxels, coords, num, count
    m = int(count.item())
    return voxels[:m], coords[:m], num[:m]


def mask_points(points, limit_range=None, mask_ego=True, out=None):
    """pcd_utils.mask_points_by_range / mask_ego_points on the device: points [N,4] f32 cuda -> same-shape tensor in
    which dropped points are NaN (the voxeliser skips them; order and length are kept, so there is no host sync)."""
    points = _need(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] != 4:
        raise _capi.HealAmdError("points must be [N,4]")
    if out is None:
        out = torch.empty_like(points)
    rng = _host_array([float(v) for v in limit_range], ctypes.c_float) if limit_range is not None else None
    _capi.call("heal_mask_points", _ptr(points), int(points.shape[0]), rng, 1 if mask_ego else 0, _ptr(out), _stream())
    return out


def voxelize_collated(point_list, lidar_range, voxel_size, max_points, max_voxels):
    """K1 for every agent of a modality into ONE set of collated buffers (collate_batch_list,
    sp_voxel_preprocessor.py:110-147) without a host round trip: agent b's rows follow agent b-1's, the running row
    offset lives on the device.  -> (voxels [cap,P,4], coords [cap,4] (b,z,y,x), num_points [cap], offsets [n+1] i32
    device; offsets[b+1]-offsets[b] = voxels of agent b, offsets[n] = total); rows beyond the total are unspecified."""
    pts = [_need(p, torch.float32, "points") for p in point_list]
    for p in pts:
        if p.dim() != 2 or p.shape[1] != 4:
            raise _capi.HealAmdError("points must be [N,4]")
    dev = pts[0].device
    caps = [min(int(p.shape[0]), int(max_voxels)) for p in pts]
    cap = max(1, sum(caps))
    voxels = torch.empty((cap, max_points, 4), dtype=torch.float32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty((cap,), dtype=torch.int32, device=dev)
    offsets = torch.zeros((len(pts) + 1,), dtype=torch.int32, device=dev)
    rng = _host_array([float(v) for v in lidar_range], ctypes.c_float)
    vs = _host_array([float(v) for v in voxel_size], ctypes.c_float)
    if len(pts) <= 16:
        # ONE launch chain for all agents (heal_voxelize_batch): the clouds are concatenated, keys carry the agent
        bounds = [0]
        for p in pts:
            bounds.append(bounds[-1] + int(p.shape[0]))
        # clouds that already lie back to back in memory (pipeline.StaticInputs) are read in place
        adjacent = all(p.is_contiguous() for p in pts) and all(
            pts[i].data_ptr() + pts[i].numel() * 4 == pts[i + 1].data_ptr() for i in range(len(pts) - 1))
        allp = pts[0] if (len(pts) == 1 or adjacent) else torch.cat(pts, 0)
        _vox_chain("heal_voxelize_batch", dev, bounds[-1], len(pts), int(max_points), int(max_voxels),
                   len(pts) * _vox_cells(lidar_range, voxel_size),
                   _ptr(allp), _host_array(bounds, ctypes.c_int32), len(pts), rng, vs, int(max_points), int(max_voxels),
                   _ptr(voxels), _ptr(coords), _ptr(num), _ptr(offsets))
        _remember("voxelize", lambda: voxelize_collated(point_list, lidar_range, voxel_size, max_points, max_voxels))
        return voxels, coords, num, offsets
    counts = torch.zeros((len(pts),), dtype=torch.int32, device=dev)
    cells = _vox_cells(lidar_range, voxel_size)
    for b, p in enumerate(pts):
        n = int(p.shape[0])
        _vox_chain("heal_voxelize", dev, n, 1, int(max_points), int(max_voxels), cells,
                   _ptr(p), n, rng, vs, int(max_points), int(max_voxels), b, _ptr(voxels), _ptr(coords), _ptr(num),
                   _ptr(counts[b:b + 1]), _ptr(offsets[b:b + 1]), _ptr(offsets[b + 1:b + 2]))
    return voxels, coords, num, offsets


def pfn_scatter(voxels, coords, num_points, weight, bn_scale, bn_shift, voxel_size, lidar_range,
                n_agents, ny, nx, n_voxels_dev=None, return_pillars=False, out=None):
    """K2.  -> canvas [n_agents,64,ny,nx] (and pillar features [M,64] when asked)."""
    voxels = _need(voxels, torch.float32, "voxels")
    coords = _need(coords, torch.int32, "coords")
    num_points = _need(num_points, torch.int32, "num_points")
    weight = _need(weight, torch.float32, "weight")
    bn_scale = _need(bn_scale, torch.float32, "bn_scale")
    bn_shift = _need(bn_shift, torch.float32, "bn_shift")
    M, P = int(voxels.shape[0]), int(voxels.shape[1])
    C = int(weight.shape[0])
    if weight.shape[1] != 10 or voxels.shape[2] != 4 or coords.shape[1] != 4:
        raise _capi.HealAmdError("pfn_scatter: expected voxels [M,P,4], coords [M,4], weight [C,10]")
    dev = voxels.device
    if out is None:
        canvas = torch.empty((n_agents, C, ny, nx), dtype=torch.float32, device=dev)
    else:
        canvas = out
        if (tuple(canvas.shape) != (n_agents, C, ny, nx) or canvas.dtype != torch.float32
                or not canvas.is_contiguous() or not canvas.is_cuda):
            raise _capi.HealAmdError("pfn_scatter: `out` must be a contiguous f32 cuda [n_agents,C,ny,nx]")
    pillars = torch.empty((max(M, 1), C), dtype=torch.float32, device=dev)
    nbytes = _capi.query("heal_pfn_scatter_workspace", M, n_agents, ny, nx, C)
    ws = _workspace("pfn_scatter", nbytes, dev)
    vx, vy, vz = (float(v) for v in voxel_size)
    xo = vx / 2 + lidar_range[0]
    yo = vy / 2 + lidar_range[1]
    zo = vz / 2 + lidar_range[2]
    with _Timed("pfn_scatter"):
        _capi.call("heal_pfn_scatter", _ptr(voxels), _ptr(coords), _ptr(num_points), M, _ptr(n_voxels_dev), P,
                   _ptr(weight), _ptr(bn_scale), _ptr(bn_shift), C, vx, vy, vz, xo, yo, zo,
                   int(n_agents), int(ny), int(nx), _ptr(canvas), _ptr(pillars), _ptr(ws), ws.numel(), _stream())
    if return_pillars:
        return canvas, pillars[:M]
    return canvas


class PillarBEV:
    """K2's result WITHOUT the dense canvas: pillar feature rows [M, 64] + the cell -> pillar-row map [n_agents, ny, nx] (-1 = empty).
    It stands for PointPillarScatter's [n_agents, 64, ny, nx] canvas (point_pillar_scatter.py:19-76; 96 % zeros) until somebody
    needs it: `stem_block(...)` -- the first BasicBlock of the PointPillars ResNetBEVBackbone reads the pillars through the map
    (heal_pillar_stem_block); `dense()` -- anybody else gets the reference's tensor.  Same protocol as PooledBEV (K4)."""

    def __init__(self, pillars, cell_map, n_agents, ny, nx):
        self.pillars, self.cell_map = pillars, cell_map
        self.n_agents, self.ny, self.nx_ = int(n_agents), int(ny), int(nx)
        self.channels = int(pillars.shape[1])
        self.device = pillars.device

    @property
    def shape(self):
        return (self.n_agents, self.channels, self.ny, self.nx_)

    @property
    def is_cuda(self):
        return True

    def dense(self):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        with _Timed("pillar_canvas", nbytes=4.0 * out.numel()):
            _capi.call("heal_pillar_canvas", _ptr(self.cell_map), _ptr(self.pillars), self.n_agents, self.channels, self.ny,
                       self.nx_, _ptr(out), _stream())
        return out

    def stem_supported(self, cout_main, cout_down):
        return (self.channels == 64 and cout_main == 64 and cout_down == 64 and ((self.nx_ - 1) // 2 + 1) % 4 == 0)

    # weight layout of stem_block: "lanes" (pillar_stem_fragments, the pixel-compacted kernel) | "tiles" (stem_fragments, v1: A/B)
    weight_layout = "tiles" if switches.get("HEAL_PILLAR_STEM") == "1" else "lanes"

    def fragments(self, w_main, w_down):
        return pillar_stem_fragments(w_main, w_down) if self.weight_layout == "lanes" else stem_fragments(w_main, w_down)

    def stem_block(self, w_main, b_main, w_down, b_down):
        """relu(conv3x3_s2(canvas, W1) + b1), conv1x1_s2(canvas, Wd) + bd straight from the pillars; weights from
        self.fragments(...)."""
        Ho, Wo = (self.ny - 1) // 2 + 1, (self.nx_ - 1) // 2 + 1
        out_main = torch.empty((self.n_agents, 64, Ho, Wo), dtype=torch.float32, device=self.device)
        out_id = torch.empty_like(out_main)
        flops = 2.0 * self.n_agents * Ho * Wo * 64 * 64 * 10          # the dense convolutions it replaces
        with _Timed("pillar_stem_block", flops=flops, nbytes=8.0 * out_main.numel(), kernel_events=True):
            _capi.call("heal_pillar_stem_block", _ptr(self.pillars), _ptr(self.cell_map), self.n_agents, self.channels, self.ny,
                       self.nx_, _ptr(w_main), _ptr(b_main), _ptr(w_down), _ptr(b_down), 1 if self.weight_layout == "tiles" else 0,
                       _ptr(out_main), _ptr(out_id), _stream())
        return out_main, out_id


def pillar_stem_fragments(w_main, w_down):
    """Weights of heal_pillar_stem_block (layout 0): w_main [64, 64, 3, 3] -> [9][4][64][16] with frag[tap][w][16 lk + ln][ks] =
    W[16 w + ln][16 lk + ks][tap]; w_down [64, 64, 1, 1] -> [4][64][16] likewise (the 16x16x4 A operand of wave w with the
    reduction index permuted so that a lane's 16 k-steps are 16 consecutive input channels)."""
    if tuple(w_main.shape) != (64, 64, 3, 3) or tuple(w_down.shape) != (64, 64, 1, 1):
        raise _capi.HealAmdError("pillar_stem_fragments: expected [64, 64, 3, 3] and [64, 64, 1, 1]")
    # [co = (w, ln), ci = (lk, ks), tap] -> [tap, w, lk, ln, ks]
    wm = w_main.detach().to(torch.float32).reshape(4, 16, 4, 16, 9).permute(4, 0, 2, 1, 3).contiguous()
    wd = w_down.detach().to(torch.float32).reshape(4, 16, 4, 16).permute(0, 2, 1, 3).contiguous()
    return wm, wd


def pfn_pillars(voxels, coords, num_points, weight, bn_scale, bn_shift, voxel_size, lidar_range, n_agents, ny, nx,
                n_voxels_dev=None):
    """K2 without the canvas -> PillarBEV (pillar features [M, 64] + cell -> pillar map); see pfn_scatter for the arguments."""
    voxels = _need(voxels, torch.float32, "voxels")
    coords = _need(coords, torch.int32, "coords")
    num_points = _need(num_points, torch.int32, "num_points")
    weight = _need(weight, torch.float32, "weight")
    bn_scale = _need(bn_scale, torch.float32, "bn_scale")
    bn_shift = _need(bn_shift, torch.float32, "bn_shift")
    M, P = int(voxels.shape[0]), int(voxels.shape[1])
    C = int(weight.shape[0])
    if weight.shape[1] != 10 or voxels.shape[2] != 4 or coords.shape[1] != 4:
        raise _capi.HealAmdError("pfn_pillars: expected voxels [M,P,4], coords [M,4], weight [C,10]")
    dev = voxels.device
    pillars = torch.empty((max(M, 1), C), dtype=torch.float32, device=dev)
    cell_map = torch.empty((n_agents, ny, nx), dtype=torch.int32, device=dev)
    vx, vy, vz = (float(v) for v in voxel_size)
    xo, yo, zo = vx / 2 + lidar_range[0], vy / 2 + lidar_range[1], vz / 2 + lidar_range[2]
    with _Timed("pfn_pillars", nbytes=16.0 * M * P + 20.0 * M + 4.0 * C * M):
        _capi.call("heal_pfn_pillars", _ptr(voxels), _ptr(coords), _ptr(num_points), M, _ptr(n_voxels_dev), P,
                   _ptr(weight), _ptr(bn_scale), _ptr(bn_shift), C, vx, vy, vz, xo, yo, zo, int(n_agents), int(ny), int(nx),
                   _ptr(pillars), _ptr(cell_map), _stream())
    return PillarBEV(pillars, cell_map, n_agents, ny, nx)


def _pfn_geom(voxel_size, lidar_range):
    vx, vy, vz = (float(v) for v in voxel_size)
    return vx, vy, vz, vx / 2 + lidar_range[0], vy / 2 + lidar_range[1], vz / 2 + lidar_range[2]


def _pfn_inputs(voxels, coords, num_points):
    voxels = _need(voxels, torch.float32, "voxels")
    coords = _need(coords, torch.int32, "coords")
    num_points = _need(num_points, torch.int32, "num_points")
    if voxels.dim() != 3 or voxels.shape[2] != 4 or coords.shape[1] != 4 or int(voxels.shape[1]) > 32:
        raise _capi.HealAmdError("pfn (training kernels): expected voxels [M,P<=32,4], coords [M,4]")
    return voxels, coords, num_points


def pfn_train_supported(voxels, weight=None):
    """heal_pfn_features / _moments / _backward are written for Linear(10 -> 64) (PillarVFE with num_filters [64]); any other
    width must take the torch path (the kernels would read weight / bn rows out of bounds)."""
    if weight is not None and tuple(weight.shape) != (64, 10):
        return False
    return voxels.is_cuda and voxels.dim() == 3 and 1 <= int(voxels.shape[1]) <= 32 and int(voxels.shape[0]) >= 1


def pfn_moments(voxels, coords, num_points, voxel_size, lidar_range):
    """-> (s1 [10], S [10,10]) float64: sums over all M x P rows of the decorated, masked point features f and of f f^T."""
    voxels, coords, num_points = _pfn_inputs(voxels, coords, num_points)
    M, P = int(voxels.shape[0]), int(voxels.shape[1])
    nb = _capi.query("heal_pfn_train_blocks", M)
    part = torch.empty((nb, 65), dtype=torch.float32, device=voxels.device)
    _capi.call("heal_pfn_moments", _ptr(voxels), _ptr(coords), _ptr(num_points), M, P, *_pfn_geom(voxel_size, lidar_range),
               _ptr(part), _stream())
    tot = part.double().sum(0)
    S = torch.zeros((10, 10), dtype=torch.float64, device=voxels.device)
    iu = torch.triu_indices(10, 10, device=voxels.device)
    S[iu[0], iu[1]] = tot[10:]
    S = S + S.t() - torch.diag(torch.diag(S))
    return tot[:10], S


def pfn_features(voxels, coords, num_points, weight, bn_scale, bn_shift, voxel_size, lidar_range):
    """Pillar features [M,64] = max over the points of relu(scale (W f) + shift): K2's first stage without the canvas."""
    voxels, coords, num_points = _pfn_inputs(voxels, coords, num_points)
    M, P = int(voxels.shape[0]), int(voxels.shape[1])
    out = torch.empty((M, 64), dtype=torch.float32, device=voxels.device)
    if tuple(weight.shape) != (64, 10) or bn_scale.numel() != 64 or bn_shift.numel() != 64:
        raise _capi.HealAmdError("pfn_features: the kernel is written for Linear(10 -> 64) (weight [64, 10], 64 BN channels)")
    _capi.call("heal_pfn_features", _ptr(voxels), _ptr(coords), _ptr(num_points), M, P, _ptr(_need(weight, torch.float32, "weight")),
               _ptr(_need(bn_scale, torch.float32, "bn_scale")), _ptr(_need(bn_shift, torch.float32, "bn_shift")),
               *_pfn_geom(voxel_size, lidar_range), _ptr(out), _stream())
    return out


def pfn_backward(voxels, coords, num_points, weight, bn_scale, bn_shift, mean, rstd, voxel_size, lidar_range, grad_pillar):
    """-> (A [64,10], B [64], Cx [64]) float64: sum dy f_{p*}, sum dy, sum dy xhat_{p*} over the pillars (include/heal_amd.h)."""
    voxels, coords, num_points = _pfn_inputs(voxels, coords, num_points)
    M, P = int(voxels.shape[0]), int(voxels.shape[1])
    nb = _capi.query("heal_pfn_train_blocks", M)
    part = torch.empty((nb, 64, 12), dtype=torch.float32, device=voxels.device)
    if tuple(weight.shape) != (64, 10) or bn_scale.numel() != 64 or bn_shift.numel() != 64:
        raise _capi.HealAmdError("pfn_backward: the kernel is written for Linear(10 -> 64) (weight [64, 10], 64 BN channels)")
    _capi.call("heal_pfn_backward", _ptr(voxels), _ptr(coords), _ptr(num_points), M, P, _ptr(_need(weight, torch.float32, "weight")),
               _ptr(_need(bn_scale, torch.float32, "bn_scale")), _ptr(_need(bn_shift, torch.float32, "bn_shift")),
               _ptr(_need(mean, torch.float32, "mean")), _ptr(_need(rstd, torch.float32, "rstd")),
               *_pfn_geom(voxel_size, lidar_range), _ptr(_need(grad_pillar, torch.float32, "grad_pillar")), _ptr(part), _stream())
    tot = part.double().sum(0)
    return tot[:, :10], tot[:, 10], tot[:, 11]


def _affine_args(affine_rows, n):
    """-> (keep-alive object, host pointer, device pointer).  A CUDA tensor of affine rows stays on the device (no host
    round trip; a captured graph then reads the poses at replay time); anything else is passed by value from the host."""
    if isinstance(affine_rows, torch.Tensor) and affine_rows.is_cuda:
        a = affine_rows.detach()
        if a.dtype != torch.float64:
            a = a.double()
        a = a.reshape(-1, 6).contiguous()
        if int(a.shape[0]) != n:
            raise _capi.HealAmdError(f"affine rows: expected {n} x (2,3), got {tuple(affine_rows.shape)}")
        return a, ctypes.c_void_p(0), ctypes.c_void_p(a.data_ptr())
    if isinstance(affine_rows, torch.Tensor):
        affine_rows = affine_rows.detach().numpy()
    a = np.ascontiguousarray(np.asarray(affine_rows, dtype=np.float64).reshape(-1, 6))
    if a.shape[0] != n:
        raise _capi.HealAmdError(f"affine rows: expected {n} x (2,3), got {a.shape}")
    return a, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(0)


def _crop_host(crop, n):
    if crop is None:
        return None, ctypes.c_void_p(0)
    c = np.ascontiguousarray(np.asarray(crop, dtype=np.int32).reshape(n, 4))
    return c, c.ctypes.data_as(ctypes.c_void_p)


def _level_crops_host(crops, L, n):
    """The crop table [L, n, 4] of a pyramid: crops[l] = per-agent (h0,h1,w0,w1) | None; a missing level or agent keeps everything."""
    if crops is None or all(c is None for c in crops):
        return None, ctypes.c_void_p(0)
    carr = np.zeros((L, n, 4), dtype=np.int32)
    for l, c in enumerate(crops):
        if c is not None:
            carr[l] = np.asarray([ci if ci is not None else (0, 0, 0, 0) for ci in c], dtype=np.int32).reshape(n, 4)
    return carr, carr.ctypes.data_as(ctypes.c_void_p)


def warp_fuse(feats, occ, affine_rows, grid_f64=True, crop=None):
    """K5 fused.  feats [n,C,H,W], occ [n,1,H,W] logits, affine_rows [n,2,3] (host array, or a CUDA tensor that is then
    read on the device at run time) -> [C,H,W]."""
    feats = _need(feats, torch.float32, "feats")
    occ = _need(occ, torch.float32, "occ")
    n, C, H, W = (int(v) for v in feats.shape)
    out = torch.empty((C, H, W), dtype=torch.float32, device=feats.device)
    a, ap, adev = _affine_args(affine_rows, n)
    c, cp = _crop_host(crop, n)
    with _Timed(f"warp_fuse_c{C}", 0.0, 4.0 * H * W * (n * (C + 1) + C)):   # read every agent's map + score, write one
        _capi.call("heal_warp_fuse", _ptr(feats), _ptr(occ), n, C, H, W, ap, adev, int(bool(grid_f64)), cp,
                   _ptr(out), _stream())
    return out


def warp_fuse_levels(feats_list, occ_list, affine_rows, grid_f64=True, crops=None):
    """K5 for every pyramid level of one scene in ONE launch (heal_warp_fuse_levels: LDS-staged source footprints).
    feats_list[l] [n,C_l,H_l,W_l], occ_list[l] [n,1,H_l,W_l] logits, affine_rows [n,2,3] (host array or CUDA tensor, shared by
    the levels), crops[l] = per-agent (h0,h1,w0,w1) | None -> list of [C_l,H_l,W_l]."""
    L = len(feats_list)
    feats_list = [_need(f, torch.float32, "feats") for f in feats_list]
    occ_list = [_need(o, torch.float32, "occ") for o in occ_list]
    n = int(feats_list[0].shape[0])
    outs, nbytes = [], 0.0
    for f, o in zip(feats_list, occ_list):
        if int(f.shape[0]) != n or tuple(o.shape) != (n, 1, int(f.shape[2]), int(f.shape[3])):
            raise _capi.HealAmdError("warp_fuse_levels: inconsistent level shapes")
        C, H, W = (int(v) for v in f.shape[1:])
        outs.append(torch.empty((C, H, W), dtype=torch.float32, device=f.device))
        nbytes += 4.0 * H * W * (n * (C + 1) + C)
    a, ap, adev = _affine_args(affine_rows, n)
    carr, cp = _level_crops_host(crops, L, n)
    fp = _host_array([f.data_ptr() for f in feats_list], ctypes.c_void_p)
    op = _host_array([o.data_ptr() for o in occ_list], ctypes.c_void_p)
    yp = _host_array([y.data_ptr() for y in outs], ctypes.c_void_p)
    with _Timed("warp_fuse_levels", 0.0, nbytes, kernel_events=True):
        _capi.call("heal_warp_fuse_levels", L, fp, op, n, _host_array([int(f.shape[1]) for f in feats_list], ctypes.c_int32),
                   _host_array([int(f.shape[2]) for f in feats_list], ctypes.c_int32),
                   _host_array([int(f.shape[3]) for f in feats_list], ctypes.c_int32), ap, adev, int(bool(grid_f64)), cp, yp,
                   _stream())
    return outs


class K5Source(ctypes.Structure):
    """heal_k5_source (include/heal_amd.h): where one agent's map of one level lies."""
    _fields_ = [("feat", ctypes.c_void_p), ("occ", ctypes.c_void_p), ("feat_row", ctypes.c_int64), ("feat_plane", ctypes.c_int64),
                ("occ_row", ctypes.c_int64), ("box", ctypes.c_int32 * 4)]


def warp_fuse_levels_src(sources, shapes, affine_rows, grid_f64=True, crops=None, outs=None):
    """warp_fuse_levels with every agent's map read IN PLACE (heal_warp_fuse_levels_src): no stacked [n, C, H, W] tensor.
    sources[l][a] = (feat, occ, (y0, x0)): feat a [C_l, bh, bw] view and occ a [bh, bw] view (unit stride along x, any row / plane
    stride: a dense crop or a slice of a larger tensor) that hold the agent's map on the box (y0, y0 + bh, x0, x0 + bw) of the
    level's H_l x W_l grid; shapes[l] = (H_l, W_l); crops as warp_fuse_levels.  An agent with a crop window needs window +- 1 inside
    its box, an agent without one the full map (checked by the library) -> list of [C_l, H_l, W_l], bit-identical to
    warp_fuse_levels on the zero-padded stack.  outs: optional preallocated contiguous [C_l, H_l, W_l] outputs."""
    L = len(sources)
    n = len(sources[0])
    desc = (K5Source * (L * n))()
    given, outs = outs, []
    chans, keep, nbytes = [], [], 0.0
    for l, (level, (H, W)) in enumerate(zip(sources, shapes)):
        if len(level) != n:
            raise _capi.HealAmdError("warp_fuse_levels_src: every level needs one source per agent")
        C = int(level[0][0].shape[0])
        for a, (f, o, (y0, x0)) in enumerate(level):
            for t, name in ((f, "feat"), (o, "occ")):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
                    raise _capi.HealAmdError(f"warp_fuse_levels_src: {name} must be a float32 CUDA/HIP tensor")
            if (f.dim() != 3 or o.dim() != 2 or int(f.shape[0]) != C or tuple(f.shape[1:]) != tuple(o.shape)
                    or (f.shape[2] > 1 and f.stride(2) != 1) or (o.shape[1] > 1 and o.stride(1) != 1)):
                raise _capi.HealAmdError("warp_fuse_levels_src: feat [C, bh, bw] and occ [bh, bw] views with unit stride along x")
            bh, bw = int(o.shape[0]), int(o.shape[1])
            d = desc[l * n + a]
            d.feat, d.occ = f.data_ptr(), o.data_ptr()
            d.feat_row, d.feat_plane, d.occ_row = int(f.stride(1)), int(f.stride(0)), int(o.stride(0))
            d.box[:] = [int(y0), int(y0) + bh, int(x0), int(x0) + bw]
            keep += [f, o]
            nbytes += 4.0 * bh * bw * (C + 1)
        dev = level[0][0].device
        if given is not None:
            y = _need(given[l], torch.float32, "out")
            if y is not given[l] or tuple(y.shape) != (C, int(H), int(W)):
                raise _capi.HealAmdError("warp_fuse_levels_src: outs[l] must be a contiguous [C_l, H_l, W_l] tensor")
        outs.append(given[l] if given is not None else torch.empty((C, int(H), int(W)), dtype=torch.float32, device=dev))
        chans.append(C)
        nbytes += 4.0 * C * H * W
    a, ap, adev = _affine_args(affine_rows, n)
    carr, cp = _level_crops_host(crops, L, n)
    yp = _host_array([y.data_ptr() for y in outs], ctypes.c_void_p)
    with _Timed("warp_fuse_levels", 0.0, nbytes, kernel_events=True):
        _capi.call("heal_warp_fuse_levels_src", L, ctypes.cast(desc, ctypes.c_void_p), n, _host_array(chans, ctypes.c_int32),
                   _host_array([int(s[0]) for s in shapes], ctypes.c_int32), _host_array([int(s[1]) for s in shapes], ctypes.c_int32),
                   ap, adev, int(bool(grid_f64)), cp, yp, _stream())
    return outs


WARP_ATT_MAX_AGENTS, WARP_ATT_MAX_LEVELS = WARP_MAX_AGENTS, WARP_MAX_LEVELS


def warp_att_fuse_levels(feats_list, affine_rows, grid_f64=True, mode="att", sqrt_dims=None, outs=None, masks=None):
    """CoAlign's multiscale fusion for every level of one scene in ONE launch (heal_warp_att_fuse_levels): per ego pixel the
    agents' maps are warped into the ego frame (agent 0 included) and reduced with the ego row of the per-pixel agent attention
    (mode "att": softmax_j(x_0 . x_j / sqrt_dim) weights) or the maximum over agents (mode "max").
    feats_list[l] [n,C_l,H_l,W_l] fp32, affine_rows [n,2,3] (host array or CUDA tensor read at run time, shared by the levels),
    sqrt_dims[l]: the divisor of the logits (None: sqrt(C_l)) -> list of [C_l,H_l,W_l] (outs[l] when the caller gives the
    destinations: one contiguous fp32 tensor of that shape per level, on the level's device).
    masks[l] [n,1,H_l,W_l] fp32 (Where2comm's communication masks; None: no masking): heal_warp_att_fuse_levels_masked, every
    tap of agent j times the mask value at that tap -- the result on maps premultiplied by their masks, which are never written."""
    if mode not in ("att", "max"):
        raise _capi.HealAmdError(f"warp_att_fuse_levels: mode must be 'att' or 'max', got {mode!r}")
    L = len(feats_list)
    if not 1 <= L <= WARP_ATT_MAX_LEVELS:
        raise _capi.HealAmdError(f"warp_att_fuse_levels: 1..{WARP_ATT_MAX_LEVELS} levels per launch (got {L})")
    feats_list = [_need(f, torch.float32, "feats") for f in feats_list]
    if any(f.dim() != 4 for f in feats_list):
        raise _capi.HealAmdError("warp_att_fuse_levels: every level must be [n, C, H, W]")
    n = int(feats_list[0].shape[0])
    if any(int(f.shape[0]) != n for f in feats_list):
        raise _capi.HealAmdError(f"warp_att_fuse_levels: levels with different agent counts {[int(f.shape[0]) for f in feats_list]}")
    if not 1 <= n <= WARP_ATT_MAX_AGENTS:
        raise _capi.HealAmdError(f"warp_att_fuse_levels: 1..{WARP_ATT_MAX_AGENTS} agents per scene (got {n})")
    if sqrt_dims is not None and len(sqrt_dims) != L:
        raise _capi.HealAmdError(f"warp_att_fuse_levels: {len(sqrt_dims)} sqrt_dims for {L} levels")
    if outs is not None and len(outs) != L:
        raise _capi.HealAmdError(f"warp_att_fuse_levels: {len(outs)} outs for {L} levels")
    if masks is not None:                                   # the same checks as the feature maps, before anything is launched
        if len(masks) != L:
            raise _capi.HealAmdError(f"warp_att_fuse_levels: {len(masks)} masks for {L} levels")
        masks = [_need(m, torch.float32, "masks") for m in masks]
        for l, (m, f) in enumerate(zip(masks, feats_list)):
            if tuple(m.shape) != (n, 1, int(f.shape[2]), int(f.shape[3])) or m.device != f.device:
                raise _capi.HealAmdError(f"warp_att_fuse_levels: level {l}: the mask is {tuple(m.shape)} on {m.device}, want "
                                         f"{(n, 1, int(f.shape[2]), int(f.shape[3]))} on {f.device}")
    given, outs, nbytes = outs, [], 0.0
    for l, f in enumerate(feats_list):                      # every destination is checked before anything is launched
        C, H, W = (int(v) for v in f.shape[1:])
        outs.append(_out_like(None if given is None else given[l], (C, H, W), f.device, f"warp_att_fuse_levels: level {l}"))
        nbytes += 4.0 * H * W * (n * C + C)                 # compulsory traffic: every agent's map once, the fused map once
    a, ap, adev = _affine_args(affine_rows, n)
    sd = [float(np.float32(np.sqrt(int(f.shape[1])) if sqrt_dims is None else sqrt_dims[l])) for l, f in enumerate(feats_list)]
    fp = _host_array([f.data_ptr() for f in feats_list], ctypes.c_void_p)
    yp = _host_array([y.data_ptr() for y in outs], ctypes.c_void_p)
    shape = (_host_array([int(f.shape[1]) for f in feats_list], ctypes.c_int32),
             _host_array([int(f.shape[2]) for f in feats_list], ctypes.c_int32),
             _host_array([int(f.shape[3]) for f in feats_list], ctypes.c_int32), _host_array(sd, ctypes.c_float))
    if masks is not None:
        nbytes += sum(4.0 * m.numel() for m in masks)
        _capi.guard_note("heal_warp_att_fuse_levels_masked", [t.data_ptr() for t in feats_list + masks + outs])
        with _Timed("warp_att_fuse_levels_masked", 0.0, nbytes, kernel_events=True):
            _capi.call("heal_warp_att_fuse_levels_masked", L, fp, _host_array([m.data_ptr() for m in masks], ctypes.c_void_p), n,
                       *shape, ap, adev, int(bool(grid_f64)), 0 if mode == "att" else 1, yp, _stream())
        return outs
    with _Timed("warp_att_fuse_levels", 0.0, nbytes, kernel_events=True):
        _capi.call("heal_warp_att_fuse_levels", L, fp, n, *shape,
                   ap, adev, int(bool(grid_f64)), 0 if mode == "att" else 1, yp, _stream())
    return outs


COMM_MAX_K = _capi.header_define("HEAL_COMM_MAX_K", _capi.HEADER_COMM)
COMM_MAX_AGENTS = _capi.header_define("HEAL_COMM_MAX_AGENTS", _capi.HEADER_COMM)


def comm_fused_enabled():
    """HEAL_COMM_FUSED as the library reads it (heal_comm_fused_enabled: the variable is one of the library's own, declared as such
    in heal_amd/switches.py): False for "0" -- Where2comm then runs the reference's torch composition on the device."""
    v = int(_capi.lib().heal_comm_fused_enabled())
    if v < 0:
        raise _capi.HealAmdError("HEAL_COMM_FUSED is not a valid setting: expected 0 or 1")
    return v == 1


def comm_mask(psm, record_len, weight, bias, thre, n_levels=1):
    """CM.  Where2comm's communication masks of every scene of a batch and every pyramid level in one pass (heal_comm_mask;
    comm_modules/where2comm.py:34-78 with the max_pool2d per level of where2comm_attn.py:264-275).
    psm [n_total, A, H, W] f32 cuda confidence logits, record_len the agents per scene (a list, or a tensor read on the host),
    weight [.., k, k] and bias [1] the smoothing filter's parameters on the device (weight None: no smoothing), thre the threshold
    -> (masks: list of [n_total, 1, H >> l, W >> l] f32 zeros and ones with the even-agent override applied,
        count [B] int32: the ones of each scene's first agent before the override,
        rate [] f32: mean over scenes of count / (H W)).  No gradient flows through it (the reference's mask has none either)."""
    who = "comm_mask"
    if not isinstance(psm, torch.Tensor) or not psm.is_cuda or psm.dtype != torch.float32 or psm.dim() != 4:
        raise _capi.HealAmdError(f"{who}: psm must be a CUDA/HIP f32 map [n_total, A, H, W] (heal_amd has no CPU path)")
    x = psm.detach().contiguous()
    n_total, A, H, W = (int(v) for v in x.shape)
    lens = [int(v) for v in (record_len.tolist() if isinstance(record_len, torch.Tensor) else record_len)]
    if not lens or min(lens) < 1 or sum(lens) != n_total:
        raise _capi.HealAmdError(f"{who}: record_len {lens} does not sum to the {n_total} agents of psm")
    k = 1
    if weight is not None:
        if bias is None:
            raise _capi.HealAmdError(f"{who}: a filter weight without a bias")
        for t, name in ((weight, "weight"), (bias, "bias")):
            if not isinstance(t, torch.Tensor) or t.device != x.device or t.dtype != torch.float32:
                raise _capi.HealAmdError(f"{who}: {name} must be a f32 tensor on {x.device}")
        k = int(weight.shape[-1])
        if weight.dim() < 2 or int(weight.shape[-2]) != k or weight.numel() != k * k or bias.numel() != 1:
            raise _capi.HealAmdError(f"{who}: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} are not a [k, k] filter and "
                                     "one bias")
        if k % 2 == 0 or not 1 <= k <= COMM_MAX_K:
            raise _capi.HealAmdError(f"{who}: the filter size must be odd and in [1, {COMM_MAX_K}] (got {k})")
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
    n_levels = int(n_levels)
    if not _capi.lib().heal_comm_mask_supported(n_total, len(lens), A, H, W, k, n_levels):
        raise _capi.HealAmdError(f"{who}: unsupported problem: {n_total} agents in {len(lens)} scenes (at most {COMM_MAX_AGENTS}), "
                                 f"map {A} x {H} x {W}, filter {k}, {n_levels} levels (1..{WARP_MAX_LEVELS})")
    dev = x.device
    masks = [torch.empty((n_total, 1, H >> l, W >> l), dtype=torch.float32, device=dev) for l in range(n_levels)]
    count = torch.empty((len(lens),), dtype=torch.int32, device=dev)
    rate = torch.empty((), dtype=torch.float32, device=dev)
    ws = _workspace("comm_mask", _capi.query("heal_comm_mask_workspace", len(lens), H, W), dev)
    _capi.guard_note("heal_comm_mask", [m.data_ptr() for m in masks])
    with _Timed("comm_mask", nbytes=4.0 * (x.numel() + sum(m.numel() for m in masks)), kernel_events=True):
        _capi.call("heal_comm_mask", _ptr(x), n_total, A, H, W, _host_array(lens, ctypes.c_int32), len(lens), _ptr(weight),
                   _ptr(bias), k, float(thre), n_levels, _host_array([m.data_ptr() for m in masks], ctypes.c_void_p), _ptr(count),
                   _ptr(rate), _ptr(ws), ws.numel(), _stream())
    return masks, count, rate


DISCO_MAX_AGENTS = WARP_MAX_AGENTS
DISCO_WIDTHS = (128, 32, 8)        # PixelWeightLayer: 2C -> 128 -> 32 -> 8 -> 1


def disco_fuse(feats, affine_rows, grid_f64, e0, w1n_frag, w2, b2, w3, b3, w4, b4, return_scores=False, out=None, scores=None):
    """DiscoNet's fusion of one scene in ONE launch (heal_disco_fuse; fusion_in_one.py:153-201): every agent warped into the ego
    frame, one logit per (agent, pixel) from the PixelWeightLayer over cat(warped neighbour, unwarped ego), softmax over agents,
    weighted sum.  BatchNorm folded by the caller, layer 1 split by input half:
    feats [n,C,H,W] fp32 (1..8 agents, C % 4 == 0), affine_rows [n,2,3] (host array or CUDA tensor read at run time),
    e0 [128,H,W] = W1e x_0 + b1, w1n_frag = mfma_a_fragments(W1n [128,C]) [8,C/4,64], w2 [32,128], b2 [32], w3 [8,32], b3 [8],
    w4 [8], b4 [1] -> out [C,H,W], or (out, scores [n,H,W] post-ReLU logits) with return_scores.  `out` / `scores`: the caller's
    destinations (contiguous f32 tensors of those shapes on feats' device; `scores` only with return_scores), written in place."""
    who = "disco_fuse"
    feats = _need(feats, torch.float32, "feats")
    if feats.dim() != 4:
        raise _capi.HealAmdError(f"{who}: feats must be [n, C, H, W], got {tuple(feats.shape)}")
    n, C, H, W = (int(v) for v in feats.shape)
    if not 1 <= n <= DISCO_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: 1..{DISCO_MAX_AGENTS} agents per scene (got {n})")
    if C % 4 or C < 4:
        raise _capi.HealAmdError(f"{who}: C must be a positive multiple of the MFMA k-step 4 (got {C})")
    m1, m2, m3 = DISCO_WIDTHS
    if scores is not None and not return_scores:
        raise _capi.HealAmdError(f"{who}: `scores` given without return_scores")
    out = _out_like(out, (C, H, W), feats.device, who)
    scores = _out_like(scores, (n, H, W), feats.device, who, "scores") if return_scores else None
    if n == 1 and not return_scores and all(t is None for t in (e0, w1n_frag, w2, b2, w3, b3, w4, b4)):
        # the softmax of one logit is exactly 1: the warped map, no PixelWeightLayer operands
        a, ap, adev = _affine_args(affine_rows, n)
        with _Timed(f"disco_fuse_c{C}", 2.0 * C * H * W, 8.0 * C * H * W, kernel_events=True):
            _capi.call("heal_disco_fuse", _ptr(feats), n, C, H, W, ap, adev, int(bool(grid_f64)), *([None] * 8), _ptr(out), None,
                       _stream())
        return out
    e0 = _need(e0, torch.float32, "e0")
    if tuple(e0.shape) != (m1, H, W):
        raise _capi.HealAmdError(f"{who}: e0 has shape {tuple(e0.shape)}, want {(m1, H, W)}")
    w1n_frag = _need(w1n_frag, torch.float32, "w1n_frag")
    if tuple(w1n_frag.shape) != (m1 // 16, C // 4, 64):
        raise _capi.HealAmdError(f"{who}: w1n_frag has shape {tuple(w1n_frag.shape)}, want {(m1 // 16, C // 4, 64)} for C = {C} "
                                 "(ops.mfma_a_fragments of the [128, C] neighbour half)")
    w2 = _need(w2, torch.float32, "w2")
    w3 = _need(w3, torch.float32, "w3")
    if tuple(w2.shape) != (m2, m1) or tuple(w3.shape) != (m3, m2):
        raise _capi.HealAmdError(f"{who}: w2 {tuple(w2.shape)} / w3 {tuple(w3.shape)}, want {(m2, m1)} / {(m3, m2)}")
    b2 = _need_channels(b2, m2, "b2", who)
    b3 = _need_channels(b3, m3, "b3", who)
    w4 = _need_channels(w4, m3, "w4", who)
    b4 = _need_channels(b4, 1, "b4", who)
    w2_frag = _derived("disco_w2_fragments", (w2,), lambda: mfma_a_fragments(w2))
    a, ap, adev = _affine_args(affine_rows, n)
    flops = 2.0 * n * H * W * (m1 * C + m2 * m1 + m3 * m2 + m3) + 2.0 * n * C * H * W
    # compulsory traffic: every agent's map once, the ego term, the fused map (and the logits when asked for)
    nbytes = 4.0 * H * W * (n * C + m1 + C + (n if return_scores else 0))
    with _Timed(f"disco_fuse_c{C}", flops, nbytes, kernel_events=True):
        _capi.call("heal_disco_fuse", _ptr(feats), n, C, H, W, ap, adev, int(bool(grid_f64)), _ptr(e0), _ptr(w1n_frag),
                   _ptr(w2_frag), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(w4), _ptr(b4), _ptr(out), _optr(scores), _stream())
    return (out, scores) if return_scores else out


W2C_MAX_AGENTS = _limit("HEAL_WARP_MAX_AGENTS")       # heal_warp_mha_fuse (include/heal_amd_ext.h)


def warp_mha_fuse(q_map, kv_map, x_ego, bq, bk, bv, heads, affine_rows, grid_f64=True, scale=None, return_logits=False, outs=None,
                  logits=None):
    """Where2comm's fusion of one scene between its projections and its out-projection in ONE launch (heal_warp_mha_fuse;
    fusion_in_one.py:431-484): the projected maps of every agent sampled in the ego frame, the projection biases added after
    sampling, multi-head attention of the ego pixel over ALL agents (no key mask), and the warped ego map (the residual).
    q_map [C,H,W] = Wq x_0 and kv_map [n,2C,H,W] = [Wk; Wv] x_j: projections of the UNWARPED maps without bias; x_ego [C,H,W] the
    ego's unwarped map; bq, bk, bv [C]; 1..W2C_MAX_AGENTS agents, C % heads == 0; affine_rows [n,2,3] (host array or CUDA tensor
    read at run time); scale: the factor on q (None: 1 / sqrt(C / heads))
    -> (ctx [C,H,W], ego_warped [C,H,W]), and the scaled logits [n,heads,H,W] with return_logits.  `outs` = (ctx, ego_warped) /
    `logits`: the caller's destinations (contiguous f32 tensors of those shapes on q_map's device; `logits` only with
    return_logits), written in place."""
    who = "warp_mha_fuse"
    q_map = _need(q_map, torch.float32, "q_map")
    kv_map = _need(kv_map, torch.float32, "kv_map")
    x_ego = _need(x_ego, torch.float32, "x_ego")
    if q_map.dim() != 3:
        raise _capi.HealAmdError(f"{who}: q_map must be [C, H, W], got {tuple(q_map.shape)}")
    C, H, W = (int(v) for v in q_map.shape)
    heads = int(heads)
    if heads < 1 or C % heads:
        raise _capi.HealAmdError(f"{who}: C = {C} is not a multiple of heads = {heads}")
    if kv_map.dim() != 4 or tuple(kv_map.shape[1:]) != (2 * C, H, W):
        raise _capi.HealAmdError(f"{who}: kv_map has shape {tuple(kv_map.shape)}, want [n, {2 * C}, {H}, {W}] (K over V)")
    n = int(kv_map.shape[0])
    if not 1 <= n <= W2C_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: 1..{W2C_MAX_AGENTS} agents per scene (got {n})")
    if tuple(x_ego.shape) != (C, H, W):
        raise _capi.HealAmdError(f"{who}: x_ego has shape {tuple(x_ego.shape)}, want {(C, H, W)}")
    bq = _need_channels(bq, C, "bq", who)
    bk = _need_channels(bk, C, "bk", who)
    bv = _need_channels(bv, C, "bv", who)
    a, ap, adev = _affine_args(affine_rows, n)
    scale = float((C // heads) ** -0.5 if scale is None else scale)
    dev = q_map.device
    if outs is not None and (not isinstance(outs, (list, tuple)) or len(outs) != 2):
        raise _capi.HealAmdError(f"{who}: `outs` must be the pair (ctx, ego_warped)")
    if logits is not None and not return_logits:
        raise _capi.HealAmdError(f"{who}: `logits` given without return_logits")
    ctx = _out_like(None if outs is None else outs[0], (C, H, W), dev, who, "outs[0]")
    ego_warped = _out_like(None if outs is None else outs[1], (C, H, W), dev, who, "outs[1]")
    logits = _out_like(logits, (n, heads, H, W), dev, who, "logits") if return_logits else None
    flops = 2.0 * H * W * C * (2 * n + 1) + 8.0 * H * W * C * (2 * n + 2)      # the dot products and sums; 4 taps per sample
    # compulsory traffic: Q, the ego map and every agent's K and V once, the context and the warped ego (and the logits when asked)
    nbytes = 4.0 * H * W * ((2 * n + 2) * C + 2 * C + (n * heads if return_logits else 0))
    with _Timed(f"warp_mha_fuse_c{C}", flops, nbytes, kernel_events=True):
        _capi.call("heal_warp_mha_fuse", _ptr(q_map), _ptr(kv_map), _ptr(x_ego), _ptr(bq), _ptr(bk), _ptr(bv), n, C, heads, H, W,
                   scale, ap, adev, int(bool(grid_f64)), _ptr(ctx), _ptr(ego_warped), _optr(logits), _stream())
    return (ctx, ego_warped, logits) if return_logits else (ctx, ego_warped)


def warp_fuse_backward(feats, occ, affine_rows, grad_out, grid_f64=True, crop=None):
    """Gradient of warp_fuse with respect to (feats, occ): grad_out [C,H,W] -> ([n,C,H,W], [n,1,H,W])."""
    feats = _need(feats, torch.float32, "feats")
    occ = _need(occ, torch.float32, "occ")
    grad_out = _need(grad_out, torch.float32, "grad_out")
    n, C, H, W = (int(v) for v in feats.shape)
    g_feats, g_occ = torch.zeros_like(feats), torch.zeros_like(occ)
    a, ap, adev = _affine_args(affine_rows, n)
    c, cp = _crop_host(crop, n)
    with _Timed(f"warp_fuse_backward_c{C}"):
        _capi.call("heal_warp_fuse_backward", _ptr(feats), _ptr(occ), n, C, H, W, ap, adev, int(bool(grid_f64)), cp,
                   _ptr(grad_out), _ptr(g_feats), _ptr(g_occ), _stream())
    return g_feats, g_occ


def warp_agent(feat, occ, affine_row, grid_f64=True, crop=None, out=None):
    """K5 split, rank-local half: feat [C,H,W], occ [1,H,W] -> (feat_ego [C,H,W], score_ego [1,H,W]).
    out = (feat_ego, score_ego): contiguous fp32 destinations to write into (the agent's row of the exchange buffer)."""
    feat = _need(feat, torch.float32, "feat")
    occ = _need(occ, torch.float32, "occ")
    C, H, W = (int(v) for v in feat.shape[-3:])
    if out is not None:
        feat_ego, score_ego = out
        if not (feat_ego.is_contiguous() and score_ego.is_contiguous() and feat_ego.dtype == score_ego.dtype == torch.float32
                and feat_ego.numel() == C * H * W and score_ego.numel() == H * W and feat_ego.is_cuda):
            raise _capi.HealAmdError("warp_agent: `out` must be contiguous fp32 CUDA tensors of C*H*W and H*W elements")
    else:
        feat_ego = torch.empty((C, H, W), dtype=torch.float32, device=feat.device)
        score_ego = torch.empty((1, H, W), dtype=torch.float32, device=feat.device)
    a, ap, adev = _affine_args(affine_row, 1)
    c, cp = _crop_host(crop, 1)
    _capi.call("heal_warp_agent", _ptr(feat), _ptr(occ), C, H, W, ap, adev, int(bool(grid_f64)), cp,
               _ptr(feat_ego), _ptr(score_ego), _stream())
    return feat_ego, score_ego


def warp_agents_pm(feats, affine_rows, grid_f64=True):
    """warp_affine_simple + permute(0, 2, 3, 1) for one scene: feats [n,C,H,W] -> ego-frame maps, token-major [n,H,W,C]."""
    feats = _need(feats, torch.float32, "feats")
    n, C, H, W = (int(v) for v in feats.shape)
    out = torch.empty((n, H, W, C), dtype=torch.float32, device=feats.device)
    a, ap, adev = _affine_args(affine_rows, n)
    with _Timed("warp_agents_pm", 0.0, 8.0 * n * C * H * W):
        _capi.call("heal_warp_agents_pm", _ptr(feats), n, C, H, W, ap, adev, int(bool(grid_f64)), _ptr(out), _stream())
    return out


def fuse_warped_rows(base, feat_offsets, score_offsets, C, H, W):
    """K5 split, post-exchange half on the exchange buffer IN PLACE: agent a's [C,H,W] features at base.flatten()[feat_offsets[a]:],
    scores at score_offsets[a] (element offsets, multiples of 4) -> [C,H,W].  No re-pack of the gathered rows."""
    base = _need(base, torch.float32, "base")
    n = len(feat_offsets)
    out = torch.empty((C, H, W), dtype=torch.float32, device=base.device)
    _capi.call("heal_fuse_warped_rows", _ptr(base), _host_array([int(v) for v in feat_offsets], ctypes.c_int64),
               _host_array([int(v) for v in score_offsets], ctypes.c_int64), n, int(C), int(H), int(W), _ptr(out), _stream())
    return out


def fuse_warped(feats_ego, scores_ego):
    """K5 split, post-all-gather half: [n,C,H,W], [n,1,H,W] -> [C,H,W]."""
    feats_ego = _need(feats_ego, torch.float32, "feats_ego")
    scores_ego = _need(scores_ego, torch.float32, "scores_ego")
    n, C, H, W = (int(v) for v in feats_ego.shape)
    out = torch.empty((C, H, W), dtype=torch.float32, device=feats_ego.device)
    _capi.call("heal_fuse_warped", _ptr(feats_ego), _ptr(scores_ego), n, C, H, W, _ptr(out), _stream())
    return out


def decode_nms(cls, reg, dirp, anchors, score_thr, dir_offset, num_bins, nms_thr, tfm, gt_range,
               nms_top=1000, sync=True):
    """K8.  cls [1,A,H,W], reg [1,7A,H,W], dirp [1,bins*A,H,W] or None, anchors [H,W,A,7] f32 cuda.
    -> (corners [K,8,3], scores [K]) or (None, None) when nothing survives (sync=True), or the
    full-capacity buffers plus the device count (sync=False)."""
    cls = _need(cls, torch.float32, "cls_preds")
    reg = _need(reg, torch.float32, "reg_preds")
    anchors = _need(anchors, torch.float32, "anchors")
    if dirp is not None:
        dirp = _need(dirp, torch.float32, "dir_preds")
    if cls.dim() == 4:
        if cls.shape[0] != 1:
            raise _capi.HealAmdError("decode_nms: batch size must be 1 (voxel_postprocessor.py:314)")
        cls, reg = cls[0], reg[0]
        dirp = dirp[0] if dirp is not None else None
    A, H, W = (int(v) for v in cls.shape)
    if anchors.numel() != H * W * A * 7:
        raise _capi.HealAmdError(f"decode_nms: anchors {tuple(anchors.shape)} do not match the {A} x {H} x {W} score map "
                                 "(anchor_args.feature_stride of the YAML vs. the model's output stride)")
    dev = cls.device
    out_c = torch.empty((nms_top, 8, 3), dtype=torch.float32, device=dev)
    out_s = torch.empty((nms_top,), dtype=torch.float32, device=dev)
    out_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    nbytes = _capi.query("heal_decode_nms_workspace", A * H * W, int(nms_top))
    ws = _workspace("decode_nms", nbytes, dev)
    t = _host_array([float(v) for v in np.asarray(tfm, dtype=np.float32).reshape(-1)], ctypes.c_float)
    g = _host_array([float(v) for v in gt_range], ctypes.c_float)
    with _Timed("decode_nms"):
        _capi.call("heal_decode_nms", _ptr(cls), _ptr(reg), _ptr(dirp), _ptr(anchors), H, W, A, int(num_bins),
                   float(score_thr), float(dir_offset), float(nms_thr), int(nms_top), t, g,
                   _ptr(out_c), _ptr(out_s), _ptr(out_n), int(nms_top), _ptr(ws), ws.numel(), _stream())
    _remember("decode_nms", lambda: decode_nms(cls, reg, dirp, anchors, score_thr, dir_offset, num_bins, nms_thr, tfm, gt_range,
                                               nms_top, sync=False))
    if not sync:
        return out_c, out_s, out_n
    k = int(out_n.item())
    if _SPARSE_CHECKS and not torch.cuda.is_current_stream_capturing():
        verify_sparse_capacity()   # first host sync after a no-sync SECOND encoder: its capacity counters are final now
    if k == 0:
        return None, None
    return out_c[:k], out_s[:k]


DECODE_MAX_AGENTS = _limit("HEAL_DECODE_MAX_AGENTS")


def decode_nms_agents(cls_list, reg_list, dir_list, anchors_list, tfms, score_thr, dir_offset, num_bins, nms_thr, gt_range,
                      nms_top=1000, sync=True, want_agent=False):
    """K8 for late fusion (heal_decode_nms_agents; voxel_postprocessor.py:277-405 with several cavs): the candidates of every
    agent decoded with its own cav -> ego matrix, pooled in agent order, one rotated NMS over the top `nms_top` of the pool.
    Per agent k: cls [1,A,H_k,W_k] or [A,H_k,W_k], reg [.,7A,H_k,W_k], dir [.,bins*A,H_k,W_k] (dir_list None: no direction
    head), anchors [H_k,W_k,A,7], all f32 cuda; contiguous views into a batched head output are read in place.
    tfms: an [n,4,4] CUDA tensor (read on the device at run time: a captured graph follows the loaded frame's poses; f64 is
    cast on the device), a list of n CUDA 4x4 tensors (stacked on the device), or a host array / list of n 4x4 matrices; a list
    that mixes the two is refused.
    -> sync=True: (corners [K,8,3], scores [K]) or (None, None); sync=False: the full-capacity buffers and the device count,
    no host synchronisation.  want_agent appends the source agent of every kept box (int32)."""
    return _decode_nms_agents("decode_nms_agents", cls_list, reg_list, dir_list, anchors_list, None, tfms, score_thr, dir_offset,
                              num_bins, nms_thr, gt_range, nms_top, sync, want_agent, False)


def decode_nms_agents_unc(cls_list, reg_list, dir_list, anchors_list, unc_list, tfms, score_thr, dir_offset, num_bins, nms_thr,
                          gt_range, nms_top=1000, sync=True, want_agent=False, want_index=False):
    """decode_nms_agents for the uncertainty detector (heal_decode_nms_agents_unc; uncertainty_voxel_postprocessor.py:116-249):
    the same arguments plus unc_list, agent k's [1,dim*A,H_k,W_k] or [dim*A,H_k,W_k] uncertainty map.  Corners, scores and count
    are decode_nms_agents' bit for bit; every kept box also gets the `dim` uncertainty channels of the anchor it was decoded from.
    -> sync=True: (corners [K,8,3], scores [K], uncertainty [K,dim][, agent [K]][, index [K]]) or Nones; sync=False: the
    full-capacity buffers (corners, scores, count, uncertainty[, agent][, index]), no host synchronisation.  want_index appends
    the pooled anchor index of every kept box (int32: agent k's anchors start at sum_{u<k} H_u W_u A)."""
    return _decode_nms_agents("decode_nms_agents_unc", cls_list, reg_list, dir_list, anchors_list, unc_list, tfms, score_thr,
                              dir_offset, num_bins, nms_thr, gt_range, nms_top, sync, want_agent, want_index)


def _decode_nms_agents(who, cls_list, reg_list, dir_list, anchors_list, unc_list, tfms, score_thr, dir_offset, num_bins, nms_thr,
                       gt_range, nms_top, sync, want_agent, want_index):
    n = len(cls_list)
    if not 1 <= n <= DECODE_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: 1..{DECODE_MAX_AGENTS} agents per scene (got {n})")
    if len(reg_list) != n or len(anchors_list) != n or (dir_list is not None and len(dir_list) != n):
        raise _capi.HealAmdError(f"{who}: {n} score maps, {len(reg_list)} regression maps, "
                                 f"{'no' if dir_list is None else len(dir_list)} direction maps, {len(anchors_list)} anchor tables")
    if unc_list is not None and len(unc_list) != n:
        raise _capi.HealAmdError(f"{who}: {n} score maps, {len(unc_list)} uncertainty maps")
    if tfms is None:
        raise _capi.HealAmdError(f"{who}: tfms is required (an [n,4,4] CUDA tensor or {n} host matrices)")

    def maps(t, name, k):
        t = _need(t, torch.float32, f"{name}[{k}]")
        if t.dim() == 4:
            if t.shape[0] != 1:
                raise _capi.HealAmdError(f"{who}: batch size must be 1 per agent (voxel_postprocessor.py:314)")
            t = t[0]
        if t.dim() != 3:
            raise _capi.HealAmdError(f"{who}: {name}[{k}] must be [1,C,H,W] or [C,H,W], got {tuple(t.shape)}")
        return t

    cls_list = [maps(t, "cls_preds", k) for k, t in enumerate(cls_list)]
    reg_list = [maps(t, "reg_preds", k) for k, t in enumerate(reg_list)]
    if dir_list is not None:
        dir_list = [maps(t, "dir_preds", k) for k, t in enumerate(dir_list)]
    anchors_list = [_need(a, torch.float32, f"anchors[{k}]") for k, a in enumerate(anchors_list)]
    A = int(cls_list[0].shape[0])
    unc_dim = 0
    if unc_list is not None:
        unc_list = [maps(t, "unc_preds", k) for k, t in enumerate(unc_list)]
        unc_dim = int(unc_list[0].shape[0]) // A
        if unc_dim < 1 or any(tuple(u.shape) != (unc_dim * A,) + tuple(c.shape[1:]) for u, c in zip(unc_list, cls_list)):
            raise _capi.HealAmdError(f"{who}: uncertainty maps {[tuple(u.shape) for u in unc_list]} are not [dim * {A}, H_k, W_k] "
                                     "with one dim for every agent")
    hs, ws_, total = [], [], 0
    for k in range(n):
        Ak, H, W = (int(v) for v in cls_list[k].shape)
        if Ak != A:
            raise _capi.HealAmdError(f"{who}: agent {k} has {Ak} anchors per cell, agent 0 has {A}")
        if tuple(reg_list[k].shape) != (7 * A, H, W) or (dir_list is not None
                                                          and tuple(dir_list[k].shape) != (int(num_bins) * A, H, W)):
            raise _capi.HealAmdError(f"{who}: agent {k}: regression / direction maps do not match the {A} x {H} x {W} score map")
        if anchors_list[k].numel() != H * W * A * 7:
            raise _capi.HealAmdError(f"{who}: anchors {tuple(anchors_list[k].shape)} of agent {k} do not match the {A} x {H} x {W} "
                                     "score map (anchor_args.feature_stride of the YAML vs. the model's output stride)")
        hs.append(H)
        ws_.append(W)
        total += A * H * W
    if total >= 2 ** 31 - 256 * DECODE_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: {total} pooled anchors (must be below 2^31)")
    dev = cls_list[0].device
    null = ctypes.c_void_p(0)
    if isinstance(tfms, (list, tuple)):
        on_dev = [isinstance(m, torch.Tensor) and m.is_cuda for m in tfms]
        if tfms and all(on_dev):
            tfms = torch.stack([m.detach() for m in tfms])
        elif any(on_dev):      # copying some of them to the host would synchronise, which sync=False promises not to do
            raise _capi.HealAmdError(f"{who}: tfms mixes CUDA tensors and host matrices; give all {n} on one side")
    if isinstance(tfms, torch.Tensor) and tfms.is_cuda:
        t = tfms.detach()
        if tuple(t.shape) != (n, 4, 4):
            raise _capi.HealAmdError(f"{who}: tfms must be [{n},4,4], got {tuple(tfms.shape)}")
        t = t.to(torch.float32).contiguous()
        t_host, t_dev = null, _ptr(t)
    else:
        if isinstance(tfms, (list, tuple)):
            tfms = [m.detach().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in tfms]
        elif isinstance(tfms, torch.Tensor):
            tfms = tfms.detach().numpy()
        t = np.ascontiguousarray(np.asarray(tfms, dtype=np.float32))
        if t.shape != (n, 4, 4):
            raise _capi.HealAmdError(f"{who}: tfms must be {n} 4x4 matrices, got {t.shape}")
        t_host, t_dev = t.ctypes.data_as(ctypes.c_void_p), null
    out_c = torch.empty((nms_top, 8, 3), dtype=torch.float32, device=dev)
    out_s = torch.empty((nms_top,), dtype=torch.float32, device=dev)
    out_a = torch.empty((nms_top,), dtype=torch.int32, device=dev) if want_agent else None
    out_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    out_u = torch.empty((nms_top, unc_dim), dtype=torch.float32, device=dev) if unc_list is not None else None
    out_i = torch.empty((nms_top,), dtype=torch.int32, device=dev) if unc_list is not None and want_index else None
    entry = "heal_" + who
    nbytes = _capi.query(entry + "_workspace", total, int(nms_top))
    ws = _workspace(who, nbytes, dev)
    g = _host_array([float(v) for v in gt_range], ctypes.c_float)

    def ptrs(ts):
        return _host_array([x.data_ptr() for x in ts], ctypes.c_void_p)

    _capi.guard_note(entry, [x.data_ptr() for ts in (cls_list, reg_list, dir_list or [], anchors_list, unc_list or []) for x in ts])
    dir_ptrs = ptrs(dir_list) if dir_list is not None else null
    hs_c, ws_c = _host_array(hs, ctypes.c_int32), _host_array(ws_, ctypes.c_int32)
    with _Timed(who):
        if unc_list is None:
            _capi.call(entry, n, ptrs(cls_list), ptrs(reg_list), dir_ptrs, ptrs(anchors_list), hs_c, ws_c, A, int(num_bins),
                       float(score_thr), float(dir_offset), float(nms_thr), int(nms_top), t_host, t_dev, g,
                       _ptr(out_c), _ptr(out_s), _ptr(out_a), _ptr(out_n), int(nms_top), _ptr(ws), ws.numel(), _stream())
        else:
            _capi.call(entry, n, ptrs(cls_list), ptrs(reg_list), dir_ptrs, ptrs(anchors_list), ptrs(unc_list), hs_c, ws_c, A,
                       int(num_bins), unc_dim, float(score_thr), float(dir_offset), float(nms_thr), int(nms_top), t_host, t_dev, g,
                       _ptr(out_c), _ptr(out_s), _ptr(out_u), _ptr(out_a), _ptr(out_i), _ptr(out_n), int(nms_top), _ptr(ws),
                       ws.numel(), _stream())
    _remember(who, lambda: _decode_nms_agents(who, cls_list, reg_list, dir_list, anchors_list, unc_list, tfms, score_thr, dir_offset,
                                              num_bins, nms_thr, gt_range, nms_top, False, want_agent, want_index))
    extra = [t for t in (out_u, out_a, out_i) if t is not None]
    if not sync:
        return (out_c, out_s, out_n, *extra)
    k = int(out_n.item())
    if _SPARSE_CHECKS and not torch.cuda.is_current_stream_capturing():
        verify_sparse_capacity()   # as decode_nms: the first host sync after a no-sync SECOND encoder
    if k == 0:
        return (None,) * (2 + len(extra))
    return (out_c[:k], out_s[:k], *(t[:k] for t in extra))


def quad_iou(a, b):
    """Pairwise rotated IoU of quads a [n,4,2], b [m,4,2] (f32 cuda) -> [n,m]."""
    a = _need(a, torch.float32, "a")
    b = _need(b, torch.float32, "b")
    n, m = int(a.shape[0]), int(b.shape[0])
    out = torch.empty((n, m), dtype=torch.float32, device=a.device)
    _capi.call("heal_quad_iou", _ptr(a), n, _ptr(b), m, _ptr(out), _stream())
    return out


EVAL_MAX_DET, EVAL_MAX_GT, EVAL_MAX_THR = _limit("HEAL_EVAL_MAX_DET"), _limit("HEAL_EVAL_MAX_GT"), _limit("HEAL_EVAL_MAX_THR")


def eval_match_supported(n, m, n_thr):
    """The limits of heal_eval_match (capacities): n <= 1024 detections, m <= 256 ground-truth boxes, 1..8 thresholds."""
    return 0 <= int(n) <= EVAL_MAX_DET and 0 <= int(m) <= EVAL_MAX_GT and 1 <= int(n_thr) <= EVAL_MAX_THR


def _need_boxes(t, name, who):
    t = _need(t, torch.float32, name)
    if t.dim() != 3 or tuple(t.shape[1:]) not in ((8, 3), (4, 2)):
        raise _capi.HealAmdError(f"{who}: {name} must be [n,8,3] or [n,4,2], got {tuple(t.shape)}")
    return t, int(t.shape[1]) * int(t.shape[2])


def _need_count(t, name, who, dev):
    if t is None:
        return None
    t = _need(t, torch.int32, name)
    if t.numel() != 1 or t.device != dev:
        raise _capi.HealAmdError(f"{who}: {name} must be one int32 word on {dev}")
    return t


def eval_match(det, score, gt, thresholds, n_dev=None, m_dev=None, sync=True, want_gt_index=False, out=None):
    """AP evaluation of one frame (heal_eval_match; eval_utils.py:40-91 caluclate_tp_fp for every threshold at once): detections
    det [n,8,3] or [n,4,2] with score [n] against ground truth gt [m,8,3] or [m,4,2], all f32 cuda; thresholds: 1..8 floats,
    passed by value.  n_dev / m_dev (int32 [1] cuda): the live counts, read on the device; n / m are then capacities and the
    tails may hold anything -- decode_nms(sync=False)'s (corners, scores, count) are scored in place.
    -> (order [n] i32, tp [T,n] u8, score_sorted [n] f32[, gt_index [T,n] i32]) in descending-score order.  sync=True slices
    them to the live n (one host read of n_dev, none without it); sync=False returns the full-capacity buffers.
    out: the APPEND form -- a dict of persistent buffers order [cap] i32, tp [T,cap] u8, score [cap] f32, optionally gt_index
    [T,cap] i32, and the int32 words cursor, gt_total, overflow.  Rows go to offset `cursor`, which then advances by the live n
    (gt_total by the live m); a frame that does not fit sets `overflow` and writes nothing.  Never reads on the host; returns out."""
    who = "eval_match"
    det, det_f = _need_boxes(det, "det", who)
    gt, gt_f = _need_boxes(gt, "gt", who)
    score = _need(score, torch.float32, "score")
    n, m = int(det.shape[0]), int(gt.shape[0])
    thr = [float(v) for v in thresholds]
    T = len(thr)
    if score.numel() != n:
        raise _capi.HealAmdError(f"{who}: {score.numel()} scores for {n} detections")
    if not eval_match_supported(n, m, T):
        raise _capi.HealAmdError(f"{who}: {n} detections x {m} ground-truth boxes x {T} thresholds exceeds the kernel's limits "
                                 f"({EVAL_MAX_DET} x {EVAL_MAX_GT} x 1..{EVAL_MAX_THR})")
    dev = det.device
    if gt.device != dev or score.device != dev:
        raise _capi.HealAmdError(f"{who}: det, score and gt must be on one device")
    n_dev = _need_count(n_dev, "n_dev", who, dev)
    m_dev = _need_count(m_dev, "m_dev", who, dev)
    null = ctypes.c_void_p(0)
    if out is None:
        order = torch.empty((n,), dtype=torch.int32, device=dev)
        tp = torch.empty((T, n), dtype=torch.uint8, device=dev)
        sorted_score = torch.empty((n,), dtype=torch.float32, device=dev)
        gi = torch.empty((T, n), dtype=torch.int32, device=dev) if want_gt_index else None
        stride, cur, tot, ovf = n, null, null, null
    else:
        order, tp, sorted_score, gi = out["order"], out["tp"], out["score"], out.get("gt_index")
        stride = int(order.numel())
        for name, t, dt, shape in (("order", order, torch.int32, (stride,)), ("tp", tp, torch.uint8, (T, stride)),
                                   ("score", sorted_score, torch.float32, (stride,)), ("gt_index", gi, torch.int32, (T, stride)),
                                   ("cursor", out["cursor"], torch.int32, None), ("gt_total", out["gt_total"], torch.int32, None),
                                   ("overflow", out["overflow"], torch.int32, None)):
            if t is None and name == "gt_index":
                continue
            if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or not t.is_contiguous()
                    or (tuple(t.shape) != shape if shape is not None else t.numel() != 1)):
                raise _capi.HealAmdError(f"{who}: out['{name}'] must be a contiguous {dt} tensor on {dev}"
                                         + (f" of shape {shape}" if shape is not None else " of one element"))
        cur, tot, ovf = _ptr(out["cursor"]), _ptr(out["gt_total"]), _ptr(out["overflow"])
    nbytes = _capi.query("heal_eval_match_workspace", n, m)
    ws = _workspace("eval_match", nbytes, dev)
    with _Timed("eval_match"):
        _capi.call("heal_eval_match", _ptr(det), det_f, n, _ptr(n_dev), _ptr(score), _ptr(gt), gt_f, m, _ptr(m_dev),
                   _host_array(thr, ctypes.c_float), T, _ptr(order), _ptr(tp), _ptr(gi), _ptr(sorted_score), stride,
                   cur, tot, ovf, _ptr(ws), ws.numel(), _stream())
    if out is not None:
        return out
    if sync and n_dev is not None:
        k = max(0, min(int(n_dev.item()), n))
        order, tp, sorted_score = order[:k], tp[:, :k], sorted_score[:k]
        gi = gi[:, :k] if gi is not None else None
    return (order, tp, sorted_score, gi) if want_gt_index else (order, tp, sorted_score)


_WINDOW_ATTN_SHAPES = {(4, 16), (8, 32), (16, 64), (4, 32), (8, 16), (8, 64), (4, 64)}


def window_attention_supported(window, dim_head, H, W):
    return (int(window), int(dim_head)) in _WINDOW_ATTN_SHAPES and H % window == 0 and W % window == 0


def window_attention(qkv, pos_bias, heads, dim_head, window, scale, out=None):
    """Fused window attention: qkv [L,H,W,3*heads*dim_head] (packed q|k|v), pos_bias [T,T] or None -> [L,H,W,heads*dim_head]
    (written into `out` when given: a contiguous [L,H,W,heads*dim_head] view)."""
    qkv = _need(qkv, torch.float32, "qkv")
    L, H, W, C3 = (int(v) for v in qkv.shape)
    if C3 != 3 * heads * dim_head or not window_attention_supported(window, dim_head, H, W):
        raise _capi.HealAmdError(f"window_attention: unsupported shape (window {window}, dim_head {dim_head}, map {H}x{W})")
    if pos_bias is not None:
        pos_bias = _need(pos_bias, torch.float32, "pos_bias")
        if tuple(pos_bias.shape) != (window * window, window * window):
            raise _capi.HealAmdError("window_attention: pos_bias must be [window^2, window^2]")
    if out is None:
        out = torch.empty((L, H, W, heads * dim_head), dtype=torch.float32, device=qkv.device)
    elif not (out.is_contiguous() and out.numel() == L * H * W * heads * dim_head and out.dtype == torch.float32):
        raise _capi.HealAmdError("window_attention: `out` must be a contiguous f32 [L,H,W,heads*dim_head] buffer")
    # per token: q k^T and p v = 4 window^2 inner FLOPs; q | k | v read + the result written = 16 inner bytes
    inner = heads * dim_head
    with _Timed(f"window_attention_ws{window}", flops=4.0 * L * H * W * window * window * inner, nbytes=16.0 * L * H * W * inner):
        _capi.call("heal_window_attention", _ptr(qkv), _optr(pos_bias), L, H, W, int(heads), int(dim_head), int(window),
                   float(scale), _ptr(out), _stream())
    return out


def window_attention_backward(qkv, pos_bias, out, grad_out, heads, dim_head, window, scale, grad_qkv=None):
    """Backward of window_attention -> (grad_qkv like qkv, grad_bias [T,T] | None); `out` is the forward's result.  grad_qkv is
    written into the caller's buffer when given.  Unmeasured so far: the modules use it only under HEAL_WATTN_GRAD=kernel."""
    who = "window_attention_backward"
    qkv = _need(qkv, torch.float32, "qkv"); out = _need(out, torch.float32, "out"); grad_out = _need(grad_out, torch.float32, "grad_out")
    if qkv.dim() != 4:
        raise _capi.HealAmdError(f"{who}: qkv must be [L,H,W,3*heads*dim_head], got {tuple(qkv.shape)}")
    L, H, W, C3 = (int(v) for v in qkv.shape)
    if C3 != 3 * heads * dim_head or not window_attention_supported(window, dim_head, H, W):
        raise _capi.HealAmdError(f"{who}: unsupported shape (window {window}, dim_head {dim_head}, map {H}x{W})")
    # the kernels read a [L,H,W,heads*dim_head] row per token of `out` and `grad_out`, and window^4 bias words, from bare pointers
    for name, t in (("out", out), ("grad_out", grad_out)):
        if tuple(t.shape) != (L, H, W, heads * dim_head):
            raise _capi.HealAmdError(f"{who}: {name} has shape {tuple(t.shape)}, want {(L, H, W, heads * dim_head)}")
    grad_qkv = _out_or_empty(grad_qkv, tuple(qkv.shape), qkv.device, who)
    grad_bias = None
    if pos_bias is not None:
        pos_bias = _need(pos_bias, torch.float32, "pos_bias")
        if tuple(pos_bias.shape) != (window * window, window * window):
            raise _capi.HealAmdError(f"{who}: pos_bias must be [window^2, window^2], got {tuple(pos_bias.shape)}")
        grad_bias = torch.zeros_like(pos_bias)
    need = _capi.query("heal_window_attention_backward_workspace", L, H, W, int(heads))
    ws = _workspace("window_attention_bwd", need, qkv.device)
    _capi.call("heal_window_attention_backward", _ptr(qkv), _optr(pos_bias), _ptr(out), _ptr(grad_out), L, H, W, int(heads),
               int(dim_head), int(window), float(scale), _ptr(grad_qkv), _optr(grad_bias), _ptr(ws), need, _stream())
    return grad_qkv, grad_bias


class WindowAttention(torch.autograd.Function):
    """window_attention under autograd: forward = K6b, backward = heal_window_attention_backward (saves qkv, the bias table and
    the output; the T x T probabilities are recomputed per window)."""

    @staticmethod
    def forward(ctx, qkv, pos_bias, heads, dim_head, window, scale):
        qkv = qkv.contiguous()
        out = window_attention(qkv, pos_bias, heads, dim_head, window, scale)
        ctx.save_for_backward(qkv, pos_bias, out)
        ctx.cfg = (int(heads), int(dim_head), int(window), float(scale))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, pos_bias, out = ctx.saved_tensors
        heads, dim_head, window, scale = ctx.cfg
        gq, gb = window_attention_backward(qkv, pos_bias, out, grad_out.contiguous(), heads, dim_head, window, scale)
        return gq, gb, None, None, None, None


_AGENT_WINDOW_MODES = {"window": 0, "grid": 1}
AGENT_WINDOW_MAX_AGENTS = _limit("HEAL_AGENT_WINDOW_MAX_AGENTS")


def agent_window_attention_supported(n_agents, window, dim_head, H, W):
    return (1 <= int(n_agents) <= AGENT_WINDOW_MAX_AGENTS and int(window) == 4 and int(dim_head) == 32 and H % window == 0
            and W % window == 0)


def agent_window_attention(qkv, bias, n_valid, mode, heads, dim_head, window, scale, out=None):
    """CoBEVT's masked attention over agents x window pixels (heal_agent_window_attention): qkv [L,H,W,3*heads*dim_head] (packed
    q|k|v, token-major), bias [heads,T,T] (T = L window^2, token order (l w1 w2)) or None, n_valid: agents >= n_valid are masked
    keys, mode 'window' | 'grid' -> [L,H,W,heads*dim_head] (written into `out` when given)."""
    qkv = _need(qkv, torch.float32, "qkv")
    if qkv.dim() != 4:
        raise _capi.HealAmdError("agent_window_attention: qkv must be [L,H,W,3*heads*dim_head]")
    L, H, W, C3 = (int(v) for v in qkv.shape)
    if mode not in _AGENT_WINDOW_MODES:
        raise _capi.HealAmdError(f"agent_window_attention: mode must be 'window' or 'grid', got {mode!r}")
    if C3 != 3 * heads * dim_head or not agent_window_attention_supported(L, window, dim_head, H, W):
        raise _capi.HealAmdError(f"agent_window_attention: unsupported shape ({L} agents, window {window}, dim_head {dim_head}, "
                                 f"map {H}x{W})")
    n_valid = int(n_valid)
    if not 1 <= n_valid <= L:
        raise _capi.HealAmdError(f"agent_window_attention: n_valid {n_valid} outside 1..{L}")
    T = L * window * window
    if bias is not None:
        bias = _need(bias, torch.float32, "bias")
        if tuple(bias.shape) != (heads, T, T):
            raise _capi.HealAmdError(f"agent_window_attention: bias must be [heads, T, T] = [{heads}, {T}, {T}]")
    inner = heads * dim_head
    out = _out_like(out, (L, H, W, inner), qkv.device, "agent_window_attention")
    # per query token: q k^T and p v over the n_valid * window^2 unmasked keys = 4 n_valid window^2 inner FLOPs; q | k | v read +
    # the result written = 16 inner bytes
    with _Timed(f"agent_window_attention_{mode}", flops=4.0 * L * H * W * n_valid * window * window * inner,
                nbytes=16.0 * L * H * W * inner):
        _capi.call("heal_agent_window_attention", _ptr(qkv), _optr(bias), L, n_valid, H, W, int(heads), int(dim_head),
                   int(window), _AGENT_WINDOW_MODES[mode], float(scale), _ptr(out), _stream())
    return out


def agent_window_attention_train_supported(n_agents, window, dim_head, H, W):
    """The shapes heal_agent_window_attention_backward takes (the forward's): the device gradient path of agent_window_attention
    (ops.AgentWindowAttention) for fp32 CUDA tensors."""
    return bool(agent_window_attention_supported(n_agents, window, dim_head, H, W)
                and _capi.lib().heal_agent_window_attention_backward_supported(int(n_agents), int(window), int(dim_head), int(H), int(W)))


def agent_window_attention_backward(qkv, bias, grad_out, n_valid, mode, heads, dim_head, window, scale, parts=None,
                                    grad_qkv=None, grad_bias=None):
    """Backward of agent_window_attention (heal_agent_window_attention_backward): qkv / bias / n_valid / mode as in the forward,
    grad_out like the forward's result -> (grad_qkv like qkv, grad_bias [heads,T,T] | None).  The forward's result itself is not
    needed: the kernel recomputes the probabilities and forms the softmax gradient's row term from them.  Masked agents' dK / dV
    rows and grad_bias columns are exact zeros.  parts: into how many ranges the groups are cut for the deterministic grad_bias sum
    (None: the library's policy).  grad_qkv / grad_bias: optional destinations (contiguous fp32 tensors of those shapes on qkv's
    device; grad_bias only together with a bias), checked before anything is launched."""
    who = "agent_window_attention_backward"
    qkv = _need(qkv, torch.float32, "qkv"); grad_out = _need(grad_out, torch.float32, "grad_out")
    if qkv.dim() != 4:
        raise _capi.HealAmdError(f"{who}: qkv must be [L,H,W,3*heads*dim_head]")
    L, H, W, C3 = (int(v) for v in qkv.shape)
    if mode not in _AGENT_WINDOW_MODES:
        raise _capi.HealAmdError(f"{who}: mode must be 'window' or 'grid', got {mode!r}")
    if C3 != 3 * heads * dim_head or not agent_window_attention_train_supported(L, window, dim_head, H, W):
        raise _capi.HealAmdError(f"{who}: unsupported shape ({L} agents, window {window}, dim_head {dim_head}, map {H}x{W})")
    inner = heads * dim_head
    if tuple(grad_out.shape) != (L, H, W, inner):
        raise _capi.HealAmdError(f"{who}: grad_out must be [L,H,W,heads*dim_head] = [{L}, {H}, {W}, {inner}]")
    if grad_out.device != qkv.device:
        raise _capi.HealAmdError(f"{who}: qkv and grad_out must be on one device")
    n_valid = int(n_valid)
    if not 1 <= n_valid <= L:
        raise _capi.HealAmdError(f"{who}: n_valid {n_valid} outside 1..{L}")
    T = L * window * window
    G = (H // window) * (W // window)
    parts = 0 if parts is None else int(parts)
    if parts and not 1 <= parts <= G:
        raise _capi.HealAmdError(f"{who}: parts {parts} outside 1..{G} (the groups)")
    ws, need = None, 0
    if bias is None and grad_bias is not None:
        raise _capi.HealAmdError(f"{who}: `grad_bias` goes with a bias")
    grad_qkv = _out_like(grad_qkv, (L, H, W, C3), qkv.device, who, "grad_qkv")
    if bias is not None:
        bias = _need(bias, torch.float32, "bias")
        if tuple(bias.shape) != (heads, T, T) or bias.device != qkv.device:
            raise _capi.HealAmdError(f"{who}: bias must be [heads, T, T] = [{heads}, {T}, {T}] on the device of qkv")
        grad_bias = _out_like(grad_bias, (heads, T, T), qkv.device, who, "grad_bias")
        need = _capi.query("heal_agent_window_attention_backward_workspace", L, H, W, int(heads), parts)
        ws = _workspace("agent_window_attention_bwd", need, qkv.device) if need else None
    # per query token: 7 products over the n_valid * window^2 unmasked keys (S and dP in both phases, dQ, dK, dV) = 14 n_valid
    # window^2 inner FLOPs; q | k | v and grad_out read + grad_qkv written = 28 inner bytes
    with _Timed(f"agent_window_attention_backward_{mode}", flops=14.0 * L * H * W * n_valid * window * window * inner,
                nbytes=28.0 * L * H * W * inner):
        _capi.call("heal_agent_window_attention_backward", _ptr(qkv), _optr(bias), _ptr(grad_out), L, n_valid, H, W,
                   int(heads), int(dim_head), int(window), _AGENT_WINDOW_MODES[mode], float(scale), parts, _ptr(grad_qkv),
                   _optr(grad_bias), _optr(ws), need, _stream())
    return grad_qkv, grad_bias


class AgentWindowAttention(torch.autograd.Function):
    """agent_window_attention under autograd: forward = heal_agent_window_attention, backward =
    heal_agent_window_attention_backward (saves qkv and the bias; the T x T probabilities are recomputed per group and the
    output is not needed again)."""

    @staticmethod
    def forward(ctx, qkv, bias, n_valid, mode, heads, dim_head, window, scale):
        qkv = qkv.contiguous()
        bias = bias.contiguous() if bias is not None else None
        out = agent_window_attention(qkv, bias, n_valid, mode, heads, dim_head, window, scale)
        ctx.save_for_backward(qkv, bias)
        ctx.cfg = (int(n_valid), mode, int(heads), int(dim_head), int(window), float(scale))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, bias = ctx.saved_tensors
        gq, gb = agent_window_attention_backward(qkv, bias, grad_out.contiguous(), *ctx.cfg)
        return gq, gb, None, None, None, None, None, None


def agent_mean(x):
    """x [L, ...] f32 -> mean over the first dimension [...] (heal_agent_mean; sums in agent order)."""
    x = _need(x, torch.float32, "x")
    L = int(x.shape[0])
    out = torch.empty(tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    n = out.numel()
    if n % 4:
        raise _capi.HealAmdError("agent_mean: the per-agent size must be a multiple of 4")
    with _Timed("agent_mean", nbytes=4.0 * (L + 1) * n):
        _capi.call("heal_agent_mean", _ptr(x), L, n, _ptr(out), _stream())
    return out


V2V_MAX_AGENTS = _limit("HEAL_V2V_MAX_AGENTS")


def v2v_message_tile_h(n_ego, cout, H, W, mode):
    """Output rows per heal_v2v_message block: 8 for the mean (2 waves per SIMD at 138 VGPRs), 4 for the max (its fold keeps E
    and a running maximum: 8 rows would leave one wave per SIMD); HEAL_V2V_TH overrides (4 | 8 | 16)."""
    return switches.number("HEAL_V2V_TH") or (4 if mode == 1 else 8)


def v2v_message_nsplit(n_ego, n_agents, cout, H, W, tile_h):
    """Agent-loop splits: 1 unless one launch has fewer blocks than two per CU (256 CUs): then enough splits for ~512 blocks, at
    most one per agent, none empty.  HEAL_V2V_SPLIT forces a value (clamped to [1, n_agents])."""
    blocks = n_ego * -(-cout // 64) * -(-W // 16) * -(-H // tile_h)
    want = switches.number("HEAL_V2V_SPLIT")
    if want is None:
        want = -(-512 // blocks) if blocks < 512 else 1
    want = max(1, min(want, n_agents))
    return -(-n_agents // -(-n_agents // want))       # no empty split


def v2v_message(xs, mask, e, w, residual=None, mode="mean", nsplit=None):
    """V2VNet's masked message aggregation (heal_v2v_message; fusion_in_one.py:266-294).  xs [n_ego, N, Cin, H, W] warped
    neighbour maps, mask [n_ego, N, H, W], e [n_ego, >= Cout, H, W] the ego term W_e * x + b (its first Cout channels are read:
    a slice of the stacked convolution), w [Cout, Cin, 3, 3] the neighbour half of msg_cnn's weight, residual [n_ego, Cout, H, W]
    or None; mode 'mean' | 'max' -> [n_ego, Cout, H, W]."""
    xs = _need(xs, torch.float32, "xs")
    mask = _need(mask, torch.float32, "mask")
    n_ego, N, cin, H, W = (int(v) for v in xs.shape)
    cout = int(w.shape[0])
    if tuple(w.shape) != (cout, cin, 3, 3) or mode not in ("mean", "max") or not 1 <= N <= V2V_MAX_AGENTS:
        raise _capi.HealAmdError(f"v2v_message: unsupported weight {tuple(w.shape)} / mode {mode} / {N} agents for xs "
                                 f"{tuple(xs.shape)} (3x3 weights, mean | max, 1..{V2V_MAX_AGENTS} agents)")
    if tuple(mask.shape) != (n_ego, N, H, W):
        raise _capi.HealAmdError(f"v2v_message: mask {tuple(mask.shape)} for xs {tuple(xs.shape)}")
    if not (isinstance(e, torch.Tensor) and e.is_cuda and e.dtype == torch.float32 and e.dim() == 4
            and int(e.shape[0]) == n_ego and int(e.shape[1]) >= cout and tuple(e.shape[2:]) == (H, W)
            and e.stride(3) == 1 and e.stride(2) == W and e.stride(1) == H * W):
        raise _capi.HealAmdError(f"v2v_message: e must be an f32 cuda [n_ego, >= {cout}, {H}, {W}] with contiguous channel planes")
    _need(e, torch.float32, "e")        # the autograd check (e is read in place: a channel slice is allowed)
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
        if tuple(residual.shape) != (n_ego, cout, H, W):
            raise _capi.HealAmdError("v2v_message: residual shape mismatch")
    m = 1 if mode == "max" else 0
    th = v2v_message_tile_h(n_ego, cout, H, W, m)
    ns = v2v_message_nsplit(n_ego, N, cout, H, W, th) if nsplit is None else int(nsplit)
    frag = conv3x3_fragments(w)
    out = torch.empty((n_ego, cout, H, W), dtype=torch.float32, device=xs.device)
    nbytes = _capi.query("heal_v2v_message_workspace", n_ego, cout, H, W, ns)
    ws = _workspace("v2v_message", nbytes, xs.device) if nbytes else None
    with _Timed(f"v2v_message_{cin}_{cout}", 2.0 * 9 * n_ego * N * cin * cout * H * W,
                4.0 * n_ego * (N * (cin + 1) * H * W + 2 * cout * H * W), kernel_events=True):
        _capi.call("heal_v2v_message", _ptr(xs), _ptr(mask), _ptr(e), int(e.stride(0)), _ptr(frag), _optr(residual), n_ego, N,
                   cin, cout, H, W, m, ns, th, _ptr(out), _optr(ws), 0 if ws is None else ws.numel(), _stream())
    return out


def gru_zero_state(gates, add=None):
    """ConvGRU cell with a zero hidden state (heal_gru_zero_state; convgru.py:52-72): gates [n, >= 2C, H, W] (u | c channel
    blocks, images gates.stride(0) apart), add None or the same layout (added to both blocks) -> h = sigmoid(u) tanh(c) [n, C, H, W].
    C = gates.shape[1] // 2 unless add is given, then both hold exactly 2C channels."""
    def check(t, name):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4
                and t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(1) == t.shape[2] * t.shape[3]):
            raise _capi.HealAmdError(f"gru_zero_state: {name} must be an f32 cuda [n, 2C, H, W] with contiguous channel planes")
        _need(t, torch.float32, name)
    check(gates, "gates")
    n, c2, H, W = (int(v) for v in gates.shape)
    if c2 % 2:
        raise _capi.HealAmdError(f"gru_zero_state: gates has {c2} channels (u | c: an even count)")
    C = c2 // 2
    if add is not None:
        check(add, "add")
        if int(add.shape[0]) != n or int(add.shape[1]) < c2 or tuple(add.shape[2:]) != (H, W):
            raise _capi.HealAmdError(f"gru_zero_state: add {tuple(add.shape)} for gates {tuple(gates.shape)}")
    h = torch.empty((n, C, H, W), dtype=torch.float32, device=gates.device)
    with _Timed("gru_zero_state", nbytes=4.0 * n * C * H * W * (3 + (2 if add is not None else 0))):
        _capi.call("heal_gru_zero_state", _ptr(gates), int(gates.stride(0)), _optr(add), 0 if add is None else int(add.stride(0)),
                   n, C, H, W, _ptr(h), _stream())
    return h


def label_assign(anchor_boxes, gt_boxes, pos_threshold, neg_threshold):
    """Anchor labelling core of generate_label: stand-up boxes [N,4] / [G,4] f32 cuda -> (assigned [N] i32: gt index of a
    positive anchor or -1, neg [N] u8)."""
    a = _need(anchor_boxes, torch.float32, "anchor_boxes")
    g = _need(gt_boxes, torch.float32, "gt_boxes")
    if a.dim() != 2 or a.shape[1] != 4 or g.dim() != 2 or g.shape[1] != 4:
        raise _capi.HealAmdError("label_assign: boxes must be [n,4]")
    n, k = int(a.shape[0]), int(g.shape[0])
    assigned = torch.empty((n,), dtype=torch.int32, device=a.device)
    neg = torch.empty((n,), dtype=torch.uint8, device=a.device)
    need = _capi.query("heal_label_assign_workspace", k)
    ws = _workspace("label_assign", need, a.device)
    _capi.call("heal_label_assign", _ptr(a), n, _ptr(g) if k else None, k, float(pos_threshold), float(neg_threshold),
               _ptr(assigned), _ptr(neg), _ptr(ws), need, _stream())
    return assigned, neg


_BEV_MODES = {"overlap": 0, "iou": 1, "iou_normal": 2}


def boxes_bev_matrix(boxes_a, boxes_b, mode="iou"):
    """pcdet BEV box ops: boxes [n,7] / [m,7] f32 cuda (x, y, z, dx, dy, dz, heading) -> [n,m] overlap area
    ('overlap'), rotated IoU ('iou') or axis-aligned IoU ('iou_normal')."""
    a = _need(boxes_a, torch.float32, "boxes_a")
    b = _need(boxes_b, torch.float32, "boxes_b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != 7 or b.shape[1] != 7:
        raise _capi.HealAmdError("boxes_bev_matrix: boxes must be [n,7]")
    n, m = int(a.shape[0]), int(b.shape[0])
    out = torch.zeros((n, m), dtype=torch.float32, device=a.device)
    _capi.call("heal_boxes_bev_matrix", _ptr(a), n, _ptr(b), m, _BEV_MODES[mode], _ptr(out), _stream())
    return out


def nms_bev(boxes_sorted, thresh, rotated=True):
    """Greedy pcdet NMS over boxes [n,7] already in descending-score order -> (keep [n] i64, count [1] i32), both on
    the device; keep[:count] are the surviving indices in ascending order."""
    b = _need(boxes_sorted, torch.float32, "boxes_sorted")
    if b.dim() != 2 or b.shape[1] != 7:
        raise _capi.HealAmdError("nms_bev: boxes must be [n,7]")
    n = int(b.shape[0])
    keep = torch.empty((n,), dtype=torch.int64, device=b.device)
    count = torch.zeros((1,), dtype=torch.int32, device=b.device)
    need = _capi.query("heal_nms_bev_workspace", n)
    ws = _workspace("nms_bev", need, b.device)
    _capi.call("heal_nms_bev", _ptr(b), n, float(thresh), int(bool(rotated)), _ptr(ws), need, _ptr(keep), _ptr(count),
               _stream())
    return keep, count


def camera_matrices(rots, trans, intrins, post_rots, post_trans):
    """[B,N,3,3] / [B,N,3] device tensors -> cam_mats [B*N,27] f32 (rots @ inv(intrins) | inv(post_rots) | post_trans |
    trans | 0): the 3x3 algebra of get_geometry in one launch."""
    f = lambda t, name: _need(t.float() if t.dtype != torch.float32 else t, torch.float32, name)
    rots, trans, intrins = f(rots, "rots"), f(trans, "trans"), f(intrins, "intrins")
    post_rots, post_trans = f(post_rots, "post_rots"), f(post_trans, "post_trans")
    n = int(trans.numel() // 3)
    if rots.numel() != 9 * n or intrins.numel() != 9 * n or post_rots.numel() != 9 * n or post_trans.numel() != 3 * n:
        raise _capi.HealAmdError("camera_matrices: inconsistent shapes")
    out = torch.empty((n, 27), dtype=torch.float32, device=trans.device)
    _capi.call("heal_camera_matrices", _ptr(rots), _ptr(trans), _ptr(intrins), _ptr(post_rots), _ptr(post_trans), n,
               _ptr(out), _stream())
    return out


def nms_quads(quads_sorted, thresh):
    """Greedy rotated NMS over quads [n,4,2] f32 cuda already in descending-score order -> (keep [n] i64, count [1] i32)
    on the device; keep[:count] are indices into the given order, in pick order."""
    q = _need(quads_sorted, torch.float32, "quads_sorted")
    if q.dim() != 3 or tuple(q.shape[1:]) != (4, 2):
        raise _capi.HealAmdError("nms_quads: quads must be [n,4,2]")
    n = int(q.shape[0])
    keep = torch.empty((n,), dtype=torch.int64, device=q.device)
    count = torch.zeros((1,), dtype=torch.int32, device=q.device)
    need = _capi.query("heal_nms_quads_workspace", n)
    ws = _workspace("nms_quads", need, q.device)
    _capi.call("heal_nms_quads", _ptr(q), n, float(thresh), _ptr(ws), need, _ptr(keep), _ptr(count), _stream())
    return keep, count


def _frustum_separable(frustum):
    """True if frustum[d][v][u] == (xs[u], ys[v], ds[d]) -- what create_frustum builds (heter_encoders.py:110-123) and what
    heal_bev_pool_pm assumes.  Checked once per tensor (a host sync; not during graph capture)."""
    if derived.capturing() and not derived.ready("frustum_separable", (frustum,)):
        raise _capi.HealAmdError("bev_pool: first use of a frustum tensor inside a graph capture (run one eager step first)")

    def build():
        D, fH, fW, _ = frustum.shape
        sep = torch.stack((frustum[0, 0, :, 0].view(1, 1, fW).expand(D, fH, fW),
                           frustum[0, :, 0, 1].view(1, fH, 1).expand(D, fH, fW),
                           frustum[:, 0, 0, 2].view(D, 1, 1).expand(D, fH, fW)), -1)
        return bool(torch.equal(sep, frustum))
    return _derived("frustum_separable", (frustum,), build)


def bev_pool_pm_supported(D, fH, C):
    mtot = (D + 15) // 16 * 16
    fh4 = (fH + 3) // 4 * 4
    lds = (fh4 * (C + 16) + 2 * mtot * 66) * 4   # LssLds, bev_pool.hip
    return (switches.get("HEAL_LSS_PATH") != "sorted" and fH <= 64 and D <= 64 and D % 4 == 0 and C % 16 == 0
            and 16 <= C <= 256 and lds <= 150 * 1024)


class PooledBEV:
    """The SPARSE PIXEL-MAJOR BEV map heal_bev_pool_scatter leaves in its workspace: rows[cell][C] for the cells any lifted point
    fell into + a generation-tagged flag per cell (include/heal_amd.h, K4).  It stands for the reference's dense
    [n_agents, C*nz, ny, nx] `voxel_pooling` result (heter_encoders.py:161-217) until somebody needs it:

      * `stem_block(...)` -- the first BasicBlock of the camera ResNetBEVBackbone reads the rows through the flags, the dense
        canvas is never written;
      * `dense()` -- everybody else gets the reference's tensor (one streaming launch).

    Exactly one of the two may be called, once: the consumer hands the workspace half back to the next scatter."""

    def __init__(self, ws, n_agents, channels, nx):
        self.ws, self.n_agents, self.channels, self.nx = ws, int(n_agents), int(channels), [int(v) for v in nx]
        self.device = ws.device
        self._consumed = False

    @property
    def shape(self):
        return (self.n_agents, self.channels * self.nx[2], self.nx[1], self.nx[0])

    @property
    def is_cuda(self):
        return True

    def _take(self):
        if self._consumed:
            raise _capi.HealAmdError("PooledBEV: the pooled map was already consumed (one consumer per bev_pool scatter)")
        self._consumed = True

    def dense(self):
        self._take()
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        with _Timed("bev_pool_emit"):
            _capi.call("heal_bev_pool_emit", self.n_agents, self.channels, _host_array(self.nx, ctypes.c_int32), _ptr(out),
                       _ptr(self.ws), self.ws.numel(), _stream())
        return out

    def stem_supported(self, cout_main, cout_down):
        return (self.nx[2] == 1 and self.channels % 32 == 0 and cout_main == 64 and cout_down == 64
                and ((self.nx[0] - 1) // 2 + 1) % 4 == 0)

    def stem_block(self, w_main, b_main, w_down, b_down):
        """relu(conv3x3_s2(x, W1) + b1), conv1x1_s2(x, Wd) + bd from the sparse map; w_main / w_down in the layouts of
        stem_fragments()."""
        self._take()
        Ho, Wo = (self.nx[1] - 1) // 2 + 1, (self.nx[0] - 1) // 2 + 1
        out_main = torch.empty((self.n_agents, 64, Ho, Wo), dtype=torch.float32, device=self.device)
        out_id = torch.empty_like(out_main)
        cin = self.channels
        flops = 2.0 * self.n_agents * Ho * Wo * 64 * cin * 10
        with _Timed("bev_stem_block", flops=flops, kernel_events=True):
            _capi.call("heal_bev_stem_block", self.n_agents, cin, _host_array(self.nx, ctypes.c_int32), _ptr(w_main),
                       _ptr(b_main), _ptr(w_down), _ptr(b_down), _ptr(out_main), _ptr(out_id), _ptr(self.ws), self.ws.numel(),
                       _stream())
        return out_main, out_id


def stem_fragments(w_main, w_down):
    """Weights of heal_bev_stem_block: w_main [64, C, 3, 3] -> [9][C/K][64][K] (tap = ky*3 + kx, K-channel chunk, cout,
    channel in chunk); w_down [64, C, 1, 1] -> [C/K][64][K]; K = 64 when C % 64 == 0, else 32."""
    co, c = int(w_main.shape[0]), int(w_main.shape[1])
    if co != 64 or c % 32 != 0 or tuple(w_main.shape[2:]) != (3, 3) or tuple(w_down.shape) != (64, c, 1, 1):
        raise _capi.HealAmdError("stem_fragments: expected [64, C, 3, 3] and [64, C, 1, 1] with C % 32 == 0")
    k = 64 if c % 64 == 0 else 32          # K chunk of k_bev_stem
    wm = w_main.detach().to(torch.float32).reshape(64, c // k, k, 9).permute(3, 1, 0, 2).contiguous()
    wd = w_down.detach().to(torch.float32).reshape(64, c // k, k).permute(1, 0, 2).contiguous()
    return wm, wd


def bev_pool_pm(head, C, D, fH, fW, frustum, cam_mats, n_agents, n_cams, dx, bx, nx, pooled=False):
    """K4, production path.  head [n_agents*n_cams, fH*fW, >= C + D] f32 cuda, PIXEL-MAJOR: per pixel the C image features
    followed by the D depth logits (what conv1x1(..., pixel_major=True) of the fused image_head | depth_head weight
    writes); frustum [D,fH,fW,3]; cam_mats [n_agents*n_cams,27] -> [n_agents, C*nz, ny, nx], or with pooled=True the
    PooledBEV hand-off (sparse pixel-major map; its consumer decides whether the dense tensor is ever written)."""
    head = _need(head, torch.float32, "head")
    frustum = _need(frustum, torch.float32, "frustum")
    cam_mats = _need(cam_mats, torch.float32, "cam_mats")
    BN, HW, CT = (int(v) for v in head.shape)
    if (BN != n_agents * n_cams or HW != fH * fW or CT < C + D or tuple(frustum.shape) != (D, fH, fW, 3)
            or tuple(cam_mats.shape) != (BN, 27)):
        raise _capi.HealAmdError("bev_pool_pm: inconsistent shapes")
    if not bev_pool_pm_supported(D, fH, C) or not _frustum_separable(frustum):
        raise _capi.HealAmdError("bev_pool_pm: shape / frustum outside the fused path (use bev_pool)")
    nxi = [int(v) for v in nx]
    dev = head.device
    nbytes = _capi.query("heal_bev_pool_pm_workspace", n_agents, C, nxi[0], nxi[1], nxi[2])
    # one scratch per problem shape: the two-half invariant holds for ONE carving of the buffer only
    ws = _workspace(("bev_pool_pm", n_agents, C, nxi[0], nxi[1], nxi[2]), nbytes, dev, zeroed=True)
    nbytes_alg = 4.0 * (BN * HW * (C + D)) + 4.0 * n_agents * C * nxi[0] * nxi[1] * nxi[2]
    with _Timed("bev_pool", nbytes=nbytes_alg, kernel_events=True):
        _capi.call("heal_bev_pool_scatter", _ptr(head), CT, _ptr(frustum), _ptr(cam_mats), n_agents, n_cams, D, fH, fW, C,
                   _host_array([float(v) for v in dx], ctypes.c_float),
                   _host_array([float(v) for v in bx], ctypes.c_float),
                   _host_array(nxi, ctypes.c_int32), _ptr(ws), ws.numel(), _stream())
    handle = PooledBEV(ws, n_agents, C, nxi)
    return handle if pooled else handle.dense()


def bev_pool_pm_multi(problems):
    """K4 for several independent problems in ONE launch (heal_bev_pool_scatter_multi): the camera agents of every camera modality of a
    scene.  problems: list of dicts with the arguments of bev_pool_pm (head, C, D, fH, fW, frustum, cam_mats, n_agents, n_cams, dx, bx,
    nx, pooled) -> list of PooledBEV | dense tensors in the same order."""
    if len(problems) == 1:
        return [bev_pool_pm(**problems[0])]
    dev = problems[0]["head"].device
    keep, wss, nbytes_alg = [], [], 0.0
    for i, q in enumerate(problems):
        head = _need(q["head"], torch.float32, "head")
        fr = _need(q["frustum"], torch.float32, "frustum")
        cm = _need(q["cam_mats"], torch.float32, "cam_mats")
        BN, HW, CT = (int(v) for v in head.shape)
        C, D, fH, fW = int(q["C"]), int(q["D"]), int(q["fH"]), int(q["fW"])
        if (BN != q["n_agents"] * q["n_cams"] or HW != fH * fW or CT < C + D or tuple(fr.shape) != (D, fH, fW, 3)
                or tuple(cm.shape) != (BN, 27)):
            raise _capi.HealAmdError("bev_pool_pm_multi: inconsistent shapes")
        if not bev_pool_pm_supported(D, fH, C) or not _frustum_separable(fr):
            raise _capi.HealAmdError("bev_pool_pm_multi: shape / frustum outside the fused path")
        nxi = [int(v) for v in q["nx"]]
        nb = _capi.query("heal_bev_pool_pm_workspace", int(q["n_agents"]), C, nxi[0], nxi[1], nxi[2])
        # one scratch per problem SLOT and shape: two problems of equal shape in one launch must not share rows / flags
        wss.append(_workspace(("bev_pool_pm", i, int(q["n_agents"]), C, nxi[0], nxi[1], nxi[2]), nb, dev, zeroed=True))
        keep.append((head, fr, cm, CT, nxi))
        nbytes_alg += 4.0 * (BN * HW * (C + D)) + 4.0 * q["n_agents"] * C * nxi[0] * nxi[1] * nxi[2]
    n = len(problems)
    PP = ctypes.c_void_p * n
    I32 = ctypes.c_int32 * n
    arr = lambda vals: I32(*[int(v) for v in vals])
    f3 = lambda key: (ctypes.c_float * (3 * n))(*[float(v) for q in problems for v in q[key]])
    with _Timed("bev_pool", nbytes=nbytes_alg, kernel_events=True):
        _capi.call("heal_bev_pool_scatter_multi", n,
                   ctypes.cast(PP(*[k[0].data_ptr() for k in keep]), ctypes.c_void_p), ctypes.cast(arr(k[3] for k in keep), ctypes.c_void_p),
                   ctypes.cast(PP(*[k[1].data_ptr() for k in keep]), ctypes.c_void_p), ctypes.cast(PP(*[k[2].data_ptr() for k in keep]), ctypes.c_void_p),
                   ctypes.cast(arr(q["n_agents"] for q in problems), ctypes.c_void_p), ctypes.cast(arr(q["n_cams"] for q in problems), ctypes.c_void_p),
                   ctypes.cast(arr(q["D"] for q in problems), ctypes.c_void_p), ctypes.cast(arr(q["fH"] for q in problems), ctypes.c_void_p),
                   ctypes.cast(arr(q["fW"] for q in problems), ctypes.c_void_p), ctypes.cast(arr(q["C"] for q in problems), ctypes.c_void_p),
                   ctypes.cast(f3("dx"), ctypes.c_void_p), ctypes.cast(f3("bx"), ctypes.c_void_p),
                   ctypes.cast((ctypes.c_int32 * (3 * n))(*[v for k in keep for v in k[4]]), ctypes.c_void_p),
                   ctypes.cast(PP(*[w.data_ptr() for w in wss]), ctypes.c_void_p),
                   ctypes.cast((ctypes.c_size_t * n)(*[w.numel() for w in wss]), ctypes.c_void_p), _stream())
    out = []
    for q, w, k in zip(problems, wss, keep):
        h = PooledBEV(w, q["n_agents"], q["C"], k[4])
        out.append(h if q.get("pooled") else h.dense())
    return out


def bev_pool(depth_logit, feat, frustum, cam_mats, n_agents, n_cams, dx, bx, nx):
    """K4 on the reference's NCHW tensors.  depth_logit [n_agents*n_cams,D,fH,fW], feat [n_agents*n_cams,C,fH,fW], frustum
    [D,fH,fW,3] (f32 cuda); cam_mats: f32 cuda [n_agents*n_cams,27] (combine 9, inv(post_rots) 9, post_trans 3,
    trans 3, pad 3); dx,bx host float[3], nx host int[3] -> [n_agents, C*nz, ny, nx].

    Shapes the fused path takes are re-laid pixel-major (one torch copy) and go through bev_pool_pm, the kernel the models
    run; everything else (and HEAL_LSS_PATH=sorted) takes the bit-reproducible radix-sort pipeline."""
    depth_logit = _need(depth_logit, torch.float32, "depth_logit")
    feat = _need(feat, torch.float32, "feat")
    frustum = _need(frustum, torch.float32, "frustum")
    BN, D, fH, fW = (int(v) for v in depth_logit.shape)
    C = int(feat.shape[1])
    if BN != n_agents * n_cams or tuple(feat.shape) != (BN, C, fH, fW) or tuple(frustum.shape) != (D, fH, fW, 3):
        raise _capi.HealAmdError("bev_pool: inconsistent shapes")
    cam_mats = _need(cam_mats, torch.float32, "cam_mats")
    if tuple(cam_mats.shape) != (BN, 27):
        raise _capi.HealAmdError("bev_pool: cam_mats must be [n_agents*n_cams, 27]")
    if bev_pool_pm_supported(D, fH, C) and D % 4 == 0 and _frustum_separable(frustum):
        head = torch.cat([feat, depth_logit], 1).permute(0, 2, 3, 1).reshape(BN, fH * fW, C + D).contiguous()
        return bev_pool_pm(head, C, D, fH, fW, frustum, cam_mats, n_agents, n_cams, dx, bx, nx)
    nxi = [int(v) for v in nx]
    dev = feat.device
    out = torch.empty((n_agents, C * nxi[2], nxi[1], nxi[0]), dtype=torch.float32, device=dev)
    nbytes = _capi.query("heal_bev_pool_workspace", n_agents, n_cams, D, fH, fW, C, nxi[0], nxi[1], nxi[2])
    ws = _workspace("bev_pool", nbytes, dev)
    with _Timed("bev_pool"):
        _capi.call("heal_bev_pool", _ptr(depth_logit), _ptr(feat), _ptr(frustum),
                   _ptr(cam_mats), n_agents, n_cams, D, fH, fW, C,
                   _host_array([float(v) for v in dx], ctypes.c_float),
                   _host_array([float(v) for v in bx], ctypes.c_float),
                   _host_array(nxi, ctypes.c_int32), _ptr(out), _ptr(ws), ws.numel(), _stream())
    return out


def bev_pool_backward(grad_out, depth_logit, feat, frustum, cam_mats, n_agents, n_cams, dx, bx, nx):
    """Gradient of bev_pool with respect to (depth_logit, feat).  grad_out [n_agents, C*nz, ny, nx] -> (grad_logit, grad_feat)
    with the shapes of depth_logit / feat."""
    depth_logit = _need(depth_logit, torch.float32, "depth_logit")
    feat = _need(feat, torch.float32, "feat")
    frustum = _need(frustum, torch.float32, "frustum")
    cam_mats = _need(cam_mats, torch.float32, "cam_mats")
    BN, D, fH, fW = (int(v) for v in depth_logit.shape)
    C = int(feat.shape[1])
    nxi = [int(v) for v in nx]
    if tuple(grad_out.shape) != (n_agents, C * nxi[2], nxi[1], nxi[0]) or tuple(frustum.shape) != (D, fH, fW, 3):
        raise _capi.HealAmdError("bev_pool_backward: inconsistent shapes")
    # cell-major rows: the gradient of one BEV cell is one contiguous row (the forward's scratch layout)
    gcells = _need(grad_out.reshape(n_agents, nxi[2], C, nxi[1], nxi[0]).permute(0, 1, 3, 4, 2).contiguous().view(-1, C),
                   torch.float32, "grad_out")
    g_logit, g_feat = torch.empty_like(depth_logit), torch.empty_like(feat)
    with _Timed("bev_pool_backward"):
        _capi.call("heal_bev_pool_backward", _ptr(gcells), _ptr(depth_logit), _ptr(feat), _ptr(frustum), _ptr(cam_mats),
                   n_agents, n_cams, D, fH, fW, C, _host_array([float(v) for v in dx], ctypes.c_float),
                   _host_array([float(v) for v in bx], ctypes.c_float), _host_array(nxi, ctypes.c_int32),
                   _ptr(g_logit), _ptr(g_feat), _stream())
    return g_logit, g_feat


# ------------------------------------------------------------------------------------------------ K3
def _i3(v):
    return _host_array([int(x) for x in v], ctypes.c_int32)


def _optr(t):
    return _ptr(t) if t is not None else None


def mean_vfe(voxels, num_points, n_dev=None):
    """MeanVFE: voxels [M,P,F], num_points [M] -> [M,F].  n_dev: optional device row count (M is then the capacity)."""
    voxels = _need(voxels, torch.float32, "voxels")
    num_points = _need(num_points, torch.int32, "num_points")
    M, P, F = (int(v) for v in voxels.shape)
    out = torch.empty((M, F), dtype=torch.float32, device=voxels.device)
    _capi.call("heal_mean_vfe", _ptr(voxels), _ptr(num_points), M, P, F, _ptr(out), _optr(n_dev), _stream())
    return out


def sp_weight_fragments(weight):
    """[K,Cin,Cout] -> the fragment order of the pair-compacted kernel (heal_sp_weight_fragments).  None when the channel counts
    have no fragment form."""
    K, cin, cout = (int(v) for v in weight.shape)
    if cin % 4 or (cin >= 16 and cin % 16) or cout % 16 or cin < 4 or int(weight.shape[0]) > 27:
        return None

    def build():
        out = torch.empty_like(weight)
        _capi.call("heal_sp_weight_fragments", _ptr(weight), K, cin, cout, _ptr(out), _stream())
        return out
    return _derived("sp_weight_fragments", (weight,), build)


class PairTiles:
    """The rulebook of a thin sparse layer as pair tiles (include/heal_amd.h, heal_sp_neighbor_tiles): one fixed-stride slot per 64
    output sites, only the used prefix written.  Stands where the [n_out, 27] neighbour table stands in SparseTensor.conv for
    c_in <= 16; `.to_neighbors()` decodes it into that table (bit for bit what heal_sp_neighbors_rank gives)."""

    def __init__(self, buf, n_out, n_out_dev=None, slot_sites=64):
        self.buf, self.n_out, self.n_out_dev, self.slot_sites = buf, int(n_out), n_out_dev, int(slot_sites)
        self.shape = (self.n_out, 27)
        self.device = buf.device

    def to_neighbors(self):
        nbr = torch.full((self.n_out, 27), -1, dtype=torch.int32, device=self.buf.device)
        _capi.call("heal_sp_tiles_to_neighbors", _ptr(self.buf), self.n_out, self.slot_sites, _optr(self.n_out_dev), _ptr(nbr),
                   _stream())
        return nbr

    def __getitem__(self, key):     # bench.py counts the live pairs of a traced layer through the table
        return self.to_neighbors()[key]


def sp_rank_enabled():
    """HEAL_SP_RULEBOOK=hash: sort + hash-grid rulebooks instead of the rank structures, for the voxel set and every layer."""
    return switches.get("HEAL_SP_RULEBOOK") == "rank"


def sp_root_rank_enabled():
    """HEAL_SP_ROOT=sort: radix sort + hash grid for the voxel set alone; the layers behind it keep their rank structures."""
    return sp_rank_enabled() and switches.get("HEAL_SP_ROOT") == "rank"


def sp_tiles_enabled():
    """HEAL_SP_TILES=0: every sparse layer through the [n_out, K] neighbour table (A/B, and what training uses)."""
    return switches.on("HEAL_SP_TILES")


class SparseTensor:
    """features [n,C] f32 + indices [n,4] i32 (b,z,y,x) sorted by linear coordinate + shape (D,H,W).

    `n_dev` (int32 [1] on the device, or None): when set, the buffers have CAPACITY rows and the live row count stays
    on the device -- no host round trip anywhere in the encoder (HIP-graph capturable).  Strided layers then size their
    outputs by a capacity bound (twice the voxel capacity, see out_sites) instead of the exact count; `overflow()` reports, after the
    fact, whether any layer produced more sites than its capacity."""

    def __init__(self, features, indices, spatial_shape, batch_size, n_dev=None, checks=None, root_cap=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self.n_dev = n_dev
        self._checks = checks if checks is not None else []
        self._root_cap = int(root_cap) if root_cap is not None else int(indices.shape[0])  # rows of the voxel set
        self._table = None
        self._rank = None   # rank structure (bitmap + prefix counts) when this site set came out of out_sites_ex()
        self._rank_root = False   # ... or the two-level structure of the voxel set (from_unsorted)

    @property
    def n(self):
        """Rows of the buffers (= live rows when n_dev is None, capacity otherwise)."""
        return int(self.indices.shape[0])

    def overflow(self):
        """Host check (synchronises): True if a strided layer found more active sites than its capacity."""
        return any(int(c.item()) > cap for c, cap in self._checks)

    @staticmethod
    def from_unsorted(features, indices, spatial_shape, batch_size, n_dev=None):
        """Sort the sites by linear coordinate (K3 keeps them sorted for coherent tiles)."""
        features = _need(features, torch.float32, "features")
        indices = _need(indices, torch.int32, "indices")
        n = int(indices.shape[0])
        dev = indices.device
        sorted_idx = torch.empty_like(indices)
        perm = torch.zeros((n,), dtype=torch.int32, device=dev)  # zeros: padding rows gather row 0, harmlessly
        rank = None
        C = int(features.shape[1])
        feats = torch.zeros((n, C), dtype=torch.float32, device=dev) if n_dev is not None else torch.empty((n, C), dtype=torch.float32, device=dev)
        if sp_root_rank_enabled():
            # rank(linear coordinate) IS the sorted position: one scatter (sites, permutation and feature rows) instead of a radix
            # sort + gather, and the structure answers the neighbour queries of the layers that read the voxel set (no hash grid)
            nbytes = _capi.query("heal_sp_root_rank_bytes", _i3(spatial_shape), int(batch_size))
            rank = torch.empty((nbytes,), dtype=torch.uint8, device=dev)   # lives as long as the site set it describes
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_root_rank", _ptr(indices), n, _i3(spatial_shape), int(batch_size), _ptr(sorted_idx),
                           _ptr(perm), _ptr(features), C, _ptr(feats), _ptr(rank), nbytes, _optr(n_dev), _stream())
        else:
            ws = _workspace("sp_sort", _capi.query("heal_sp_sort_workspace", n), dev)
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_sort_sites", _ptr(indices), n, _i3(spatial_shape), int(batch_size), _ptr(sorted_idx),
                           _ptr(perm), _ptr(ws), ws.numel(), _optr(n_dev), _stream())
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_gather_rows", _ptr(features), _ptr(perm), n, C, _optr(n_dev), _ptr(feats), _stream())
        st = SparseTensor(feats, sorted_idx, spatial_shape, batch_size, n_dev)
        st._rank, st._rank_root = rank, rank is not None
        st._perm = perm   # row i of the sorted set = input row perm[i] (the gradient path re-applies it differentiably)
        return st

    def table(self):
        if self._table is None:
            cap = _capi.query("heal_sp_table_capacity", self.n)
            dev = self.indices.device
            keys = torch.empty((cap,), dtype=torch.int32, device=dev)
            vals = torch.empty((cap,), dtype=torch.int32, device=dev)
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_hash_build", _ptr(self.indices), self.n, _i3(self.spatial_shape), self.batch_size,
                           _ptr(keys), _ptr(vals), cap, _optr(self.n_dev), _stream())
            self._table = (keys, vals, cap)
        return self._table

    def neighbors(self, out_indices, out_shape, ksize, stride, padding, n_out_dev=None):
        n_out = int(out_indices.shape[0])
        K = int(ksize[0] * ksize[1] * ksize[2])
        nbr = torch.empty((n_out, K), dtype=torch.int32, device=self.indices.device)
        if self._rank is not None:
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_neighbors_root" if self._rank_root else "heal_sp_neighbors_rank",
                           _ptr(out_indices), n_out, _i3(ksize), _i3(stride), _i3(padding),
                           _i3(self.spatial_shape), _i3(out_shape), self.batch_size, _ptr(self._rank), self._rank.numel(),
                           self.n, _optr(self.n_dev), _ptr(nbr), _optr(n_out_dev), _stream())
            return nbr
        keys, vals, cap = self.table()
        with _Timed("sp_rulebook"):
            _capi.call("heal_sp_neighbors", _ptr(out_indices), n_out, _i3(ksize), _i3(stride), _i3(padding),
                       _i3(self.spatial_shape), _i3(out_shape), self.batch_size, _ptr(keys), _ptr(vals), cap,
                       _ptr(nbr), _optr(n_out_dev), _stream())
        return nbr

    def rulebook(self, out_indices, out_shape, ksize, stride, padding, cin, cout, n_out_dev=None):
        """What SparseTensor.conv needs for a (cin -> cout) layer on these output sites: pair tiles when the thin-layer kernel
        takes the layer (3 x 3 x 3, c_in <= 16, rank-structure path), the neighbour table otherwise."""
        if not self.tiles_ok(ksize, cin, cout):
            return self.neighbors(out_indices, out_shape, ksize, stride, padding, n_out_dev=n_out_dev)
        n_out = int(out_indices.shape[0])
        # sites per slot: 64.  128 fill the 16-pair tiles of a strided layer better (2.5 live taps of 27 per site on conv2's
        # SparseConv3d: -5 us on that convolution) but the rulebook kernel then has half the waves for the same lookups (+22 us):
        # HEAL_SP_SLOT_SITES=128 is the A/B switch of a HEAL_BUILD_EXPERIMENTAL=1 library (profiles/r06_k3_thin.json)
        sites = switches.number("HEAL_SP_SLOT_SITES")
        buf = torch.empty((_capi.query("heal_sp_pair_tiles_words", n_out, sites),), dtype=torch.int32, device=self.indices.device)
        with _Timed("sp_rulebook"):
            _capi.call("heal_sp_neighbor_tiles", _ptr(out_indices), n_out, _i3(ksize), _i3(stride), _i3(padding),
                       _i3(self.spatial_shape), _i3(out_shape), self.batch_size, _ptr(self._rank), self._rank.numel(),
                       int(bool(self._rank_root)), self.n, _optr(self.n_dev), sites, _ptr(buf), _optr(n_out_dev), _stream())
        return PairTiles(buf, n_out, n_out_dev, sites)

    def tiles_ok(self, ksize, cin, cout):
        return (sp_tiles_enabled() and self._rank is not None and tuple(int(k) for k in ksize) == (3, 3, 3)
                and self.n < (1 << 24) and bool(_capi.query("heal_sp_conv_tiles_supported", int(cin), int(cout))))

    def out_sites(self, ksize, stride, padding):
        """Active output sites of a strided conv: (indices sorted, out_shape, n_out_dev).  Exact-size indices and
        n_out_dev None when this tensor carries host counts; capacity-size indices plus the device count otherwise."""
        return self.out_sites_ex(ksize, stride, padding)[:3]

    def out_sites_ex(self, ksize, stride, padding):
        """out_sites() plus the rank structure of the output site set (None on the hash + sort path, HEAL_SP_RULEBOOK=hash):
        hand it to the SparseTensor built on these sites (`._rank`) and its neighbour queries skip the hash grid."""
        out_shape = [(self.spatial_shape[d] + 2 * padding[d] - ksize[d]) // stride[d] + 1 for d in range(3)]
        K = int(ksize[0] * ksize[1] * ksize[2])
        dev = self.indices.device
        cells = self.batch_size * out_shape[0] * out_shape[1] * out_shape[2]
        worst = max(1, min(self.n * min(K, 8), cells))
        # capacity bound of the no-sync mode: twice the voxel capacity at every level.  Measured on 64-line sweeps at
        # 0.1 m voxels the site count goes x1.36 (isolated far-range voxels dilate), x0.68, x0.48, x0.51 through the
        # four strided layers; overflow() reports a violation.
        out_cap = worst if self.n_dev is None else max(1, min(worst, 2 * self._root_cap))
        out_idx = torch.empty((out_cap, 4), dtype=torch.int32, device=dev)
        n_out = torch.zeros((1,), dtype=torch.int32, device=dev)
        rank = None
        if sp_rank_enabled():
            nbytes = _capi.query("heal_sp_rank_bytes", _i3(out_shape), self.batch_size)
            rank = torch.empty((nbytes,), dtype=torch.uint8, device=dev)   # lives as long as the site set it describes
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_out_sites_rank", _ptr(self.indices), self.n, _i3(ksize), _i3(stride), _i3(padding),
                           _i3(self.spatial_shape), _i3(out_shape), self.batch_size, _ptr(out_idx), out_cap, _ptr(n_out),
                           _ptr(rank), nbytes, _optr(self.n_dev), _ptr(sparse_overflow_flag(dev)), _stream())
        else:
            ws = _workspace("sp_out_sites", _capi.query("heal_sp_out_sites_workspace", self.n, K), dev)
            with _Timed("sp_rulebook"):
                _capi.call("heal_sp_out_sites", _ptr(self.indices), self.n, _i3(ksize), _i3(stride), _i3(padding),
                           _i3(self.spatial_shape), _i3(out_shape), self.batch_size, _ptr(out_idx), out_cap, _ptr(n_out),
                           _ptr(ws), ws.numel(), _optr(self.n_dev), _stream())
        if self.n_dev is None:
            return out_idx[:int(n_out.item())], out_shape, None, rank
        self._checks.append((n_out, out_cap))
        _SPARSE_CHECKS.append((n_out, out_cap))
        if len(_SPARSE_CHECKS) > 4096:   # nobody verifies (no host sync on this path at all): keep the list bounded
            del _SPARSE_CHECKS[:2048]
        return out_idx, out_shape, n_out, rank

    def conv(self, nbr, weight, bn_scale, bn_shift, relu=True, n_out_dev=None):
        """Gather-GEMM: weight [K,Cin,Cout]; returns features [n_out,Cout]."""
        weight = _need(weight, torch.float32, "weight")
        K, cin, cout = (int(v) for v in weight.shape)
        features = _need_rows(self.features, cin, "features", "SparseTensor.conv")
        if not isinstance(nbr, PairTiles):       # pair tiles: a word buffer, checked against K and the channels below
            nbr = _need_nbr(nbr, K, "SparseTensor.conv")
        bn_scale = _need_channels(bn_scale, cout, "bn_scale", "SparseTensor.conv")
        bn_shift = _need_channels(bn_shift, cout, "bn_shift", "SparseTensor.conv")
        frag = sp_weight_fragments(weight)
        n_out = int(nbr.shape[0])
        out = torch.empty((n_out, cout), dtype=torch.float32, device=nbr.device)
        # SURVEY 8d, K3 per layer: 4 (N_in C_in + N_out C_out) + 4 K C_in C_out + 8 R bytes, 2 R C_in C_out flops; with device
        # row counts the host only knows capacities: bench.py fills in the live N_in / N_out / R of its instrumented pass
        with _Timed(f"sp_conv_{cin}_{cout}") as tm:
            if isinstance(nbr, PairTiles):
                if K != 27 or not _capi.query("heal_sp_conv_tiles_supported", cin, cout):
                    raise ValueError(f"SparseTensor.conv: pair tiles do not serve a {K}-tap {cin} -> {cout} layer "
                                     "(SparseTensor.rulebook decides per layer)")
                _capi.call("heal_sp_conv_tiles", _ptr(features), _ptr(nbr.buf), n_out, nbr.slot_sites, cin, cout, _ptr(frag),
                           _ptr(bn_scale), _ptr(bn_shift), int(bool(relu)), _ptr(out), _optr(n_out_dev), _stream())
            else:
                _capi.call("heal_sp_conv", _ptr(features), _ptr(nbr), n_out, K, cin, cout, _ptr(weight), _optr(frag),
                           _ptr(bn_scale), _ptr(bn_shift), int(bool(relu)), _ptr(out), _optr(n_out_dev), _stream())
        if SP_TRACE is not None and TIMING is not None:
            SP_TRACE.append({"cin": cin, "cout": cout, "K": K, "n_in": self.n_dev if self.n_dev is not None else self.n,
                             "n_out": n_out_dev if n_out_dev is not None else n_out, "nbr": nbr, "events": (tm.e0, tm.e1)})
        return out

    def dense(self):
        """-> [B, C*D, H, W] with channel = c*D + z (height_compression.py:21-23)."""
        C = int(self.features.shape[1])
        D, H, W = self.spatial_shape
        dev = self.indices.device
        out = torch.empty((self.batch_size, C * D, H, W), dtype=torch.float32, device=dev)
        ws = _workspace("sp_to_bev", _capi.query("heal_sp_to_bev_workspace", self.batch_size, D, H, W), dev)
        with _Timed("sp_to_bev"):
            _capi.call("heal_sp_to_bev", _ptr(self.features), _ptr(self.indices), self.n, C, _i3(self.spatial_shape),
                       self.batch_size, _ptr(out), _ptr(ws), ws.numel(), _optr(self.n_dev), _stream())
        return out


_SP_IDENT = {}


def sp_conv_raw(features, nbr, weight):
    """The bare sparse convolution (no BatchNorm, no ReLU): out[o] = sum_tap weight[tap]^T features[nbr[o][tap]].  features
    [n_in, Cin], nbr [n_out, K] i32, weight [K, Cin, Cout] -> [n_out, Cout].  Building block of the gradient path (forward AND,
    with the transposed rulebook and weight[tap]^T, the gradient with respect to the input features)."""
    features = _need(features, torch.float32, "features")
    weight = _need(weight, torch.float32, "weight")
    K, cin, cout = (int(v) for v in weight.shape)
    features = _need_rows(features, cin, "features", "sp_conv_raw")
    nbr = _need_nbr(nbr, K, "sp_conv_raw")
    key = (cout, str(features.device))
    ident = _SP_IDENT.get(key)
    if ident is None:
        ident = _SP_IDENT[key] = (torch.ones(cout, device=features.device), torch.zeros(cout, device=features.device))
    n_out = int(nbr.shape[0])
    out = torch.empty((n_out, cout), dtype=torch.float32, device=features.device)
    if n_out:
        _capi.call("heal_sp_conv", _ptr(features), _ptr(nbr), n_out, K, cin, cout, _ptr(weight), _optr(sp_weight_fragments(weight)),
                   _ptr(ident[0]), _ptr(ident[1]), 0, _ptr(out), None, _stream())
    return out


def sp_wgrad_supported(cin, cout):
    return 1 <= cin <= 64 and cout in (16, 32, 48, 64)


def sp_wgrad(features, grad_out, nbr):
    """Weight gradient of the bare sparse convolution: dW[tap] = sum over the rule pairs of x[i]^T g[o] -> [K, Cin, Cout]."""
    features = _need(features, torch.float32, "features")
    grad_out = _need(grad_out, torch.float32, "grad_out")
    nbr = _need(nbr, torch.int32, "nbr")
    if nbr.dim() != 2 or features.dim() != 2 or grad_out.dim() != 2:
        raise _capi.HealAmdError(f"sp_wgrad: features {tuple(features.shape)}, grad_out {tuple(grad_out.shape)} and nbr "
                                 f"{tuple(nbr.shape)} must be matrices")
    n_out, K = (int(v) for v in nbr.shape)
    cin, cout = int(features.shape[1]), int(grad_out.shape[1])
    if int(grad_out.shape[0]) != n_out:
        raise _capi.HealAmdError(f"sp_wgrad: grad_out has {int(grad_out.shape[0])} rows for the {n_out} output rows of nbr")
    if n_out == 0:
        return torch.zeros((K, cin, cout), dtype=torch.float32, device=features.device)
    chunks = _capi.query("heal_sp_wgrad_chunks", n_out)
    part = torch.empty((chunks, K, cin, cout), dtype=torch.float32, device=features.device)
    _capi.call("heal_sp_wgrad", _ptr(features), _ptr(grad_out), _ptr(nbr), n_out, K, cin, cout, None, _ptr(part), _stream())
    return part.sum(0)


def sp_transpose_neighbors(nbr, n_in):
    """nbr [n_out, K] -> nbr_t [n_in, K]: nbr_t[i][tap] = o where nbr[o][tap] = i (else -1): the rulebook of the backward pass."""
    nbr = _need(nbr, torch.int32, "nbr")
    n_out, K = (int(v) for v in nbr.shape)
    nbr_t = torch.empty((int(n_in), K), dtype=torch.int32, device=nbr.device)
    _capi.call("heal_sp_transpose_neighbors", _ptr(nbr), n_out, K, int(n_in), _ptr(nbr_t), None, _stream())
    return nbr_t


# ------------------------------------------------------------------------------------------------ K6
def _agent_attention_args(who, q, k, v, key_mask, agent_major):
    """q, k, v [n_pix, L, 256] (or [L, n_pix, 256]) f32 cuda of ONE shape and key_mask [L] int32 cuda, made contiguous: the kernels
    read L rows of 256 floats per pixel from each of the three and L mask words from bare pointers, so a `v` with fewer pixels
    or a short mask would be read out of bounds without an error.  -> (q, k, v, key_mask, n_pix, L)"""
    q = _need(q, torch.float32, "q"); k = _need(k, torch.float32, "k"); v = _need(v, torch.float32, "v")
    if q.dim() != 3 or int(q.shape[2]) != 256:
        raise _capi.HealAmdError(f"{who}: q has shape {tuple(q.shape)}, want [n_pix, L, 256] ([L, n_pix, 256] agent-major): "
                                 "the last dimension must be 256")
    for name, t in (("k", k), ("v", v)):
        if tuple(t.shape) != tuple(q.shape):
            raise _capi.HealAmdError(f"{who}: {name} has shape {tuple(t.shape)}, q has {tuple(q.shape)}")
    L, n_pix = (int(q.shape[0]), int(q.shape[1])) if agent_major else (int(q.shape[1]), int(q.shape[0]))
    if not 1 <= L <= AGENT_ATTENTION_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: {L} agents, the kernel takes 1..{AGENT_ATTENTION_MAX_AGENTS}")
    if key_mask is not None:
        key_mask = _need(key_mask, torch.int32, "key_mask")
        if key_mask.numel() != L:
            raise _capi.HealAmdError(f"{who}: key_mask has {key_mask.numel()} entries for {L} agents")
    return q, k, v, key_mask, n_pix, L


def agent_attention(q, k, v, heads, scale, key_mask=None, out_rows=None, agent_major=False, out=None):
    """K6.  q,k,v [n_pix, L, 256] f32 cuda -> [n_pix, out_rows, 256] (softmax over the L agents per
    pixel and head; key_mask [L] int32 cuda marks real agents).  agent_major: q, k, v [L, n_pix, 256] -> [out_rows, n_pix, 256].
    The result is written into `out` when given."""
    who = "agent_attention"
    q, k, v, key_mask, n_pix, L = _agent_attention_args(who, q, k, v, key_mask, agent_major)
    rows = L if out_rows is None else int(out_rows)
    if not 1 <= rows <= L:
        raise _capi.HealAmdError(f"{who}: out_rows {rows} outside 1..{L}")
    out = _out_or_empty(out, (rows, n_pix, 256) if agent_major else (n_pix, rows, 256), q.device, who)
    with _Timed(f"agent_attention_h{heads}"):
        _capi.call("heal_agent_attention", _ptr(q), _ptr(k), _ptr(v), _optr(key_mask), n_pix, L, 256, int(heads),
                   float(scale), rows, _ptr(out), int(bool(agent_major)), _stream())
    return out


def agent_attention_backward(q, k, v, grad_out, heads, scale, key_mask=None, agent_major=False, grads=None):
    """Backward of agent_attention: grad_out [n_pix, out_rows, 256] (or [out_rows, n_pix, 256]) -> (grad_q, grad_k, grad_v), each
    shaped like q (written into the three buffers of `grads` when given).  Rows >= out_rows of the forward output were not
    produced and carry no gradient."""
    who = "agent_attention_backward"
    q, k, v, key_mask, n_pix, L = _agent_attention_args(who, q, k, v, key_mask, agent_major)
    grad_out = _need(grad_out, torch.float32, "grad_out")
    rows = int(grad_out.shape[0 if agent_major else 1]) if grad_out.dim() == 3 else 0
    if not 1 <= rows <= L:
        raise _capi.HealAmdError(f"{who}: grad_out has shape {tuple(grad_out.shape)}: its out_rows must be in 1..{L}")
    if tuple(grad_out.shape) != ((rows, n_pix, 256) if agent_major else (n_pix, rows, 256)):
        raise _capi.HealAmdError(f"{who}: grad_out has shape {tuple(grad_out.shape)} for q of shape {tuple(q.shape)}")
    if grads is None:
        grads = (None, None, None)
    gq, gk, gv = (_out_or_empty(g, tuple(q.shape), q.device, who) for g in grads)
    with _Timed(f"agent_attention_bwd_h{heads}"):
        _capi.call("heal_agent_attention_backward", _ptr(q), _ptr(k), _ptr(v), _optr(key_mask), _ptr(grad_out), n_pix, L, 256,
                   int(heads), float(scale), rows, _ptr(gq), _ptr(gk), _ptr(gv), int(bool(agent_major)), _stream())
    return gq, gk, gv


class AgentAttention(torch.autograd.Function):
    """agent_attention under autograd (the gradient path of HGTCavAttention and AttFusion on the device): forward = K6, backward =
    heal_agent_attention_backward; saves q, k, v only (the L x L probabilities are recomputed per pixel)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale, out_rows, agent_major):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.save_for_backward(q, k, v)
        ctx.cfg = (int(heads), float(scale), bool(agent_major))
        return agent_attention(q, k, v, heads, scale, out_rows=out_rows, agent_major=agent_major)

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v = ctx.saved_tensors
        heads, scale, am = ctx.cfg
        gq, gk, gv = agent_attention_backward(q, k, v, grad_out.contiguous(), heads, scale, agent_major=am)
        return gq, gk, gv, None, None, None, None


AGENT_ATTENTION_MAX_AGENTS = _limit("HEAL_AGENT_ATTENTION_MAX_AGENTS")


def agent_attention_train_supported(q, heads):
    """The device gradient path: fp32 CUDA tensors, 256 channels, heads in {1, 4, 8, 16}; the caller checks that there are at most
    AGENT_ATTENTION_MAX_AGENTS agents."""
    return bool(q.is_cuda and q.dtype == torch.float32 and q.shape[-1] == 256 and heads in (1, 4, 8, 16))


# ------------------------------------------------------------------------------------------------ KD
def kd_kl_torch(student, teacher):
    """The reference's composition (point_pillar_disconet_loss.py:37-44): KLDivLoss(size_average=True, reduce=True), i.e.
    reduction 'mean' over ELEMENTS, of log_softmax(student) against softmax(teacher) over the channels of every pixel.  The CPU,
    non-fp32 and teacher-with-gradient path, and the HEAL_KD_FUSED=0 side of the A/B."""
    import warnings
    N, C, H, W = teacher.shape
    t = teacher.permute(0, 2, 3, 1).reshape(N * H * W, C)
    s = student.permute(0, 2, 3, 1).reshape(N * H * W, C)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)        # torch recommends 'batchmean'; the reference asks for 'mean'
        return torch.nn.functional.kl_div(torch.nn.functional.log_softmax(s, dim=1), torch.nn.functional.softmax(t, dim=1),
                                          reduction="mean")


def kd_kl_supported(student, teacher):
    """The fused distillation term: CUDA fp32 maps of one 4-D shape and a teacher outside the autograd graph (the kernel has no
    gradient for it).  HEAL_KD_FUSED=0 forces the torch composition (scripts/kd_bench.py)."""
    return bool(isinstance(student, torch.Tensor) and isinstance(teacher, torch.Tensor) and student.is_cuda and teacher.is_cuda
                and student.dtype == torch.float32 and teacher.dtype == torch.float32 and student.dim() == 4
                and student.shape == teacher.shape and student.numel() > 0 and student.device == teacher.device
                and not (teacher.requires_grad and torch.is_grad_enabled())
                and switches.on("HEAL_KD_FUSED"))


def kd_kl_loss(student, teacher, need_grad=True, grad_out=None):
    """KD.  student, teacher [N, C, H, W] f32 cuda (made contiguous) -> (loss [1], grad | None): the KL term of DiscoNet's
    distillation, mean over the N*C*H*W elements, and d loss / d student = (softmax(student) - softmax(teacher)) / (N*C*H*W).
    need_grad=False passes a NULL gradient: the kernel only reads.  grad_out: a contiguous f32 buffer of the student's shape to
    write the gradient into.  Two launches, no host synchronisation, no atomics (bit-equal from run to run)."""
    who = "kd_kl_loss"
    (student, teacher), _ = _loss_inputs(who, (("student", student), ("teacher", teacher)), ())
    if student.shape != teacher.shape:
        raise _capi.HealAmdError(f"{who}: student {tuple(student.shape)} and teacher {tuple(teacher.shape)} must be equal, "
                                 "non-empty [N, C, H, W] maps")
    N, C, H, W = (int(v) for v in student.shape)
    (grad,) = _loss_grad_buffers(who, (student,), bool(need_grad), None if grad_out is None else (grad_out,))
    nbytes, ws, loss = _loss_workspace(who, "kd_kl", "heal_kd_kl_loss_workspace", (N, C, H, W), f"shape {(N, C, H, W)} is", 1,
                                       student.device)
    with _Timed(f"kd_kl_loss_c{C}", nbytes=4.0 * student.numel() * (3 if need_grad else 2)):
        _capi.call("heal_kd_kl_loss", _ptr(student), _ptr(teacher), N, C, H, W, _ptr(loss), _ptr(grad), _ptr(ws),
                   ctypes.c_size_t(nbytes), _stream())
    return loss, grad


class _FusedLoss(torch.autograd.Function):
    """The fused criteria under autograd.  run(need) is the raw operator with everything but need_grad bound: it runs the kernel,
    which also writes d loss / d map for the maps that need one.  forward saves those; backward multiplies each by the incoming
    gradient -- per_term: of the map's own term (det, center: out = terms [k], map i belongs to term i), otherwise of the one scalar
    (kd, occ, depth: out = loss [1], returned 0-d).  Only `maps` are differentiable; labels and settings travel inside run.  An
    operator whose maps share terms (unc) returns out = (total, terms): the terms ride along without a gradient."""

    @staticmethod
    def forward(ctx, run, per_term, need, *maps):
        out, grads = run(need)
        if not isinstance(grads, (tuple, list)):            # the one map's gradient (kd, depth), or None: no map needed one
            grads = [grads] * len(maps)
        ctx.per_term, ctx.have = per_term, tuple(g is not None for g in grads)
        ctx.save_for_backward(*[g for g in grads if g is not None])
        if isinstance(out, tuple):
            ctx.mark_non_differentiable(*out[1:])
            return out
        return out if per_term else out.reshape(())

    @staticmethod
    def backward(ctx, grad, *_):
        saved = iter(ctx.saved_tensors)
        return (None, None, None,
                *[(grad[i] if ctx.per_term else grad) * next(saved) if have else None for i, have in enumerate(ctx.have)])


class KdKlLoss:
    """kd_kl_loss under autograd, KdKlLoss.apply(student, teacher) as the loss module calls it: -> the 0-d loss with the gradient
    for the student; the teacher receives none."""

    @staticmethod
    def apply(student, teacher):
        return _FusedLoss.apply(lambda need: kd_kl_loss(student, teacher, need_grad=need[0]), False, (_wants_grad(student),), student)


# ------------------------------------------------------------------------------------------------ DL
# The criterion terms of the training step (csrc/det_loss.hip).  HEAL_LOSS_FUSED=0 forces the torch compositions of
# heal_amd/opencood/loss/ (scripts/loss_bench.py), =1 the kernels wherever *_supported holds.
_LABEL_DTYPES = (torch.float32, torch.float64)


LOSS_MAX_ANCHORS, OCC_LOSS_MAX_LEVELS = _limit("HEAL_LOSS_MAX_ANCHORS"), _limit("HEAL_OCC_LOSS_MAX_LEVELS")


def loss_fused_enabled():
    return switches.on("HEAL_LOSS_FUSED")


def _loss_map_ok(t):
    return bool(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.numel() > 0)


def _loss_labels_ok(device, *labels):
    """Labels float32 or float64 (one type for all of them) on the maps' device."""
    return bool(all(isinstance(t, torch.Tensor) and t.device == device and t.dtype in _LABEL_DTYPES for t in labels)
                and len({t.dtype for t in labels}) == 1)


def det_loss_supported(cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, gamma=2.0, num_bins=2, iou=None,
                       batch_size=None):
    """The fused detection terms: CUDA fp32 head maps [N, A, H, W], [N, 7A, H, W] and (with a `dir` block) [N, 2A, H, W], at most
    LOSS_MAX_ANCHORS anchors, labels float32 or float64 on the same device with N*H*W*A (x 7) elements, gamma == 2, two direction bins, no `iou` block.  With
    a `dir` block A must be 2: the composition's own direction term is only defined there.  batch_size: what the loss module
    derived from record_len, when it differs from N the composition runs.  HEAL_LOSS_FUSED=0 forces the composition."""
    if not loss_fused_enabled() or iou or gamma != 2.0 or not (_loss_map_ok(cls_preds) and _loss_map_ok(reg_preds)):
        return False
    N, A, H, W = (int(v) for v in cls_preds.shape)
    maps = [cls_preds, reg_preds]
    if dir_preds is not None:
        if num_bins != 2 or A != 2 or not _loss_map_ok(dir_preds) or tuple(dir_preds.shape) != (N, 2 * A, H, W):
            return False
        maps.append(dir_preds)
    return bool(A <= LOSS_MAX_ANCHORS and tuple(reg_preds.shape) == (N, 7 * A, H, W) and all(m.device == cls_preds.device for m in maps)
                and (batch_size is None or int(batch_size) == N)
                and _loss_labels_ok(cls_preds.device, pos_equal_one, neg_equal_one, targets)
                and pos_equal_one.numel() == N * H * W * A and neg_equal_one.numel() == N * H * W * A
                and targets.numel() == N * H * W * A * 7
                and _capi.query("heal_det_loss_workspace", N, A, H, W) > 0)


def _loss_inputs(who, maps, labels):
    """Checked, detached, contiguous copies of the fp32 maps (None passes through) and the labels."""
    out = []
    dev = None
    for name, t in maps:
        if t is None:
            out.append(None)
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
        if t.dtype != torch.float32 or t.dim() != 4 or t.numel() == 0:
            raise _capi.HealAmdError(f"{who}: {name} must be a non-empty 4-D torch.float32 map, got {t.dtype} {tuple(t.shape)}")
        dev = dev if dev is not None else t.device
        if t.device != dev:
            raise _capi.HealAmdError(f"{who}: {name} is on {t.device}, the first map on {dev}")
        out.append(t.detach().contiguous())
    labs = []
    for name, t in labels:
        if not isinstance(t, torch.Tensor) or t.device != dev:
            raise _capi.HealAmdError(f"{who}: {name} must be a tensor on {dev}")
        if t.dtype not in _LABEL_DTYPES or t.dtype != labels[0][1].dtype:
            raise _capi.HealAmdError(f"{who}: {name} must be float32 or float64, the same for every label, got {t.dtype}")
        labs.append(t.detach().contiguous())
    return out, labs


def _loss_grad_buffers(who, maps, need_grad, grad_out):
    """need_grad: bool or one bool per map.  -> list of (buffer | None) per map; buffers from grad_out where given."""
    need = [bool(need_grad)] * len(maps) if isinstance(need_grad, bool) else [bool(v) for v in need_grad]
    if len(need) != len(maps):
        raise _capi.HealAmdError(f"{who}: need_grad has {len(need)} entries for {len(maps)} maps")
    grads = []
    for i, (m, want) in enumerate(zip(maps, need)):
        if m is None or not want:
            grads.append(None)
            continue
        g = grad_out[i] if grad_out is not None and grad_out[i] is not None else torch.empty_like(m)
        if not g.is_cuda or g.dtype != torch.float32 or g.shape != m.shape or not g.is_contiguous() or g.device != m.device:
            raise _capi.HealAmdError(f"{who}: grad_out[{i}] must be a contiguous f32 CUDA tensor of its map's shape")
        grads.append(g)
    return grads


def _loss_workspace(who, key, query, args, what, n_out, device, given=None):
    """Workspace query (raises where it answers 0: `what` out of range), the operator's workspace `key` -- or `given`, a caller's
    buffer, checked -- and the uninitialised f32 result [n_out].  -> (bytes, workspace, result)."""
    nbytes = _capi.query(query, *args)
    if nbytes == 0:
        raise _capi.HealAmdError(f"{who}: {what} out of range")
    if given is not None and not (given.is_cuda and given.dtype == torch.uint8 and given.is_contiguous() and given.numel() >= nbytes
                                  and given.data_ptr() % 256 == 0):
        raise _capi.HealAmdError(f"{who}: workspace must be a contiguous 256-B aligned uint8 CUDA tensor of >= {nbytes} bytes")
    ws = given if given is not None else _workspace(key, nbytes, device)
    return nbytes, ws, torch.empty(n_out, dtype=torch.float32, device=device)


def _anchor_head_inputs(who, maps, labels, dim, anchor_yaw, weights, sigma, need_grad, grad_out):
    """What det_loss and unc_loss do before their call.  maps: (name, tensor) of cls_preds, reg_preds, (unc_preds with dim set,)
    dir_preds | None; labels: (name, tensor) of pos_equal_one, neg_equal_one, targets.  -> (checked contiguous maps, labels,
    (N, A, H, W), the ctypes yaw array | NULL, grad buffers, bytes moved)."""
    names = ", ".join(name[:-len("_preds")] for name, _ in maps)
    maps, (pos, neg, tgt) = _loss_inputs(who, maps, labels)
    N, A, H, W = (int(v) for v in maps[0].shape)
    per_anchor = (1, 7, 2) if dim is None else (1, 7, dim, 2)
    if A > LOSS_MAX_ANCHORS or any(m is not None and tuple(m.shape) != (N, c * A, H, W) for m, c in zip(maps, per_anchor)):
        raise _capi.HealAmdError(f"{who}: maps {', '.join(str(tuple(m.shape)) for m in maps if m is not None)} are not [N, A, H, W], "
                                 f"[N, 7A, H, W]{'' if dim is None else f', [N, {dim}A, H, W]'} (, [N, 2A, H, W]) with at most "
                                 f"{LOSS_MAX_ANCHORS} anchors")
    if pos.numel() != N * H * W * A or neg.numel() != N * H * W * A or tgt.numel() != 7 * N * H * W * A:
        raise _capi.HealAmdError(f"{who}: labels of {pos.numel()}, {neg.numel()}, {tgt.numel()} elements for N*H*W*A = {N * H * W * A}")
    yaw = ctypes.c_void_p(0)
    if maps[-1] is not None:
        if anchor_yaw is None or len(anchor_yaw) != A:
            raise _capi.HealAmdError(f"{who}: dir_preds needs anchor_yaw with {A} angles (radians)")
        yaw = ctypes.cast((ctypes.c_double * A)(*[float(v) for v in anchor_yaw]), ctypes.c_void_p)
    if len(weights) != len(maps) or not float(sigma) > 0:
        raise _capi.HealAmdError(f"{who}: weights must be ({names}) and sigma positive")
    grads = _loss_grad_buffers(who, maps, need_grad, grad_out)
    moved = sum(4.0 * m.numel() for m in maps if m is not None) + sum(4.0 * g.numel() for g in grads if g is not None) \
        + float(pos.element_size()) * (2 * pos.numel() + tgt.numel())
    return maps, (pos, neg, tgt), (N, A, H, W), yaw, grads, moved


def det_loss(cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, pos_cls_weight, alpha, sigma, weights,
             anchor_yaw=None, dir_offset=0.0, need_grad=True, grad_out=None):
    """DL.  PointPillarLoss's three terms and their gradients in one pass: cls_preds [N, A, H, W], reg_preds [N, 7A, H, W],
    dir_preds [N, 2A, H, W] | None, f32 cuda (made contiguous); pos_equal_one, neg_equal_one [N, H, W, A], targets [N, H, W, 7A],
    float32 or float64, read in place.  weights = (cls, reg, dir) loss weights, anchor_yaw: A angles in RADIANS, gamma = 2 and two
    direction bins.  -> (terms [3] = cls, reg, dir loss, each x weight / N, (grad_cls, grad_reg, grad_dir) | None).
    need_grad: bool or one per map; False passes NULL gradients: the kernels only read.  grad_out: buffers to write into."""
    who = "det_loss"
    maps, (pos, neg, tgt), (N, A, H, W), yaw, grads, moved = _anchor_head_inputs(
        who, (("cls_preds", cls_preds), ("reg_preds", reg_preds), ("dir_preds", dir_preds)),
        (("pos_equal_one", pos_equal_one), ("neg_equal_one", neg_equal_one), ("targets", targets)), None, anchor_yaw, weights, sigma,
        need_grad, grad_out)
    nbytes, ws, terms = _loss_workspace(who, "det_loss", "heal_det_loss_workspace", (N, A, H, W), f"shape {(N, A, H, W)} is", 3,
                                        maps[0].device)
    with _Timed(f"det_loss_a{A}", nbytes=moved):
        _capi.call("heal_det_loss", *(_ptr(m) for m in maps), _ptr(pos), _ptr(neg), _ptr(tgt), int(pos.dtype == torch.float64),
                   N, A, H, W, float(pos_cls_weight), float(alpha), float(sigma), *(float(w) for w in weights), yaw,
                   float(dir_offset), _ptr(terms), *(_ptr(g) for g in grads), _ptr(ws), ctypes.c_size_t(nbytes), _stream())
    return terms, (tuple(grads) if any(g is not None for g in grads) else None)


def _wants_grad(t):
    return bool(t is not None and t.requires_grad and torch.is_grad_enabled())


def _loss_terms(op, per_term, maps, *rest, **cfg):
    """op(*maps, *rest, **cfg) under autograd (_FusedLoss), with a gradient for each of `maps` that requires one."""
    return _FusedLoss.apply(lambda need: op(*maps, *rest, need_grad=need, **cfg), per_term, tuple(_wants_grad(t) for t in maps),
                            *maps)


def det_loss_terms(cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, **cfg):
    """The differentiable form of det_loss: -> terms [3] (cls, reg, dir), gradients for the maps that require one."""
    return _loss_terms(det_loss, True, (cls_preds, reg_preds, dir_preds), pos_equal_one, neg_equal_one, targets, **cfg)


_UNC_XY = {"l2": 0, "l1": 1}              # HEAL_UNC_L2 / HEAL_UNC_L1 of include/heal_amd_unc.h
_UNC_ANGLE = {"l2": 0, "von-mise": 1}     # HEAL_UNC_L2 / HEAL_UNC_VON_MISES


def unc_loss_supported(cls_preds, reg_preds, unc_preds, dir_preds, pos_equal_one, neg_equal_one, targets, dim, xy_loss_type="l2",
                       angle_loss_type="l2", gamma=2.0, num_bins=2, iou=None, batch_size=None):
    """The fused terms of PointPillarUncertaintyLoss: what det_loss_supported asks of the maps, labels, gamma, num_bins, iou and
    batch_size, a CUDA fp32 unc_preds [N, dim*A, H, W] on the same device, dim in {2, 3, 7}, xy_loss_type l2 | l1 and
    angle_loss_type l2 | von-mise (heal_unc_loss_supported).  HEAL_LOSS_FUSED=0 forces the composition."""
    if not det_loss_supported(cls_preds, reg_preds, dir_preds, pos_equal_one, neg_equal_one, targets, gamma=gamma,
                              num_bins=num_bins, iou=iou, batch_size=batch_size):
        return False
    N, A, H, W = (int(v) for v in cls_preds.shape)
    if xy_loss_type not in _UNC_XY or angle_loss_type not in _UNC_ANGLE or not isinstance(dim, int):
        return False
    return bool(_loss_map_ok(unc_preds) and unc_preds.device == cls_preds.device and tuple(unc_preds.shape) == (N, dim * A, H, W)
                and _capi.lib().heal_unc_loss_supported(A, dim, _UNC_XY[xy_loss_type], _UNC_ANGLE[angle_loss_type],
                                                        int(dir_preds is not None))
                and _capi.query("heal_unc_loss_workspace", N, A, H, W) > 0)


def unc_loss(cls_preds, reg_preds, unc_preds, dir_preds, pos_equal_one, neg_equal_one, targets, pos_cls_weight, alpha, sigma,
             weights, dim, xy_loss_type="l2", angle_loss_type="l2", angle_weight=1.0, lambda_V=1.0, s0=1.0, limit_period=False,
             anchor_yaw=None, dir_offset=0.0, need_grad=True, grad_out=None):
    """UL.  PointPillarUncertaintyLoss's four terms and their gradients in one pass (heal_unc_loss): det_loss's maps and labels
    plus unc_preds [N, dim*A, H, W]; weights = (cls, reg, unc, dir) loss weights; dim, the loss types and angle_weight, lambda_V,
    s0, limit_period are the `uncertainty` block's.  -> (terms [4] = cls, reg, unc, dir loss, each x weight / N,
    (grad_cls, grad_reg, grad_unc, grad_dir) | None); grad_reg carries the reg term's and the unc term's gradient.
    need_grad: bool or one per map; False passes NULL gradients: the kernels only read.  grad_out: buffers to write into."""
    who = "unc_loss"
    dim = int(dim)
    maps, (pos, neg, tgt), (N, A, H, W), yaw, grads, moved = _anchor_head_inputs(
        who, (("cls_preds", cls_preds), ("reg_preds", reg_preds), ("unc_preds", unc_preds), ("dir_preds", dir_preds)),
        (("pos_equal_one", pos_equal_one), ("neg_equal_one", neg_equal_one), ("targets", targets)), dim, anchor_yaw, weights, sigma,
        need_grad, grad_out)
    if xy_loss_type not in _UNC_XY or angle_loss_type not in _UNC_ANGLE:
        raise _capi.HealAmdError(f"{who}: xy_loss_type {xy_loss_type!r} (l2 | l1), angle_loss_type {angle_loss_type!r} (l2 | von-mise)")
    nbytes, ws, terms = _loss_workspace(who, "unc_loss", "heal_unc_loss_workspace", (N, A, H, W), f"shape {(N, A, H, W)} is", 4,
                                        maps[0].device)
    with _Timed(f"unc_loss_a{A}_d{dim}", nbytes=moved):
        _capi.call("heal_unc_loss", *(_ptr(m) for m in maps), _ptr(pos), _ptr(neg), _ptr(tgt), int(pos.dtype == torch.float64),
                   N, A, H, W, dim, float(pos_cls_weight), float(alpha), float(sigma), *(float(w) for w in weights),
                   _UNC_XY[xy_loss_type], _UNC_ANGLE[angle_loss_type], float(angle_weight), float(lambda_V), float(s0),
                   int(bool(limit_period)), yaw, float(dir_offset), _ptr(terms), *(_ptr(g) for g in grads), _ptr(ws),
                   ctypes.c_size_t(nbytes), _stream())
    return terms, (tuple(grads) if any(g is not None for g in grads) else None)


def _unc_loss_total(*args, **cfg):
    """unc_loss for _FusedLoss: grad_reg is the sum of two terms' gradients (reg and unc), so the differentiable output is the
    TOTAL, added in the loss module's order (dir + ((reg + cls) + unc)); the four terms come along for the bookkeeping."""
    terms, grads = unc_loss(*args, **cfg)
    total = (terms[1] + terms[0]) + terms[2]
    return ((terms[3] + total if args[3] is not None else total), terms), grads


def unc_loss_terms(cls_preds, reg_preds, unc_preds, dir_preds, pos_equal_one, neg_equal_one, targets, **cfg):
    """The differentiable form of unc_loss: -> (total, terms [4] = cls, reg, unc, dir); the total carries the gradients for the
    maps that require one, the terms are detached."""
    return _loss_terms(_unc_loss_total, False, (cls_preds, reg_preds, unc_preds, dir_preds), pos_equal_one, neg_equal_one, targets,
                       **cfg)


def occ_loss_supported(occ_list, pos_equal_one, neg_equal_one, relative_downsample, gamma=2.0):
    """The fused occupancy term: 1..4 CUDA fp32 maps [N, 1, H // k_i, W // k_i] (the pooled label's shape) for labels [N, H, W, 2]
    float32 or float64 on the same device, gamma == 2.  Two anchors because the composition pools anchors 0 and 1 only.
    HEAL_LOSS_FUSED=0 forces the composition."""
    if (not loss_fused_enabled() or gamma != 2.0 or not isinstance(occ_list, (list, tuple))
            or not 1 <= len(occ_list) <= OCC_LOSS_MAX_LEVELS):
        return False
    if len(relative_downsample) < len(occ_list) or not all(_loss_map_ok(o) for o in occ_list):
        return False
    dev = occ_list[0].device
    if not _loss_labels_ok(dev, pos_equal_one, neg_equal_one) or pos_equal_one.dim() != 4 or pos_equal_one.shape != neg_equal_one.shape:
        return False
    N, H, W, A = (int(v) for v in pos_equal_one.shape)
    ks = [int(k) for k in relative_downsample[:len(occ_list)]]
    return bool(A == 2 and all(k >= 1 and H // k >= 1 and W // k >= 1 for k in ks)
                and all(o.device == dev and tuple(o.shape) == (N, 1, H // k, W // k) for o, k in zip(occ_list, ks))
                and _capi.query("heal_occ_loss_workspace", N, H, W, len(ks), ctypes.cast((ctypes.c_int * len(ks))(*ks), ctypes.c_void_p)) > 0)


def occ_loss(occ_list, pos_equal_one, neg_equal_one, relative_downsample, level_weight, pos_cls_weight, alpha, need_grad=True,
             grad_out=None):
    """DL.  The focal occupancy loss of every pyramid level in one pass: occ_list: 1..4 maps [N, 1, H // k_i, W // k_i] f32 cuda
    (made contiguous), labels [N, H, W, A] float32 or float64 read in place and pooled on the fly (foreground: any anchor of the
    k_i x k_i window positive, background: every one negative; floor mode).  -> (loss [1] = sum_i level_weight[i] / N * level sum,
    [d loss / d occ_i] | None).  need_grad: bool or one per level; False only reads."""
    who = "occ_loss"
    if not isinstance(occ_list, (list, tuple)) or not 1 <= len(occ_list) <= OCC_LOSS_MAX_LEVELS:
        raise _capi.HealAmdError(f"{who}: occ_list must hold 1..4 maps")
    L = len(occ_list)
    if len(relative_downsample) < L or len(level_weight) < L:
        raise _capi.HealAmdError(f"{who}: {L} levels need as many relative_downsample and level_weight entries")
    occ, (pos, neg) = _loss_inputs(who, [(f"occ_list[{i}]", o) for i, o in enumerate(occ_list)],
                                   (("pos_equal_one", pos_equal_one), ("neg_equal_one", neg_equal_one)))
    if pos.dim() != 4 or pos.shape != neg.shape or int(pos.shape[3]) > LOSS_MAX_ANCHORS:
        raise _capi.HealAmdError(f"{who}: labels {tuple(pos.shape)}, {tuple(neg.shape)} must be equal [N, H, W, A] with at most "
                                 f"{LOSS_MAX_ANCHORS} anchors")
    N, H, W, A = (int(v) for v in pos.shape)
    ks = [int(k) for k in relative_downsample[:L]]
    for i, (o, k) in enumerate(zip(occ, ks)):
        if k < 1 or tuple(o.shape) != (N, 1, H // max(k, 1), W // max(k, 1)):
            raise _capi.HealAmdError(f"{who}: occ_list[{i}] is {tuple(o.shape)}, the labels pooled by {k} are {(N, 1, H // max(k, 1), W // max(k, 1))}")
    grads = _loss_grad_buffers(who, occ, need_grad, grad_out)
    k_arr = (ctypes.c_int * L)(*ks)
    w_arr = (ctypes.c_float * L)(*[float(v) for v in level_weight[:L]])
    o_arr = (ctypes.c_void_p * L)(*[o.data_ptr() for o in occ])
    g_arr = (ctypes.c_void_p * L)(*[g.data_ptr() if g is not None else None for g in grads])
    nbytes, ws, loss = _loss_workspace(who, "occ_loss", "heal_occ_loss_workspace", (N, H, W, L, ctypes.cast(k_arr, ctypes.c_void_p)),
                                       f"labels {(N, H, W, A)} with levels {ks} are", 1, pos.device)
    moved = sum(4.0 * o.numel() for o in occ) + sum(4.0 * g.numel() for g in grads if g is not None) \
        + float(pos.element_size()) * 2 * pos.numel() * (L + 1)
    with _Timed(f"occ_loss_l{L}", nbytes=moved):
        _capi.call("heal_occ_loss", ctypes.cast(o_arr, ctypes.c_void_p), _ptr(pos), _ptr(neg), int(pos.dtype == torch.float64), N, A,
                   H, W, L, ctypes.cast(k_arr, ctypes.c_void_p), ctypes.cast(w_arr, ctypes.c_void_p), float(pos_cls_weight),
                   float(alpha), _ptr(loss), ctypes.cast(g_arr, ctypes.c_void_p), _ptr(ws), ctypes.c_size_t(nbytes), _stream())
    return loss, (grads if any(g is not None for g in grads) else None)


def occ_loss_term(occ_list, pos_equal_one, neg_equal_one, **cfg):
    """occ_loss under autograd: -> the 0-d loss, gradients for the levels that require one."""
    return _FusedLoss.apply(lambda need: occ_loss(list(occ_list), pos_equal_one, neg_equal_one, need_grad=need, **cfg), False,
                            tuple(_wants_grad(o) for o in occ_list), *occ_list)


def depth_focal_loss_supported(depth_logit, depth_gt_indices, fg_mask=None, gamma=2.0, smooth_target=False):
    """The fused depth-bin term: CUDA fp32 logits [M, D, h, w], int64 target indices [M, h, w] and an optional float32 mask of
    that shape on the same device, gamma == 2, smooth_target off.  HEAL_LOSS_FUSED=0 forces the composition."""
    if not loss_fused_enabled() or gamma != 2.0 or smooth_target or not _loss_map_ok(depth_logit):
        return False
    M, D, h, w = (int(v) for v in depth_logit.shape)
    dev = depth_logit.device
    if not (isinstance(depth_gt_indices, torch.Tensor) and depth_gt_indices.device == dev and depth_gt_indices.dtype == torch.int64
            and tuple(depth_gt_indices.shape) == (M, h, w)):
        return False
    if fg_mask is not None and not (isinstance(fg_mask, torch.Tensor) and fg_mask.device == dev and fg_mask.dtype == torch.float32
                                    and tuple(fg_mask.shape) == (M, h, w)):
        return False
    return _capi.query("heal_depth_focal_loss_workspace", M, D, h, w) > 0


def depth_focal_loss(depth_logit, depth_gt_indices, fg_mask=None, alpha=0.25, weight=1.0, need_grad=True, grad_out=None):
    """DL.  depth_logit [M, D, h, w] f32 cuda (made contiguous), depth_gt_indices [M, h, w] int64, fg_mask [M, h, w] f32 | None ->
    (loss [1], grad | None): weight x the mean over M*h*w of -alpha (1 - p_g)^2 log p_g (x 3.25 where the mask is > 0, 0.25
    where it is 0), p the channel softmax, and its gradient.  A target index outside [0, D) contributes 0 and receives an all-zero
    gradient; the reference's one_hot raises there.  need_grad=False only reads."""
    who = "depth_focal_loss"
    (depth_logit,), _ = _loss_inputs(who, (("depth_logit", depth_logit),), ())
    M, D, h, w = (int(v) for v in depth_logit.shape)
    dev = depth_logit.device
    if (not isinstance(depth_gt_indices, torch.Tensor) or depth_gt_indices.device != dev or depth_gt_indices.dtype != torch.int64
            or tuple(depth_gt_indices.shape) != (M, h, w)):
        raise _capi.HealAmdError(f"{who}: depth_gt_indices must be int64 {(M, h, w)} on {dev}")
    if fg_mask is not None and (not isinstance(fg_mask, torch.Tensor) or fg_mask.device != dev or fg_mask.dtype != torch.float32
                                or tuple(fg_mask.shape) != (M, h, w)):
        raise _capi.HealAmdError(f"{who}: fg_mask must be float32 {(M, h, w)} on {dev}")
    idx = depth_gt_indices.contiguous()
    mask = fg_mask.detach().contiguous() if fg_mask is not None else None
    (grad,) = _loss_grad_buffers(who, (depth_logit,), bool(need_grad), None if grad_out is None else (grad_out,))
    nbytes, ws, loss = _loss_workspace(who, "depth_focal_loss", "heal_depth_focal_loss_workspace", (M, D, h, w),
                                       f"shape {(M, D, h, w)} is", 1, dev)
    moved = 4.0 * depth_logit.numel() * (2 if grad is not None else 1) + 8.0 * idx.numel() + (4.0 * idx.numel() if mask is not None else 0)
    with _Timed(f"depth_focal_loss_d{D}", nbytes=moved):
        _capi.call("heal_depth_focal_loss", _ptr(depth_logit), _ptr(idx), _ptr(mask), M, D, h, w, float(alpha), float(weight),
                   _ptr(loss), _ptr(grad), _ptr(ws), ctypes.c_size_t(nbytes), _stream())
    return loss, grad


def depth_focal_loss_term(depth_logit, depth_gt_indices, fg_mask=None, alpha=0.25, weight=1.0):
    """depth_focal_loss under autograd: -> the 0-d loss; the indices and the mask receive no gradient."""
    return _FusedLoss.apply(lambda need: depth_focal_loss(depth_logit, depth_gt_indices, fg_mask, alpha, weight, need_grad=need[0]),
                            False, (_wants_grad(depth_logit),), depth_logit)


# ------------------------------------------------------------------------------------------------ CP
# The anchor-free centre head (csrc/center_head.hip, the front end in csrc/decode_nms.hip; include/heal_amd_center.h): the
# criterion with its target assignment, the box map and decode + NMS.  HEAL_LOSS_FUSED=0 forces the torch composition of
# heal_amd/opencood/loss/center_point_loss.py (scripts/center_bench.py).
CENTER_MAX_OBJS = _limit("HEAL_CENTER_MAX_OBJS", _capi.HEADER_CENTER)
CENTER_MAX_BATCH = _limit("HEAL_CENTER_MAX_BATCH", _capi.HEADER_CENTER)


def _doubles(values, n, name, who):
    values = [float(v) for v in values]
    if len(values) != n:
        raise _capi.HealAmdError(f"{who}: {name} must have {n} values, got {len(values)}")
    return (ctypes.c_double * n)(*values)


def _center_shapes(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask):
    """(B, Mmax, H, W) of a centre-head problem, or None where the tensors are not one: CUDA fp32 maps [B, 1, H, W] and [B, 8, H, W],
    boxes [B, Mmax, 7] (floating point) and mask [B, Mmax] on the same device."""
    if not (_loss_map_ok(cls_preds) and _loss_map_ok(bbox_preds)):
        return None
    B, A, H, W = (int(v) for v in cls_preds.shape)
    dev = cls_preds.device
    if A != 1 or tuple(bbox_preds.shape) != (B, 8, H, W) or bbox_preds.device != dev:
        return None
    if not (isinstance(object_bbx_center, torch.Tensor) and isinstance(object_bbx_mask, torch.Tensor)
            and object_bbx_center.device == dev and object_bbx_mask.device == dev and object_bbx_center.is_floating_point()
            and object_bbx_center.dim() == 3 and int(object_bbx_center.shape[0]) == B and int(object_bbx_center.shape[2]) == 7
            and tuple(object_bbx_mask.shape) == tuple(object_bbx_center.shape[:2]) and object_bbx_center.shape[1] >= 1):
        return None
    return B, int(object_bbx_center.shape[1]), H, W


def center_loss_supported(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask, cav_lidar_range, voxel_size,
                          out_size_factor, max_objs):
    """The fused CenterPointLoss: CUDA fp32 maps [B, 1, H, W] and [B, 8, H, W] with (H, W) the feature map of the range, the voxel
    size and the factor, boxes [B, Mmax, 7] and mask [B, Mmax] on the same device, max_objs <= CENTER_MAX_OBJS
    (heal_center_loss_supported).  HEAL_LOSS_FUSED=0 forces the composition."""
    if not loss_fused_enabled():
        return False
    shapes = _center_shapes(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask)
    if shapes is None or len(cav_lidar_range) != 6 or len(voxel_size) != 3:
        return False
    B, Mmax, H, W = shapes
    return bool(_capi.query("heal_center_loss_supported", B, Mmax, H, W, _doubles(cav_lidar_range, 6, "cav_lidar_range", "center_loss"),
                            _doubles(voxel_size, 3, "voxel_size", "center_loss"), int(out_size_factor), int(max_objs)))


def center_loss(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask, cav_lidar_range, voxel_size, out_size_factor, max_objs,
                min_radius, gaussian_overlap, code_weights, cls_weight, loc_weight, need_grad=True, grad_out=None, debug=False,
                workspace=None):
    """CP.  CenterPointLoss.forward, target assignment included, in one call: cls_preds [B, 1, H, W], bbox_preds [B, 8, H, W] f32
    cuda (made contiguous); object_bbx_center [B, Mmax, 7] (cast to float32 as the reference does) and object_bbx_mask [B, Mmax]
    (cast to int32) stay on the device.  -> (terms [2] = cls, reg loss, (grad_cls, grad_bbox) | None), with debug=True also a
    dict of the assigned targets: heatmap [B, 1, H, W], anno_boxes [B, max_objs, 8], inds [B, max_objs] int64, masks
    [B, max_objs] uint8.  need_grad: bool or one per map; False passes NULL gradients.  grad_out: buffers to write into.
    workspace: a uint8 buffer to use instead of the operator's own (the tests hand in a poisoned one)."""
    who = "center_loss"
    shapes = _center_shapes(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask)
    if shapes is None:
        raise _capi.HealAmdError(f"{who}: needs CUDA/HIP f32 maps [B, 1, H, W] and [B, 8, H, W], boxes [B, Mmax, 7] and a mask "
                                 "[B, Mmax] on the same device (heal_amd has no CPU path)")
    B, Mmax, H, W = shapes
    (cls_preds, bbox_preds), _ = _loss_inputs(who, (("cls_preds", cls_preds), ("bbox_preds", bbox_preds)), ())
    dev = cls_preds.device
    boxes = object_bbx_center.detach().to(torch.float32).contiguous()
    mask = object_bbx_mask.detach().to(torch.int32).contiguous()
    rng, vox = _doubles(cav_lidar_range, 6, "cav_lidar_range", who), _doubles(voxel_size, 3, "voxel_size", who)
    cw = _doubles(code_weights, 8, "code_weights", who)
    max_objs = int(max_objs)
    if not _capi.query("heal_center_loss_supported", B, Mmax, H, W, rng, vox, int(out_size_factor), max_objs):
        raise _capi.HealAmdError(f"{who}: maps {(B, H, W)} with max_objs {max_objs} (<= {CENTER_MAX_OBJS}) are out of range, or "
                                 "(H, W) is not the feature map of cav_lidar_range / voxel_size / out_size_factor")
    grads = _loss_grad_buffers(who, (cls_preds, bbox_preds), need_grad, grad_out)
    nbytes, ws, terms = _loss_workspace(who, "center_loss", "heal_center_loss_workspace", (B, H, W, max_objs),
                                        f"maps {(B, H, W)} with max_objs {max_objs} are", 2, dev, given=workspace)
    dbg = None
    if debug:
        dbg = {"heatmap": torch.empty((B, 1, H, W), dtype=torch.float32, device=dev),
               "anno_boxes": torch.empty((B, max_objs, 8), dtype=torch.float32, device=dev),
               "inds": torch.empty((B, max_objs), dtype=torch.int64, device=dev),
               "masks": torch.empty((B, max_objs), dtype=torch.uint8, device=dev)}
    opt = (lambda k: _ptr(dbg[k])) if dbg is not None else (lambda k: ctypes.c_void_p(0))
    moved = 4.0 * (cls_preds.numel() + bbox_preds.numel()) + sum(4.0 * g.numel() for g in grads if g is not None) \
        + 4.0 * (boxes.numel() + mask.numel())
    with _Timed("center_loss", nbytes=moved):
        _capi.call("heal_center_loss", _ptr(cls_preds), _ptr(bbox_preds), _ptr(boxes), _ptr(mask), B, Mmax, H, W, rng, vox,
                   int(out_size_factor), max_objs, int(min_radius), float(gaussian_overlap), cw, float(cls_weight),
                   float(loc_weight), _ptr(terms), _ptr(grads[0]), _ptr(grads[1]), opt("heatmap"), opt("anno_boxes"), opt("inds"),
                   opt("masks"), _ptr(ws), ctypes.c_size_t(nbytes), _stream())
    grads = tuple(grads) if any(g is not None for g in grads) else None
    return (terms, grads, dbg) if debug else (terms, grads)


def center_loss_terms(cls_preds, bbox_preds, object_bbx_center, object_bbx_mask, **cfg):
    """The differentiable form of center_loss: -> terms [2] (cls, reg), gradients for the maps that require one; the boxes and the
    mask receive none."""
    return _loss_terms(center_loss, True, (cls_preds, bbox_preds), object_bbx_center, object_bbx_mask, **cfg)


def center_boxes(bbox_preds, cav_lidar_range, voxel_size, out_size_factor):
    """CP.  generate_predicted_boxes: bbox_preds [B, 8, H, W] f32 cuda -> reg_preds [B, H*W, 7] = (x, y, z, h, w, l, yaw) in
    metres, one streaming launch.  No gradient flows through it (the criterion reads bbox_preds): the input is detached."""
    who = "center_boxes"
    if not _loss_map_ok(bbox_preds) or int(bbox_preds.shape[1]) != 8:
        raise _capi.HealAmdError(f"{who}: bbox_preds must be a CUDA/HIP f32 map [B, 8, H, W] (heal_amd has no CPU path; the "
                                 "reference's reshape only lines up for anchor_number 1)")
    x = bbox_preds.detach().contiguous()
    B, _, H, W = (int(v) for v in x.shape)
    out = torch.empty((B, H * W, 7), dtype=torch.float32, device=x.device)
    with _Timed("center_boxes", nbytes=4.0 * (x.numel() + out.numel()), kernel_events=True):
        _capi.call("heal_center_boxes", _ptr(x), B, H, W, _doubles(cav_lidar_range, 6, "cav_lidar_range", who),
                   _doubles(voxel_size, 3, "voxel_size", who), int(out_size_factor), _ptr(out), _stream())
    return out


def center_decode_nms(cls, boxes, dirp, score_thr, dir_offset, num_bins, nms_thr, tfm, gt_range, nms_top=1000, sync=True):
    """K8 for the centre head.  cls [1,1,H,W] (or [1,H,W]), boxes [1,H*W,7] (or [H*W,7]: the 3-D reg_preds), dirp
    [1,bins,H,W] or None, f32 cuda.  -> as decode_nms."""
    who = "center_decode_nms"
    cls = _need(cls, torch.float32, "cls_preds")
    boxes = _need(boxes, torch.float32, "reg_preds")
    if dirp is not None:
        dirp = _need(dirp, torch.float32, "dir_preds")
    if cls.dim() == 4:
        if cls.shape[0] != 1:
            raise _capi.HealAmdError(f"{who}: batch size must be 1 (voxel_postprocessor.py:314)")
        cls = cls[0]
        dirp = dirp[0] if dirp is not None else None
    if boxes.dim() == 3:
        if boxes.shape[0] != 1:
            raise _capi.HealAmdError(f"{who}: batch size must be 1 (voxel_postprocessor.py:314)")
        boxes = boxes[0]
    A, H, W = (int(v) for v in cls.shape)
    if A != 1 or tuple(boxes.shape) != (H * W, 7):
        raise _capi.HealAmdError(f"{who}: scores {tuple(cls.shape)} and boxes {tuple(boxes.shape)} are not [1, H, W] and "
                                 "[H*W, 7] (one box per cell: anchor_number 1)")
    if dirp is not None and tuple(dirp.shape) != (int(num_bins), H, W):
        raise _capi.HealAmdError(f"{who}: dir_preds {tuple(dirp.shape)} is not [{int(num_bins)}, {H}, {W}]")
    dev = cls.device
    out_c = torch.empty((nms_top, 8, 3), dtype=torch.float32, device=dev)
    out_s = torch.empty((nms_top,), dtype=torch.float32, device=dev)
    out_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    nbytes = _capi.query("heal_decode_nms_workspace", H * W, int(nms_top))
    ws = _workspace("decode_nms", nbytes, dev)
    t = _host_array([float(v) for v in np.asarray(tfm, dtype=np.float32).reshape(-1)], ctypes.c_float)
    g = _host_array([float(v) for v in gt_range], ctypes.c_float)
    with _Timed("center_decode_nms"):
        _capi.call("heal_center_decode_nms", _ptr(cls), _ptr(boxes), _ptr(dirp), H, W, int(num_bins), float(score_thr),
                   float(dir_offset), float(nms_thr), int(nms_top), t, g, _ptr(out_c), _ptr(out_s), _ptr(out_n), int(nms_top),
                   _ptr(ws), ws.numel(), _stream())
    _remember("center_decode_nms", lambda: center_decode_nms(cls, boxes, dirp, score_thr, dir_offset, num_bins, nms_thr, tfm,
                                                             gt_range, nms_top, sync=False))
    if not sync:
        return out_c, out_s, out_n
    k = int(out_n.item())
    if k == 0:
        return None, None
    return out_c[:k], out_s[:k]


# ------------------------------------------------------------------------------------------------ K6c
def ln_stats(x, eps):
    """(mean, rstd) of every token of x [..., C] -> [T, 2] f32: the statistics half of a LayerNorm whose application is
    folded into the consuming heal_linear."""
    x = _need(x, torch.float32, "x")
    C = int(x.shape[-1])
    T = x.numel() // C
    stats = torch.empty((T, 2), dtype=torch.float32, device=x.device)
    _capi.call("heal_ln_stats", _ptr(x), T, C, float(eps), _ptr(stats), _stream())
    return stats


def linear_supported(n_tokens, n_in, n_out):
    return n_out % 128 == 0 and n_in % 32 == 0 and n_in >= 32 and n_tokens > 0


_ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2}


def linear(x, weight, bias=None, stats=None, act=None, residual=None, out=None, row_map=None, parts=1, colscale=None,
           colscale_part=0, group_rows=0, bias_per_group=False, x_parts=1):
    """heal_linear: out = act(norm(x) W^T * colscale + bias) + residual on the fp32 matrix cores.
    x [T, K] (any leading dims, contiguous), weight [N, K] (nn.Linear layout), stats from ln_stats() (gamma / beta already folded
    into weight / bias), row_map = (inner, outer): token t is written to row (t % inner) * outer + t // inner, parts: the N
    columns are split into `parts` equal column blocks written to out[p] -> returns [parts, T, N / parts] (parts > 1) or [T, N]."""
    x = _need(x, torch.float32, "x")
    weight = _need(weight, torch.float32, "weight")
    # x_parts > 1: x is [x_parts, T, K / x_parts] -- the reduction runs over the channel blocks of several tensors (the three
    # window-attention branches feeding the merged to_out projection) without a concatenated copy
    xk = int(x.shape[-1])
    K = xk * int(x_parts)
    T = x.numel() // K
    N = int(weight.shape[0])
    if int(weight.shape[1]) != K or not linear_supported(T, K, N) or N % parts or (N // parts) % 4:
        raise _capi.HealAmdError(f"linear: unsupported shape T={T} K={K} N={N} parts={parts}")
    pc = N // parts
    if out is None:
        out = torch.empty((parts, T, pc) if parts > 1 else (T, N), dtype=torch.float32, device=x.device)
    inner, outer = (int(row_map[0]), int(row_map[1])) if row_map is not None else (0, 0)
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
    with _Timed(f"linear_{K}_{N}", flops=2.0 * T * K * N, kernel_events=True):
        _capi.call("heal_linear", _ptr(x), xk, xk if x_parts > 1 else 0, T * xk, _optr(stats), _ptr(weight), _optr(bias),
                   int(bool(bias_per_group)),
                   _optr(colscale), int(colscale_part), int(group_rows), _optr(residual), N if residual is not None else 0,
                   _ptr(out), pc, T, N, K, inner, outer, pc, T * pc, _ACT[act], _stream())
    return out


def split_attn_weights(branches, groups, rows_per_group, w_out, b_out, fc1, ln_g, ln_b, eps, fc2):
    """branches [3, groups * rows_per_group, C] (window attention outputs before to_out) -> (scale [groups,3,C], bias [groups,C])."""
    branches = _need(branches, torch.float32, "branches")
    C = int(branches.shape[-1])
    dev = branches.device
    ws = _workspace("split_attn", _capi.query("heal_split_attn_workspace", groups, rows_per_group, C), dev)
    scale = torch.empty((groups, 3, C), dtype=torch.float32, device=dev)
    bias = torch.empty((groups, C), dtype=torch.float32, device=dev)
    _capi.call("heal_split_attn_weights", _ptr(branches), int(branches.stride(0)), groups, rows_per_group, C, _ptr(w_out),
               _ptr(b_out), _ptr(fc1), _ptr(ln_g), _ptr(ln_b), float(eps), _ptr(fc2), _ptr(ws), _ptr(scale), _ptr(bias),
               _stream())
    return scale, bias


def split_attn_colsum(branches, groups, rows_per_group):
    """First half of split_attn_weights for tokens spread over ranks: [groups, 3, ceil(rows / 512), C] per-chunk column sums of
    the local tokens of branches [3, groups * rows_per_group, C] (a fresh tensor: it is handed to a collective)."""
    branches = _need(branches, torch.float32, "branches")
    C = int(branches.shape[-1])
    out = torch.empty((groups, 3, (rows_per_group + 511) // 512, C), dtype=torch.float32, device=branches.device)
    _capi.call("heal_split_attn_colsum", _ptr(branches), int(branches.stride(0)), groups, rows_per_group, C, _ptr(out), _stream())
    return out


def split_attn_weights_from_colsum(colsum, rows_per_part, w_out, b_out, fc1, ln_g, ln_b, eps, fc2):
    """Second half: colsum [n_parts, groups, 3, chunks, C] (the all-gathered halves) -> (scale [groups,3,C], bias [groups,C])."""
    colsum = _need(colsum, torch.float32, "colsum")
    n_parts, groups, _three, chunks, C = (int(v) for v in colsum.shape)
    if chunks != (rows_per_part + 511) // 512:
        raise ValueError(f"split_attn_weights_from_colsum: {chunks} chunks do not match {rows_per_part} rows per part")
    dev = colsum.device
    scale = torch.empty((groups, 3, C), dtype=torch.float32, device=dev)
    bias = torch.empty((groups, C), dtype=torch.float32, device=dev)
    _capi.call("heal_split_attn_weights_from_colsum", _ptr(colsum), n_parts, groups, int(rows_per_part), C, _ptr(w_out),
               _ptr(b_out), _ptr(fc1), _ptr(ln_g), _ptr(ln_b), float(eps), _ptr(fc2), _ptr(scale), _ptr(bias), _stream())
    return scale, bias


# ------------------------------------------------------------------------------------------------ K7
def grouped16_fragments(weight, cg):
    """[C, cg, 3, 3] grouped weight (cg = 16 | 8) -> MFMA A fragments of the 16-channel super-groups
    [C/16][tap][ks][lane] (block-diagonal zero padding for cg = 8)."""
    def build():
        C = int(weight.shape[0])
        w = weight.detach().reshape(C // 16, 16, cg, 9)                   # [sg, co, ci_in_group, tap]
        if cg == 16:
            full = w
        else:                                                             # two groups of 8: rows 0-7 use ci 0-7, rows 8-15 ci 8-15
            full = torch.zeros((C // 16, 16, 16, 9), dtype=w.dtype, device=w.device)
            full[:, :8, :8] = w[:, :8]
            full[:, 8:, 8:] = w[:, 8:]
        # [sg, co(ln), ks, lk, tap] -> [sg, tap, ks, lk, ln]
        return full.reshape(C // 16, 16, 4, 4, 9).permute(0, 4, 2, 3, 1).contiguous()
    return _derived("grouped16_fragments", (weight,), build)


def grouped_small_fragments(weight, cg):
    """[C, cg, 3, 3] grouped weight (cg = 4 | 8 | 16) -> weight operands of heal_grouped_small_conv3x3: [C/16][tap][ci][16 output channels
    of the super-group]."""
    C = int(weight.shape[0])
    return _derived("grouped_small_fragments", (weight,),
                    lambda: weight.detach().reshape(C // 16, 16, cg, 9).permute(0, 3, 2, 1).contiguous())   # [sg, tap, ci, co]


def pyramid_roi_enabled():
    """HEAL_PYRAMID_ROI (default on; the library reads it, heal_roi_enabled): may the fusion pyramid's lean walk run a stage with
    per-image regions of interest?  Asked at every call."""
    return bool(_capi.query("heal_roi_enabled"))


def conv1x1_box_tiles(box, Ho, Wo):
    """Host mirror of heal_conv1x1_box_roi's tiles for one image (include/heal_amd_roi.h): int64 [tiles, 64], row t the flattened
    output pixels y * Wo + x that workgroup tile t computes and writes, in the kernel's order; -1 where the last tile reaches behind
    the box.  tiles = ceil(bw * bh / 64) of the image's ceil(Ho * Wo / 64); an empty box has none.  Wo % 4 == 0."""
    y0, y1, x0, x1 = (int(v) for v in box)
    if Wo % 4:
        raise ValueError("the box rule needs an output width that is a multiple of 4")
    if y0 >= y1 or x0 >= x1:
        return np.zeros((0, 64), dtype=np.int64)
    xa, xb = x0 // 4 * 4, -(-x1 // 4) * 4
    bw, npix = xb - xa, (xb - xa) * (y1 - y0)
    q = np.arange(-(-npix // 64) * 64, dtype=np.int64)
    return np.where(q < npix, (y0 + q // bw) * Wo + xa + q % bw, -1).reshape(-1, 64)


def _roi_table(roi, n, Ho, Wo, who):
    """Per-image output boxes [(y0, y1, x0, x1)] * n -> the host int32 [n, 4] array of the *_roi entry points (keep it alive over the
    call).  The table travels by value in the kernel arguments: under graph capture the boxes are constants of the graph."""
    t = np.ascontiguousarray(np.asarray(roi, dtype=np.int64).reshape(-1, 4))
    if t.shape[0] != n or n > WARP_MAX_AGENTS:
        raise _capi.HealAmdError(f"{who}: a ROI needs one (y0, y1, x0, x1) box for each of the {n} images, at most {WARP_MAX_AGENTS}")
    if (t < 0).any() or (t[:, :2] > Ho).any() or (t[:, 2:] > Wo).any():
        raise _capi.HealAmdError(f"{who}: ROI box outside the {Ho} x {Wo} output map: {t.tolist()}")
    return np.ascontiguousarray(t.astype(np.int32))


def grouped_conv3x3(x, weight, bias, groups, stride=1, relu=True, roi=None):
    """32-group 3x3 conv (padding 1, stride 1 | 2) with fused bias + ReLU.  x [n,C,H,W], weight [C,C/groups,3,3].  4, 8 or 16
    channels per group run on the 16-block 4x4x1 MFMA (heal_grouped_small_conv3x3; measured 5 agents, us: 128 ch 256^2 166 ->
    98, 256 ch 128^2 84 -> 59, 512 ch 64^2 78 -> 49, stride 2: 256 ch 256^2 207 -> 107, 512 ch 128^2 122 -> 68);
    HEAL_GCONV_MFMA=16 | 8 selects the older 16x16x4 kernel (one m-tile per 16-channel group: 53 us; pairs of 8-channel groups
    with block-diagonal weights: 98 us), =0 the vector-ALU stencil, which also takes the shapes the MFMA kernels do not.
    roi: per-image output boxes [(y0, y1, x0, x1)] * n (heal_grouped_small_conv3x3_roi): tiles that hold no pixel of their image's
    box are not computed and their part of the result is UNINITIALISED memory; the other kernels compute the whole map."""
    x = _need(x, torch.float32, "x")
    weight = _need(weight, torch.float32, "weight")
    n, C, H, W = (int(v) for v in x.shape)
    bias = _need_bias(bias, C, "grouped_conv3x3")
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    y = _out_or_empty(None, (n, C, Ho, Wo), x.device, "grouped_conv3x3")
    cg = C // groups
    mode = switches.get("HEAL_GCONV_MFMA")
    if C % 16 == 0 and W % 4 == 0 and Wo % 4 == 0 and mode in ("1", "s") and cg in (4, 8, 16):
        frag = grouped_small_fragments(weight, cg)
        table = _roi_table(roi, n, Ho, Wo, "grouped_conv3x3") if roi is not None else None
        with _Timed(f"grouped_conv3x3_c{C}" + ("_s2" if stride == 2 else ""), 2.0 * 9 * n * C * cg * Ho * Wo,
                    4.0 * n * C * (H * W + Ho * Wo), kernel_events=True):
            if table is not None:
                _capi.call("heal_grouped_small_conv3x3_roi", _ptr(x), _ptr(frag), _ptr(bias), n, C, cg, H, W, int(stride),
                           int(bool(relu)), ctypes.c_void_p(table.ctypes.data), _ptr(y), _stream())
            else:
                _capi.call("heal_grouped_small_conv3x3", _ptr(x), _ptr(frag), _ptr(bias), n, C, cg, H, W, int(stride),
                           int(bool(relu)), _ptr(y), _stream())
        return y
    if stride == 1 and C % 16 == 0 and W % 4 == 0 and ((cg == 16 and mode != "0") or (cg == 8 and mode == "8")):   # mode "16" | "8"
        frag = grouped16_fragments(weight, cg)
        with _Timed(f"grouped_conv3x3_c{C}", 2.0 * 9 * n * C * cg * Ho * Wo, 4.0 * n * C * (H * W + Ho * Wo)):
            _capi.call("heal_grouped16_conv3x3", _ptr(x), _ptr(frag), _ptr(bias), n, C, H, W, int(bool(relu)), _ptr(y),
                       _stream())
        return y
    with _Timed(f"grouped_conv3x3_c{C}" + ("_s2" if stride == 2 else ""), 2.0 * 9 * n * C * (C // groups) * Ho * Wo,
                4.0 * n * C * (H * W + Ho * Wo)):
        _capi.call("heal_grouped_conv3x3", _ptr(x), _ptr(weight), _ptr(bias), n, C, int(groups), H, W, int(stride),
                   int(bool(relu)), _ptr(y), _stream())
    return y


def gconv_conv3_supported(width, cg, cout, H, W):
    return bool(_capi.query("heal_gconv_conv3_supported", int(width), int(cg), int(cout), int(H), int(W)))


def gconv_conv3(x, w2, b2, groups, w3, b3, residual=None, relu=True):
    """Back half of a ResNeXt bottleneck in one kernel: y = act(conv1x1(relu(gconv3x3(x, w2) + b2), w3) + b3 (+ residual)); the 2C-wide
    intermediate never reaches HBM.  x [n, width, H, W], w2 [width, width / groups, 3, 3], w3 [cout, width, 1, 1]."""
    x = _need(x, torch.float32, "x")
    n, width, H, W = (int(v) for v in x.shape)
    cg = width // groups
    cout = int(w3.shape[0])
    frag2 = grouped_small_fragments(_need(w2, torch.float32, "w2"), cg)
    frag3 = _derived("gconv_conv3_fragments", (w3,), lambda: mfma_a_fragments(w3.detach().reshape(cout, width)))
    y = torch.empty((n, cout, H, W), dtype=torch.float32, device=x.device)
    flops = 2.0 * n * H * W * (9 * width * cg + width * cout)
    nbytes = 4.0 * n * H * W * (width + cout * (2 if residual is not None else 1))
    with _Timed(f"gconv_conv3_{width}_{cout}", flops, nbytes, kernel_events=True):
        _capi.call("heal_gconv_conv3", _ptr(x), _ptr(frag2), _ptr(_need(b2, torch.float32, "b2")), _ptr(frag3),
                   _ptr(_need(b3, torch.float32, "b3")), _optr(residual), n, width, cg, cout, H, W, int(bool(relu)), _ptr(y), _stream())
    return y


def bias_act_(x, bias=None, residual=None, relu=True):
    """In place: x = act(x + bias[c] + residual).  x [n,C,H,W] contiguous f32 cuda."""
    x = _need(x, torch.float32, "x")
    n, C = int(x.shape[0]), int(x.shape[1])
    HW = int(x.shape[2] * x.shape[3])
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
    _capi.call("heal_bias_act", _ptr(x), _ptr(bias), _ptr(residual), n, C, HW, int(bool(relu)), _stream())
    return x


def mfma_a_fragments(wm):
    """[M,K] matrix -> MFMA 16x16x4 A-fragment order [M/16, K/4, 64]: frag[mt][ks][lane] =
    wm[mt*16 + (lane & 15)][ks*4 + (lane >> 4)]."""
    M, K = wm.shape
    return wm.reshape(M // 16, 16, K // 4, 4).permute(0, 2, 3, 1).reshape(M // 16, K // 4, 64).contiguous()


def conv1x1_fragments(w):
    """MFMA A-fragment layout of a [Cout,Cin,1,1] (or [Cout,Cin]) weight, zero-padded to [ceil64(Cout), ceil32(Cin)]."""
    def build():
        cout, cin = int(w.shape[0]), int(w.shape[1])
        mpad, kpad = (cout + 63) // 64 * 64, (cin + 31) // 32 * 32
        wm = w.detach().reshape(cout, cin)
        if (mpad, kpad) != (cout, cin):
            wm = torch.nn.functional.pad(wm, (0, kpad - cin, 0, mpad - cout))
        fr = mfma_a_fragments(wm)            # [M/16, K/4, 64] -> four k-steps per lane contiguous: [M/16, K/16, 64, 4]
        return fr.reshape(mpad // 16, kpad // 16, 4, 64).permute(0, 1, 3, 2).contiguous()
    return _derived("conv1x1_fragments", (w,), build)


def conv1x1_supported(cin, cout, hw, stride=1, out_w=None):
    """Shapes heal_conv1x1 takes: 16-byte pixel rows (stride 1: Ho*Wo % 4 == 0; stride 2: Wo % 4 == 0) and maps large
    enough to fill a few tiles."""
    if stride == 1:
        return hw % 4 == 0 and hw >= 64
    return stride == 2 and out_w is not None and out_w % 4 == 0 and hw >= 64


def conv1x1_ksplit(n, cin, cout, hw):
    """K splits for a stride-1 NCHW pointwise convolution: 1 unless the grid is small (< 128 blocks of 64 channels x 64 pixels)
    and the reduction deep (>= 8 chunks of 32 channels); then enough splits for ~256 blocks, at least 2 chunks each, none empty.
    HEAL_C1_KSPLIT forces a value (0 / 1: off)."""
    chunks = (cin + 31) // 32
    blocks = -(-cout // 64) * -(-hw // 64) * n
    want = switches.number("HEAL_C1_KSPLIT")
    if want is None:
        want = min(chunks // 2, max(2, 256 // blocks)) if blocks < 128 and chunks >= 8 else 1
    if want < 2 or chunks < 2 or hw % 4:
        return 1
    want = min(want, chunks, 65535 // n)
    return -(-chunks // -(-chunks // want))       # ceil(chunks / ceil(chunks / want)): no empty split


def stem7x7_fragments(w):
    """[64, cin, 7, 7] -> MFMA A-fragment order [4][ceil(cin * 49 / 4)][64] of heal_stem7x7."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if cout != 64 or tuple(w.shape[2:]) != (7, 7) or not 1 <= cin <= 4:
        raise _capi.HealAmdError(f"stem7x7: weight must be [64, 1..4, 7, 7], got {tuple(w.shape)}")

    def build():
        K = cin * 49
        ks = (K + 3) // 4
        wk = torch.nn.functional.pad(w.detach().to(torch.float32).reshape(64, K), (0, 4 * ks - K))      # [64, 4 ks]
        return wk.reshape(4, 16, ks, 4).permute(0, 2, 3, 1).contiguous()                                # [mt][ks][lk][ln]
    return _derived("stem7x7_fragments", (w,), build)


def stem7x7(x, w, bias, pool=True):
    """relu(conv7x7/2(x[:, :cin], w) + bias) (+ 3x3/2 max-pool) in one kernel; x [n, >= cin, H, W] is read in place (the first
    cin = w.shape[1] channels of every image).  -> [n, 64, Hp, Wp]."""
    x = _need(x, torch.float32, "x")
    n, cx, H, W = (int(v) for v in x.shape)
    cin = int(w.shape[1])
    if cx < cin:
        raise _capi.HealAmdError(f"stem7x7: input has {cx} channels, the weight wants {cin}")
    frag = stem7x7_fragments(w)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = ((Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1) if pool else (Hc, Wc)
    y = torch.empty((n, 64, Ho, Wo), dtype=torch.float32, device=x.device)
    with _Timed(f"stem7x7_{cin}" + ("_pool" if pool else ""), 2.0 * n * 64 * cin * 49 * Hc * Wc, kernel_events=True):
        _capi.call("heal_stem7x7", _ptr(x), cx * H * W, n, cin, H, W, _ptr(frag),
                   _ptr(_need_bias(bias, 64, "stem7x7")), int(bool(pool)), _ptr(y), _stream())
    return y


def conv1x1_tiled_ok(n, cin, cout, hw):
    """Shapes the 128 x 128 x 32 core (heal_conv1x1_tiled, 32x32x2 fp32 MFMA) takes over from heal_conv1x1: 32-channel K chunks,
    64- or 128-channel M tiles, enough blocks to fill the chip, and a reduction deep enough to be MFMA- rather than HBM-bound.
    OPT-IN (HEAL_C1_TILED=1, =force for every shape it can take): measured at the scenes' shapes (scripts/c1t_bench.py,
    profiles/r04_c1t_bench.json) it is at parity with the 64 x 64 kernel -- 0.70-1.07x, ahead only on 256 -> 2048 and single-image
    256 -> 128; neither tile shape of either kernel moves the 85-105 TFLOP/s these 5-GFLOP launches reach in isolation."""
    mode = switches.get("HEAL_C1_TILED")
    if mode == "0" or not experimental_build() or cin % 32 or cout % 64 or hw % 4 or hw < 128:
        return False
    bm = 128 if cout % 128 == 0 else 64
    blocks = (cout // bm) * -(-hw // 128) * n
    if mode == "force":
        return True
    return blocks >= 256 and cin >= 128


def arith_products():
    """HEAL_ARITH: "" / "f32" (default: exact-fp32 MFMA everywhere) | "bf16x6" | "bf16x9" -- the OPT-IN split-bf16 evaluation of the
    pointwise convolutions (heal_conv1x1_split; fp32 in / out / accumulate, 6 or 9 bf16 partial products per fp32 product)."""
    return {"bf16x6": 6, "bf16x9": 9}.get(switches.get("HEAL_ARITH"), 0)


def conv1x1_split_fragments(w):
    """[Cout, Cin(,1,1)] fp32 -> the three bf16 planes (w = h + m + l, round to nearest) in the fragment order of heal_conv1x1_split:
    [Cout/128][Cin/32][k16 step 2][row block 4][plane 3][lane 64][8] with element = W_p[128 ct + 32 rb + lane % 32][32 c + 16 s +
    8 (lane / 32) + e]."""
    def build():
        cout, cin = int(w.shape[0]), int(w.shape[1])
        wm = w.detach().reshape(cout, cin).to(torch.float32)
        h = wm.to(torch.bfloat16)
        r1 = wm - h.float()
        m = r1.to(torch.bfloat16)
        lo = (r1 - m.float()).to(torch.bfloat16)
        planes = torch.stack([h, m, lo], 0)                                    # [3, cout, cin]
        f = planes.reshape(3, cout // 128, 4, 32, cin // 32, 2, 2, 8)          # [p, ct, rb, li, c, s, kb, e]
        return f.permute(1, 4, 5, 2, 0, 6, 3, 7).contiguous()                  # [ct, c, s, rb, p, kb, li, e]
    return _derived("conv1x1_split_fragments", (w,), build)


def _w_rowmajor(w):
    w2 = w.detach().reshape(int(w.shape[0]), int(w.shape[1]))
    return w2 if w2.is_contiguous() else w2.contiguous()


def _out_or_empty(out, shape, device, who):
    """The caller's destination (a contiguous f32 tensor of exactly `shape`, e.g. a batch slice of a larger map) or a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous()):
        raise _capi.HealAmdError(f"{who}: `out` must be a contiguous f32 cuda tensor of shape {tuple(shape)}")
    return out


def _out_like(out, shape, device, who, name="out"):
    """_out_or_empty for a destination that must also lie on the operands' device (`name`: the argument in the message)."""
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != device):
        raise _capi.HealAmdError(f"{who}: `{name}` must be a contiguous f32 tensor of shape {tuple(shape)} on {device}")
    return _out_or_empty(out, shape, device, f"{who} ({name})" if name != "out" else who)


def conv1x1(x, w, bias=None, residual=None, act=0, in_scale=None, stride=1, pixel_major=False, out=None, roi=None,
            fragments=None, roi_rule="tile"):
    """Pointwise convolution with fused prologue / epilogue: act(W (in_scale . x) + bias (+ residual));
    act 0 none | 1 ReLU | 2 SiLU; stride 1 | 2.  x [n,Cin,H,W] f32 cuda, w [Cout,Cin,1,1], in_scale [n,Cin].
    fragments: the conv1x1_fragments layout of `w`, made by the caller (xca_fragments).  For a weight that a kernel wrote on the
    device during this forward: such a tensor has no parameter behind it and no version that moves when it is rewritten, so it must
    not go through the weight-derived cache.  The launch is then heal_conv1x1 itself (no split-K, no opt-in kernel).
    pixel_major=True: the result comes back as [n, Ho*Wo, Cout] (a pixel's channels contiguous) instead of NCHW.
    out: optional destination (NCHW result only), e.g. the batch slice of a stage's output that an agent chunk fills.
    roi: per-image output boxes [(y0, y1, x0, x1)] * n (heal_conv1x1_roi; NCHW result only): 64-pixel tiles that hold no pixel of
    their image's box are not computed and their part of the result keeps what the buffer held (uninitialised memory for a new
    one).  The split-K and the opt-in kernels take no ROI: they compute the whole map.
    roi_rule: "tile" (above) | "box" (heal_conv1x1_box_roi): the tiles enumerate each image's box, its columns rounded outward to
    multiples of 4; exactly those pixels are computed and written (conv1x1_box_tiles is the host's count of it)."""
    if roi_rule not in ("tile", "box"):
        raise _capi.HealAmdError(f"conv1x1: roi_rule must be 'tile' or 'box' (got {roi_rule!r})")
    x = _need(x, torch.float32, "x")
    n, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    bias = _need_bias(bias, cout, "conv1x1")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    hard_ok = stride in (1, 2) and ((Ho * Wo) % 4 == 0 if stride == 1 else Wo % 4 == 0)
    if int(w.shape[1]) != cin or not hard_ok:
        raise _capi.HealAmdError(f"conv1x1: unsupported shape Cin={cin} Cout={cout} HxW={H}x{W} stride={stride}")
    if (out is not None or roi is not None) and pixel_major:
        raise _capi.HealAmdError("conv1x1: `out` and `roi` are for the NCHW result")
    nprod = arith_products() if fragments is None else 0
    if (nprod and stride == 1 and not pixel_major and in_scale is None and w.dtype == torch.float32
            and _capi.query("heal_conv1x1_split_supported", cin, cout, H, W)):
        y = _out_or_empty(out, (n, cout, H, W), x.device, "conv1x1")
        if residual is not None:
            residual = _need(residual, torch.float32, "residual")
            if tuple(residual.shape) != tuple(y.shape):
                raise _capi.HealAmdError("conv1x1: residual shape mismatch")
        frag = conv1x1_split_fragments(w)
        with _Timed(f"conv1x1_{cin}_{cout}", 2.0 * n * cin * cout * H * W,
                    4.0 * n * (cin * H * W + cout * H * W * (2 if residual is not None else 1)), kernel_events=True):
            _capi.call("heal_conv1x1_split", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, n, cin, cout, H, W, int(act), nprod, _ptr(y), _stream())
        return y
    if (fragments is None and stride == 1 and not pixel_major and in_scale is None and conv1x1_tiled_ok(n, cin, cout, H * W)
            and w.dtype == torch.float32):
        y = _out_or_empty(out, (n, cout, H, W), x.device, "conv1x1")
        if residual is not None:
            residual = _need(residual, torch.float32, "residual")
            if tuple(residual.shape) != tuple(y.shape):
                raise _capi.HealAmdError("conv1x1: residual shape mismatch")
        wr = _w_rowmajor(w)
        with _Timed(f"conv1x1_{cin}_{cout}", 2.0 * n * cin * cout * H * W,
                    4.0 * n * (cin * H * W + cout * H * W * (2 if residual is not None else 1))):
            _capi.call("heal_conv1x1_tiled", _ptr(x), _ptr(wr), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, n, cin, cout, H, W, int(act), 0, 0, 0, _ptr(y), _stream())
        return y
    if fragments is None:
        frag = conv1x1_fragments(w)
    else:
        frag = _need(fragments, torch.float32, "fragments")
        if frag.numel() != ((cout + 63) // 64 * 64) * ((cin + 31) // 32 * 32):
            raise _capi.HealAmdError(f"conv1x1: `fragments` has {frag.numel()} elements for a {cout} x {cin} weight")
    if pixel_major:
        if residual is not None or cout % 4 != 0:
            raise _capi.HealAmdError("conv1x1: pixel-major output needs Cout % 4 == 0 and takes no residual")
        y = torch.empty((n, Ho * Wo, cout), dtype=torch.float32, device=x.device)
    else:
        y = _out_or_empty(out, (n, cout, Ho, Wo), x.device, "conv1x1")
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise _capi.HealAmdError("conv1x1: residual shape mismatch")
    if in_scale is not None:
        in_scale = _need(in_scale.reshape(n, cin), torch.float32, "in_scale")
    ksplit = conv1x1_ksplit(n, cin, cout, H * W) if (stride == 1 and not pixel_major and fragments is None) else 1
    if ksplit > 1:
        nbytes = _capi.query("heal_conv1x1_splitk_workspace", n, cout, H, W, ksplit)
        ws = _workspace("conv1x1_splitk", nbytes, x.device)
        with _Timed(f"conv1x1_{cin}_{cout}", 2.0 * n * cin * cout * H * W,
                    4.0 * n * (cin * H * W + cout * H * W * (2 if residual is not None else 1)), kernel_events=True):
            _capi.call("heal_conv1x1_splitk", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, _ptr(in_scale) if in_scale is not None else None,
                       n, cin, cout, H, W, int(act), ksplit, _ptr(y), _ptr(ws), ws.numel(), _stream())
        return y
    table = _roi_table(roi, n, Ho, Wo, "conv1x1") if roi is not None else None
    with _Timed(f"conv1x1_{cin}_{cout}" + ("_s2" if stride == 2 else ""), 2.0 * n * cin * cout * Ho * Wo,
                4.0 * n * (cin * Ho * Wo + cout * Ho * Wo * (2 if residual is not None else 1)), kernel_events=True):
        if table is not None and roi_rule == "box":
            _capi.call("heal_conv1x1_box_roi", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, _ptr(in_scale) if in_scale is not None else None,
                       n, cin, cout, H, W, int(stride), int(act), ctypes.c_void_p(table.ctypes.data), _ptr(y), _stream())
        elif table is not None:
            _capi.call("heal_conv1x1_roi", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, _ptr(in_scale) if in_scale is not None else None,
                       n, cin, cout, H, W, int(stride), int(act), 0, ctypes.c_void_p(table.ctypes.data), _ptr(y), _stream())
        else:
            _capi.call("heal_conv1x1", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None,
                       _ptr(residual) if residual is not None else None, _ptr(in_scale) if in_scale is not None else None,
                       n, cin, cout, H, W, int(stride), int(act), int(bool(pixel_major)), _ptr(y), _stream())
    return y


def conv1x1_d2s(x, w, bias, act, k, dst, channel_offset):
    """Pointwise convolution to Cout = C k^2 channels whose epilogue writes depth-to-space into dst[:, off:off+C] (dst
    [n, Ctot, H k, W k], contiguous): a ConvTranspose2d(kernel = stride = k) deblock written straight into the concatenated
    tensor.  x [n,Cin,H,W], w [C k^2, Cin, 1, 1] (row c k^2 + dy k + dx = output channel c at sub-pixel (dy, dx))."""
    x = _need(x, torch.float32, "x")
    dst = _need(dst, torch.float32, "dst")
    n, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    if (not dst.is_contiguous() or int(dst.shape[0]) != n or int(dst.shape[2]) != H * k or int(dst.shape[3]) != W * k
            or cout % (k * k) or W % 4):
        raise _capi.HealAmdError(f"conv1x1_d2s: destination {tuple(dst.shape)} does not fit x {tuple(x.shape)} at k={k}")
    bias = _need_bias(bias, cout, "conv1x1_d2s")
    if conv1x1_tiled_ok(n, cin, cout, H * W) and w.dtype == torch.float32:
        wr = _w_rowmajor(w)
        with _Timed(f"conv1x1_{cin}_{cout}", 2.0 * n * cin * cout * H * W, 4.0 * n * H * W * (cin + cout)):
            _capi.call("heal_conv1x1_tiled", _ptr(x), _ptr(wr), _ptr(bias) if bias is not None else None, None, n, cin, cout, H, W,
                       int(act), int(k), int(dst.shape[1]), int(channel_offset), _ptr(dst), _stream())
        return dst[:, channel_offset:channel_offset + cout // (k * k)]
    frag = conv1x1_fragments(w)
    with _Timed(f"conv1x1_{cin}_{cout}", 2.0 * n * cin * cout * H * W, 4.0 * n * H * W * (cin + cout), kernel_events=True):
        _capi.call("heal_conv1x1_d2s", _ptr(x), _ptr(frag), _ptr(bias) if bias is not None else None, n, cin, cout, H, W,
                   int(act), int(k), int(dst.shape[1]), int(channel_offset), _ptr(dst), _stream())
    return dst[:, channel_offset:channel_offset + cout // (k * k)]


def conv3x3_fragments(w):
    """MFMA A-fragment layout of a [Cout,Cin,3,3] weight for heal_conv3x3: zero-padded to [ceil64(Cout), ceil8(Cin)],
    ordered [Cout/64][Cin/8][tap][k-step][m-tile][lane] (see include/heal_amd.h)."""
    def build():
        cout, cin = int(w.shape[0]), int(w.shape[1])
        mpad, kpad = (cout + 63) // 64 * 64, (cin + 7) // 8 * 8
        wm = w.detach().reshape(cout, cin, 9)
        if (mpad, kpad) != (cout, cin):
            wm = torch.nn.functional.pad(wm, (0, 0, 0, kpad - cin, 0, mpad - cout))
        # [mb, mt, ln, chunk, ks, lk, tap] -> [mb, chunk, tap, ks, mt, lk, ln]
        return wm.reshape(mpad // 64, 4, 16, kpad // 8, 2, 4, 9).permute(0, 3, 6, 4, 1, 5, 2).contiguous()
    return _derived("conv3x3_fragments", (w,), build)


def conv3x3_same(x, w, bias, stride, pad, act="none"):
    """Dense 3x3 convolution with explicit (left, right, top, bottom) zero padding where left / top are 0 | 1 and right / bottom
    at most 1 (TF-style "same" padding of the EfficientNet stem), bias and none | relu | silu fused.  x [n,Cin,H,W]."""
    x = _need(x, torch.float32, "x")
    n, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    pl, pr, pt, pb = (int(v) for v in pad)
    Ho, Wo = (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1
    if pl not in (0, 1) or pt not in (0, 1) or pr > 1 or pb > 1 or tuple(w.shape[1:]) != (cin, 3, 3):
        raise _capi.HealAmdError(f"conv3x3_same: unsupported padding {pad} / weight {tuple(w.shape)}")
    frag = conv3x3_fragments(w)
    y = torch.empty((n, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    with _Timed(f"conv3x3_{cin}_{cout}_s{stride}same", 2.0 * 9 * n * cin * cout * Ho * Wo, 4.0 * n * (cin * H * W + cout * Ho * Wo),
                kernel_events=True):
        _capi.call("heal_conv3x3_same", _ptr(x), _ptr(frag), _ptr(_need_bias(bias, cout, "conv3x3_same")),
                   n, cin, cout, H, W, int(stride), pt, pl, Ho, Wo, {"none": 0, "relu": 1, "silu": 2}[act], _ptr(y), _stream())
    return y


def conv3x3_winograd_waves(n=1, cout=64, H=256, W=256):
    """Waves per Winograd block: 8 (16x16-pixel tiles, one block per CU: best operand reuse) when that still gives every CU two
    or more blocks, else 4 (8x16-pixel tiles, two independent blocks per CU whose transform / MFMA phases overlap; measured
    crossover, scripts/conv3x3_bench.py); HEAL_WG_WAVES overrides."""
    waves = switches.number("HEAL_WG_WAVES")
    if waves is not None:
        return waves
    blocks8 = n * ((cout + 63) // 64) * ((H + 15) // 16) * ((W + 15) // 16)
    return 8 if blocks8 >= 512 else 4


def conv3x3_winograd_kc(cin, waves, H=1, W=1):
    """Input channels per chunk of the Winograd K loop: 16 where the kernel has it (an experimental build, 8-wave blocks,
    cin % 16 == 0, a map whose 16-channel chunk stays below 2^31 bytes) and HEAL_WG_KC asks for it, else 8.  Measured in round 5
    (profiles/r05_wino_kc16.txt): 4-13 % slower, hence experimental."""
    ok16 = (switches.number("HEAL_WG_KC") == 16 and waves == 8 and cin % 16 == 0 and 16 * H * W * 4 < 2 ** 31 and experimental_build())
    return 16 if ok16 else 8


def experimental_build():
    """True if libheal_amd.so was built with HEAL_BUILD_EXPERIMENTAL=1 (the measured-negative kernels of
    include/heal_amd_experimental.h are present)."""
    return hasattr(_capi.lib(), "heal_gconv_conv3")


def conv3x3_winograd_fragments(w, waves=8, kc=8):
    """Winograd-domain weights U = G g G^T of a [Cout,Cin,3,3] filter bank in the lane-major fragment order
    heal_conv3x3_winograd[_kc] reads for `waves` waves per block and `kc` channels per chunk (include/heal_amd.h)."""
    def build():
        cout, cin = int(w.shape[0]), int(w.shape[1])
        mpad, kpad = (cout + 63) // 64 * 64, (cin + kc - 1) // kc * kc
        G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64,
                         device=w.device)
        U = (G @ w.detach().double() @ G.t()).float().reshape(cout, cin, 16)      # xi = 4a + b
        if (mpad, kpad) != (cout, cin):
            U = torch.nn.functional.pad(U, (0, 0, 0, kpad - cin, 0, mpad - cout))
        # [mb, mt, ln, chunk, ks, lk, w, xi_i] -> [mb, chunk, w, lk, ln, xi_i, ks, mt]
        return U.reshape(mpad // 64, 4, 16, kpad // kc, kc // 4, 4, waves, 16 // waves).permute(0, 3, 6, 5, 2, 7, 4, 1).contiguous()
    return _derived("conv3x3_winograd_fragments", (w,), build, (waves, kc))


def conv3x3_winograd4_fragments(w):
    """F(4x4,3x3) Winograd-domain weights U = G g G^T (6 x 6 per filter, formed in float64) of a [Cout,Cin,3,3] filter bank
    in the lane-major order heal_conv3x3_winograd4 reads: [Cout/32][Cin/16][wave 8][lane 64][xi_i 9][ks 4], value
    U[xi = 9 (wave & 3) + xi_i][co = 32 mb + 16 (wave >> 2) + (lane & 15)][ci = 16 chunk + 4 ks + (lane >> 4)], zero-padded."""
    def build():
        cout, cin = int(w.shape[0]), int(w.shape[1])
        mpad, kpad = (cout + 31) // 32 * 32, (cin + 15) // 16 * 16
        G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                          [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64, device=w.device)
        U = (G @ w.detach().double() @ G.t()).float().reshape(cout, cin, 36)      # xi = 6 a + b
        if (mpad, kpad) != (cout, cin):
            U = torch.nn.functional.pad(U, (0, 0, 0, kpad - cin, 0, mpad - cout))
        # [mb, mt, ln, chunk, ks, lk, g, xi_i] -> [mb, chunk, mt, g, lk, ln, xi_i, ks]   (wave = 4 mt + g, lane = 16 lk + ln)
        return U.reshape(mpad // 32, 2, 16, kpad // 16, 4, 4, 4, 9).permute(0, 3, 1, 6, 5, 2, 7, 4).contiguous()
    return _derived("conv3x3_winograd4_fragments", (w,), build)


def conv3x3_winograd4_ok(n, cout, H, W):
    """F(4x4,3x3) (heal_conv3x3_winograd4) is OPT-IN: HEAL_C3_ALGO=winograd4.  Measured 0.80 - 1.03x of F(2x2,3x3) at the scenes'
    shapes (profiles/r03_wino_f44_vs_f22.json): a quarter of the multiplications instead of 4/9, but twice the transform work per
    output at 32 output channels per block."""
    return switches.get("HEAL_C3_ALGO") == "winograd4" and experimental_build()


def conv3x3_algo(stride, n=1, cout=64, H=256, W=256):
    """'winograd' | 'direct' for a shape; HEAL_C3_ALGO overrides for A/B.  Winograd F(2x2,3x3) is the stride-1 formulation
    and runs one 8-wave block per CU on a 16x16-pixel x 64-channel tile: below ~one block per CU the implicit GEMM with its
    smaller tiles fills the chip better (measured crossover ~100 blocks, scripts/conv3x3_bench.py)."""
    a = switches.get("HEAL_C3_ALGO")
    if stride != 1 or a == "direct":
        return "direct"
    if a in ("winograd", "winograd4"):
        return "winograd"
    blocks = n * ((cout + 63) // 64) * ((H + 15) // 16) * ((W + 15) // 16)
    return "winograd" if blocks >= 96 else "direct"


def conv_gemm_supported(cin, cout, Wo):
    return cout % 128 == 0 and cin % 32 == 0 and Wo % 4 == 0 and switches.on("HEAL_CONV_GEMM")


def conv_gemm(x, w, bias=None, residual=None, relu=False, stride=1):
    """heal_conv_gemm: dense 3x3 (padding 1) or 1x1 convolution as an implicit GEMM on 128 x 128 x 32 tiles of the 32x32x2 fp32
    MFMA.  x [n,Cin,H,W], w [Cout,Cin,k,k] (re-laid [Cout, k*k, Cin] once, cached) -> [n,Cout,Ho,Wo]."""
    x = _need(x, torch.float32, "x")
    n, cin, H, W = (int(v) for v in x.shape)
    cout, ks = int(w.shape[0]), int(w.shape[2])
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    wt = _derived("conv_gemm_tapmajor", (w,), lambda: w.detach().permute(0, 2, 3, 1).reshape(cout, ks * ks, cin).contiguous())
    y = torch.empty((n, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    bias = _need_bias(bias, cout, "conv_gemm")
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise _capi.HealAmdError("conv_gemm: residual shape mismatch")
    name = (f"conv3x3_{cin}_{cout}" if ks == 3 else f"conv{ks}x{ks}_{cin}_{cout}") + ("_s2" if stride == 2 else "")
    with _Timed(name, 2.0 * ks * ks * n * cin * cout * Ho * Wo, 4.0 * n * (cin * H * W + cout * Ho * Wo), kernel_events=True):
        _capi.call("heal_conv_gemm", _ptr(x), _ptr(wt), _optr(bias), _optr(residual), n, cin, cout, H, W, ks, int(stride),
                   int(bool(relu)), _ptr(y), _stream())
    return y


def conv7x7_s2_supported(cin, cout, W):
    return cin % 32 == 0 and cout <= 128 and ((W - 1) // 2 + 1) % 4 == 0 and switches.on("HEAL_CONV_GEMM")


def conv7x7_s2(x, w, bias=None, relu=False):
    """Conv2d(Cin, Cout <= 128, kernel 7, stride 2, padding 3) (+ bias) (+ ReLU) on heal_conv_gemm's 128 x 128 x 32 implicit GEMM: BevEncode's
    stem of the old-style Lift-Splat model (lss_submodule.py:242).  The kernel wants 128-channel output tiles: the weight (and bias) are
    padded with zero rows once (cached), the first Cout channels of the result are returned."""
    cout = int(w.shape[0])
    bias = _need_bias(bias, cout, "conv7x7_s2")

    def build():
        wp = torch.zeros((128,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
        wp[:cout] = w.detach()
        bp = None
        if bias is not None:
            bp = torch.zeros((128,), dtype=torch.float32, device=w.device)
            bp[:cout] = bias.detach()
        return wp, bp
    wp, bp = _derived("conv7x7_s2_pad128", (w, bias), build)
    y = conv_gemm(x, wp, bp, None, relu, 2)
    return y[:, :cout].contiguous() if cout < 128 else y


def conv3x3_winograd_ksplit(n, cin, cout, H, W, waves):
    """K splits of a Winograd launch: 1 unless the grid is small (< 256 blocks: less than one per CU) and the reduction deep
    (>= 32 chunks of 8 input channels); then enough splits for ~768 blocks (three per CU: two resident 4-wave blocks + one queued),
    at least 8 chunks each, none empty.  The camera trunk's Up block (lss_submodule.py:33-50: 432 -> 512 and 512 -> 512 at
    4 x 24 x 32 pixels = 192 blocks of 54 / 64 chunks) is what this is for.  HEAL_C3_KSPLIT forces a value (0 / 1: off)."""
    chunks = (cin + 7) // 8
    blocks = -(-W // 16) * -(-H // (2 * waves)) * n * -(-cout // 64)
    want = switches.number("HEAL_C3_KSPLIT")
    if want is None:
        want = min(chunks // 8, max(2, -(-768 // blocks))) if blocks < 256 and chunks >= 32 else 1
    if want < 2 or chunks < 2 or (H * W) % 4 or n * want > 65535:
        return 1
    want = min(want, chunks)
    return -(-chunks // -(-chunks // want))       # ceil(chunks / ceil(chunks / want)): no empty split


def conv3x3(x, w, bias=None, residual=None, relu=False, stride=1):
    """Dense 3x3 convolution, padding 1, stride 1 | 2, on the fp32 matrix cores with fused bias (+ residual) (+ ReLU).
    x [n,Cin,H,W] f32 cuda, w [Cout,Cin,3,3] -> [n,Cout,Ho,Wo].  Stride 1 runs the Winograd F(2x2,3x3) formulation
    (heal_conv3x3_winograd), stride 2 the implicit GEMM (heal_conv3x3)."""
    x = _need(x, torch.float32, "x")
    n, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    if tuple(w.shape[1:]) != (cin, 3, 3) or stride not in (1, 2):
        raise _capi.HealAmdError(f"conv3x3: unsupported weight {tuple(w.shape)} / stride {stride} for input {tuple(x.shape)}")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((n, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise _capi.HealAmdError("conv3x3: residual shape mismatch")
    bias = _need_bias(bias, cout, "conv3x3")
    if stride == 1 and conv3x3_winograd4_ok(n, cout, H, W):
        frag = conv3x3_winograd4_fragments(w)
        with _Timed(f"conv3x3w_{cin}_{cout}", 2.0 * 9 * n * cin * cout * Ho * Wo, 4.0 * n * (cin * H * W + cout * Ho * Wo)):
            _capi.call("heal_conv3x3_winograd4", _ptr(x), _ptr(frag), _ptr(bias), _ptr(residual), n, cin, cout, H, W,
                       int(bool(relu)), _ptr(y), _stream())
        return y
    if conv3x3_algo(stride, n, cout, H, W) == "winograd":
        waves = conv3x3_winograd_waves(n, cout, H, W)
        kc = conv3x3_winograd_kc(cin, waves, H, W)
        frag = conv3x3_winograd_fragments(w, waves, kc)
        ksplit = conv3x3_winograd_ksplit(n, cin, cout, H, W, waves) if kc == 8 else 1
        with _Timed(f"conv3x3w_{cin}_{cout}", 2.0 * 9 * n * cin * cout * Ho * Wo, 4.0 * n * (cin * H * W + cout * Ho * Wo),
                    kernel_events=True):
            if ksplit > 1:
                ws = _workspace("conv3x3w_splitk", _capi.query("heal_conv3x3_winograd_splitk_workspace", n, cout, H, W, ksplit),
                                x.device)
                _capi.call("heal_conv3x3_winograd_splitk", _ptr(x), _ptr(frag), _ptr(bias), _ptr(residual), n, cin, cout, H, W,
                           int(bool(relu)), waves, ksplit, _ptr(y), _ptr(ws), ws.numel(), _stream())
            else:
                _capi.call("heal_conv3x3_winograd_kc", _ptr(x), _ptr(frag), _ptr(bias), _ptr(residual), n, cin, cout, H, W,
                           int(bool(relu)), waves, kc, _ptr(y), _stream())
        return y
    if stride == 2 and cin >= 128 and conv_gemm_supported(cin, cout, Wo) and n * Ho * Wo >= 65536:
        # the large stride-2 layers: the 128 x 128 x 32 implicit GEMM on 32x32x2 MFMA (heal_conv_gemm).  Measured
        # (scripts/conv_gemm_bench.py; round 4, after the kernel's weight staging stopped going through scratch memory):
        # 384 -> 256 @256^2 x 8: 2.19 vs 3.69 ms for heal_conv3x3 (MIOpen 2.63) = 106 TFLOP/s; 128 -> 256: 0.74 vs 1.02;
        # 128 -> 128 @256^2 x 5: 0.30 vs 0.31; 256 -> 256 @128^2 x 5 (20 480 pixels: below the bound) 0.35 vs 0.29 for MIOpen
        return conv_gemm(x, w, bias, residual, relu, stride)
    frag = conv3x3_fragments(w)
    with _Timed(f"conv3x3_{cin}_{cout}" + ("_s2" if stride == 2 else ""), 2.0 * 9 * n * cin * cout * Ho * Wo,
                4.0 * n * (cin * H * W + cout * Ho * Wo), kernel_events=True):
        _capi.call("heal_conv3x3", _ptr(x), _ptr(frag), _ptr(bias), _ptr(residual), n, cin, cout, H, W, int(stride),
                   int(bool(relu)), _ptr(y), _stream())
    return y


# ------------------------------------------------------------------------------------------------ dense convolution backward
def conv_grad_enabled():
    """HEAL_CONV_GRAD=kernel: the dense 3x3 / 1x1 convolutions of the gradient path run forward, data gradient and weight gradient
    on this library's kernels (ConvGrad).  Opt-in: until scripts/conv_grad_bench.py says otherwise the library composition stays
    the default, as with HEAL_WATTN_GRAD."""
    return switches.get("HEAL_CONV_GRAD") == "kernel"


# what ConvGrad ran since the process started (tests and scripts/conv_grad_bench.py read it): forward calls, heal_conv_wgrad calls,
# data gradients on heal_conv3x3 / heal_conv1x1 and data gradients left to the library (stride 2, maps the pointwise kernel refuses)
CONV_GRAD_CALLS = {"forward": 0, "wgrad": 0, "dx_kernel": 0, "dx_library": 0}


def _conv_wgrad_shape(x, g, k, stride):
    """(n, cin, cout, H, W) if x [n, cin, H, W] and g [n, cout, Ho, Wo] belong to one k x k convolution of that stride, else None."""
    if not (isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dim() == 4 and g.dim() == 4
            and k in (1, 3) and stride in (1, 2)):
        return None
    n, cin, H, W = (int(v) for v in x.shape)
    if min(n, cin, H, W) < 1 or int(g.shape[1]) < 1:
        return None
    if (int(g.shape[0]), int(g.shape[2]), int(g.shape[3])) != (n, (H - 1) // stride + 1, (W - 1) // stride + 1):
        return None
    return n, cin, int(g.shape[1]), H, W


def conv_wgrad_supported(x, g, k, stride):
    """True if heal_conv_wgrad takes the pair: f32 device tensors x [n, Cin, H, W], g [n, Cout, Ho, Wo], k 1 | 3 (padding k // 2),
    stride 1 | 2.  No alignment or divisibility requirement."""
    shape = _conv_wgrad_shape(x, g, k, stride)
    return (shape is not None and x.is_cuda and g.is_cuda and x.dtype == torch.float32 and g.dtype == torch.float32
            and bool(_capi.query("heal_conv_wgrad_supported", *shape, int(k), int(stride))))


def conv_wgrad(x, g, k, stride):
    """Weight gradient of a dense convolution (what torch.nn.grad.conv2d_weight returns): x [n, Cin, H, W], g [n, Cout, Ho, Wo]
    f32 cuda, k 1 | 3 with padding k // 2, stride 1 | 2 -> dW [Cout, Cin, k, k].  fp32 MFMA over the pixels; the reduction is
    split over blocks and summed in a fixed order (bit-equal across calls)."""
    x = _need(x, torch.float32, "x")
    g = _need(g, torch.float32, "g")
    shape = _conv_wgrad_shape(x, g, k, stride)
    if shape is None or not _capi.query("heal_conv_wgrad_supported", *shape, int(k), int(stride)):
        raise _capi.HealAmdError(f"conv_wgrad: x {tuple(x.shape)} and g {tuple(g.shape)} do not belong to a supported "
                                 f"convolution (k={k}, stride={stride}; k 1 | 3, stride 1 | 2)")
    n, cin, cout, H, W = shape
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    nbytes = _capi.query("heal_conv_wgrad_workspace", n, cin, cout, H, W, int(k), int(stride))
    ws = _workspace("conv_wgrad", nbytes, x.device) if nbytes else None
    with _Timed(f"conv_wgrad{k}_{cin}_{cout}" + ("_s2" if stride == 2 else ""), 2.0 * g.numel() * cin * k * k,
                4.0 * (x.numel() + g.numel() + dw.numel())):
        _capi.call("heal_conv_wgrad", _ptr(x), _ptr(g), n, cin, cout, H, W, int(k), int(stride), _ptr(dw), _ptr(ws),
                   ws.numel() if ws is not None else 0, _stream())
    CONV_GRAD_CALLS["wgrad"] += 1
    return dw


def conv_grad_supported(x, weight, stride):
    """True if ConvGrad takes the convolution: x f32 on the device, weight [Cout, Cin, k, k] with k 1 | 3 (padding k // 2, no groups,
    no dilation), stride 1 | 2, and a map the forward kernel takes (heal_conv1x1 wants 16-byte pixel rows)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and weight.is_cuda
            and weight.dtype == torch.float32 and weight.dim() == 4 and stride in (1, 2)):
        return False
    n, cin, H, W = (int(v) for v in x.shape)
    cout, k = int(weight.shape[0]), int(weight.shape[2])
    if tuple(weight.shape[1:]) != (cin, k, k) or k not in (1, 3) or min(n, cin, cout, H, W) < 1:
        return False
    if not _capi.query("heal_conv_wgrad_supported", n, cin, cout, H, W, k, int(stride)):
        return False
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return k == 3 or conv1x1_supported(cin, cout, Ho * Wo, stride, Wo)


def _conv_grad_wt(weight):
    """The weight of the data-gradient convolution: [Cin, Cout, k, k], taps flipped (3x3) -- dx = conv(g, flip(W)^T)."""
    k = int(weight.shape[2])
    return _derived("conv_grad_wt", (weight,),
                    lambda: (weight.flip(2, 3) if k == 3 else weight).transpose(0, 1).contiguous())


class ConvGrad(torch.autograd.Function):
    """A dense convolution (3x3 padding 1 | 1x1, stride 1 | 2) under autograd on this library's kernels:
    apply(x, weight, bias | None, stride) -> conv2d(x, weight, bias, stride, k // 2).  Forward: heal_conv3x3 / heal_conv1x1 on the
    raw weight.  Backward: dW = heal_conv_wgrad, db = sum of g, dx = the forward kernels on the flipped, channel-transposed weight at
    stride 1; at stride 2 (and for maps the pointwise kernel refuses) dx = torch.nn.grad.conv2d_input on the library."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        x = x.contiguous()
        k = int(weight.shape[2])
        y = conv3x3(x, weight, bias, None, False, stride) if k == 3 else conv1x1(x, weight, bias, None, 0, stride=stride)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (k, int(stride), bias is not None)
        CONV_GRAD_CALLS["forward"] += 1
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        k, stride, has_bias = ctx.cfg
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            cin, cout = int(weight.shape[1]), int(weight.shape[0])
            if stride == 1 and k == 3:
                dx = conv3x3(g, _conv_grad_wt(weight), None, None, False, 1)
            elif stride == 1 and conv1x1_supported(cout, cin, int(g.shape[2] * g.shape[3])):
                dx = conv1x1(g, _conv_grad_wt(weight), None, None, 0)
            if dx is not None:
                CONV_GRAD_CALLS["dx_kernel"] += 1
            else:
                dx = torch.nn.grad.conv2d_input(x.shape, weight, g, stride=stride, padding=k // 2)
                CONV_GRAD_CALLS["dx_library"] += 1
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad(x, g, k, stride)
        if has_bias and ctx.needs_input_grad[2]:
            db = g.sum((0, 2, 3))
        return dx, dw, db, None


# ------------------------------------------------------------------------------- BatchNorm + residual + ReLU of the gradient path
_BN_GRAD_MODES = ("torch", "kernel")
_BN_GRAD_MODE = "torch"


class bn_grad:
    """ops.bn_grad("kernel"): the BatchNorm2d (+ residual) (+ ReLU) sites of the gradient path (bev_blocks.grad_bn_act) run as
    ops.BatchNormAct on this library's kernels; ops.bn_grad("torch") (the default): the library composition.  A plain setter --
    the mode is set when the object is made -- and a context manager, which puts the previous mode back on exit:
        ops.bn_grad("kernel")                 # from here on
        with ops.bn_grad("kernel"): ...       # for the block
    A process-wide Python setting, deliberately not an environment switch."""

    def __init__(self, mode):
        global _BN_GRAD_MODE
        if mode not in _BN_GRAD_MODES:
            raise ValueError(f"bn_grad: mode must be one of {_BN_GRAD_MODES}, got {mode!r}")
        self.previous = _BN_GRAD_MODE
        _BN_GRAD_MODE = mode

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _BN_GRAD_MODE
        _BN_GRAD_MODE = self.previous
        return False


def bn_grad_enabled():
    """True in ops.bn_grad("kernel") mode."""
    return _BN_GRAD_MODE == "kernel"


# what bev_blocks.grad_bn_act ran since the process started (tests and scripts/bn_grad_bench.py read it): BatchNormAct forwards and
# backwards, and sites left to the torch modules (the default mode, CPU tensors, other dtypes, BatchNorms the kernels do not take)
BN_GRAD_CALLS = {"forward": 0, "backward": 0, "module": 0}


def _bn_shape(x):
    """(n, C, HW) of a 4-D map, else None."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        return None
    n, C, H, W = (int(v) for v in x.shape)
    return (n, C, H * W) if H * W < 2 ** 31 else None


def bn_train_supported(x):
    """True if the BatchNorm training kernels take the map: a contiguous f32 device tensor [n, C, H, W] within the index ranges of
    heal_bn_train_supported.  No alignment or divisibility requirement."""
    shape = _bn_shape(x)
    return (shape is not None and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and min(shape) >= 1
            and bool(_capi.lib().heal_bn_train_supported(*shape)))


def _bn_map(t, name, who, like=None):
    """A contiguous f32 device map; `like`: the map whose shape and device it must share.  Nothing is copied or converted."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise _capi.HealAmdError(f"{who}: {name} must have dtype torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise _capi.HealAmdError(f"{who}: {name} must be contiguous")
    if like is None:
        if not bn_train_supported(t):
            raise _capi.HealAmdError(f"{who}: {name} of shape {tuple(t.shape)} is not a supported [n, C, H, W] map")
    elif t.shape != like.shape or t.device != like.device:
        raise _capi.HealAmdError(f"{who}: {name} has shape {tuple(t.shape)} on {t.device}, want {tuple(like.shape)} on {like.device}")
    return t


def _bn_vec(t, C, name, who, like):
    """A contiguous f32 vector of C values on the device of `like`."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device:
        raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor on the device of the map")
    if t.dtype != torch.float32:
        raise _capi.HealAmdError(f"{who}: {name} must have dtype torch.float32, got {t.dtype}")
    if tuple(t.shape) != (C,) or not t.is_contiguous():
        raise _capi.HealAmdError(f"{who}: {name} has shape {tuple(t.shape)}, want a contiguous [{C}]")
    return t


def _bn_workspace(x, shape):
    need = _capi.query("heal_bn_train_workspace", *shape)
    return _workspace("bn_train", need, x.device), need


def bn_stats(x, eps, momentum=0.0, running_mean=None, running_var=None, out=None):
    """Batch statistics of x [n, C, H, W] (heal_bn_stats) -> (mean [C], rstd [C]) with rstd = 1 / sqrt(biased variance + eps), from
    fp64 sums, each rounded once.  running_mean / running_var (both or neither) are updated in place as nn.BatchNorm2d does
    (momentum; the unbiased variance).  out: optional (mean, rstd) destinations."""
    who = "bn_stats"
    x = _bn_map(x, "x", who)
    n, C, HW = shape = _bn_shape(x)
    if (running_mean is None) != (running_var is None):
        raise _capi.HealAmdError(f"{who}: running_mean and running_var go together")
    if running_mean is not None:
        _bn_vec(running_mean, C, "running_mean", who, x)
        _bn_vec(running_var, C, "running_var", who, x)
        if n * HW < 2:
            raise _capi.HealAmdError(f"{who}: the unbiased variance of the running statistics needs n * H * W >= 2, got {n * HW}")
    if not float(eps) >= 0.0:
        raise _capi.HealAmdError(f"{who}: eps must not be negative, got {eps}")
    mean, rstd = out if out is not None else (torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(2))
    _bn_vec(mean, C, "out[0]", who, x)
    _bn_vec(rstd, C, "out[1]", who, x)
    ws, need = _bn_workspace(x, shape)
    with _Timed("bn_stats", 3.0 * x.numel(), 4.0 * x.numel()):
        _capi.call("heal_bn_stats", _ptr(x), n, C, HW, float(eps), float(momentum), _ptr(mean), _ptr(rstd), _optr(running_mean),
                   _optr(running_var), _ptr(ws), need, _stream())
    return mean, rstd


def bn_act_forward(x, residual, mean, rstd, gamma, beta, relu, out=None):
    """y = [relu]((x - mean) * rstd * gamma + beta (+ residual)) per channel of x [n, C, H, W] (heal_bn_act_forward).  mean / rstd:
    bn_stats' or a frozen BatchNorm's running mean and 1 / sqrt(running_var + eps).  out: optional destination like x."""
    who = "bn_act_forward"
    x = _bn_map(x, "x", who)
    n, C, HW = _bn_shape(x)
    if residual is not None:
        _bn_map(residual, "residual", who, x)
    for t, name in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta")):
        _bn_vec(t, C, name, who, x)
    y = _bn_map(out, "out", who, x) if out is not None else torch.empty_like(x)
    maps = 2 + (residual is not None)
    with _Timed("bn_act_forward", 4.0 * x.numel(), 4.0 * maps * x.numel(), kernel_events=True):
        _capi.call("heal_bn_act_forward", _ptr(x), _optr(residual), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), n, C, HW,
                   int(bool(relu)), _ptr(y), _stream())
    return y


def bn_act_backward(dy, x, y, mean, rstd, gamma, relu, batch_stats, want=(True, True, True, True), out=None):
    """Backward of bn_act_forward (heal_bn_act_backward) -> (dx, dresidual, dgamma, dbeta), None where `want` (four flags in that
    order) does not ask for one.  y: the forward's result, needed exactly when relu (the mask is y > 0).  batch_stats: the
    statistics were the batch's own (the gradient flows through them) | frozen.  out: optional destinations, a 4-tuple with None
    where the wrapper shall allocate."""
    who = "bn_act_backward"
    x = _bn_map(x, "x", who)
    n, C, HW = shape = _bn_shape(x)
    _bn_map(dy, "dy", who, x)
    if bool(relu) != (y is not None):
        raise _capi.HealAmdError(f"{who}: y (the forward's result) is required exactly when relu is set")
    if y is not None:
        _bn_map(y, "y", who, x)
    for t, name in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma")):
        _bn_vec(t, C, name, who, x)
    want = tuple(bool(w) for w in want)
    if len(want) != 4:
        raise _capi.HealAmdError(f"{who}: want must hold four flags (dx, dresidual, dgamma, dbeta)")
    out = tuple(out) if out is not None else (None,) * 4
    res = []
    for i, name in enumerate(("dx", "dresidual", "dgamma", "dbeta")):
        t = out[i] if want[i] else None
        if want[i] and t is None:
            t = torch.empty_like(x) if i < 2 else torch.empty(C, dtype=torch.float32, device=x.device)
        elif t is not None:
            t = _bn_map(t, f"out[{name}]", who, x) if i < 2 else _bn_vec(t, C, f"out[{name}]", who, x)
        res.append(t)
    if not any(want):
        return tuple(res)
    ws, need = _bn_workspace(x, shape)
    reads = (2 + bool(relu)) * ((want[2] or want[3] or (batch_stats and want[0])) + (want[0] or want[1]))
    with _Timed("bn_act_backward", 8.0 * x.numel(), 4.0 * (reads + want[0] + want[1]) * x.numel()):
        _capi.call("heal_bn_act_backward", _ptr(dy), _ptr(x), _optr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), n, C, HW,
                   int(bool(relu)), int(bool(batch_stats)), _optr(res[0]), _optr(res[1]), _optr(res[2]), _optr(res[3]), _ptr(ws), need,
                   _stream())
    return tuple(res)


class BatchNormAct(torch.autograd.Function):
    """BatchNorm2d (+ residual) (+ ReLU) under autograd on this library's kernels:
    apply(x, residual | None, bn_weight, bn_bias, running_mean, running_var, training, momentum, eps, relu)
        -> [relu](batch_norm(x) (+ residual)).
    training: heal_bn_stats (the running buffers are updated in place) then heal_bn_act_forward; otherwise heal_bn_act_forward from
    the running statistics.  Saves x, y (only with relu), mean, rstd and the weight -- what the composition holds.  Backward: one
    heal_bn_act_backward call for the gradients that are needed; without ReLU the residual's gradient is grad_out itself."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, training, momentum, eps, relu):
        if training:
            mean, rstd = bn_stats(x, eps, momentum, running_mean, running_var)
        else:
            mean, rstd = running_mean, 1.0 / torch.sqrt(running_var + eps)      # F.batch_norm's own expression
        y = bn_act_forward(x, residual, mean, rstd, weight, bias, relu)
        ctx.save_for_backward(x, y if relu else None, mean, rstd, weight)
        ctx.cfg = (bool(relu), bool(training), residual is not None)
        BN_GRAD_CALLS["forward"] += 1
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, mean, rstd, weight = ctx.saved_tensors
        relu, training, has_res = ctx.cfg
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad
        want_res = has_res and need[1]
        dx, dres, dgamma, dbeta = bn_act_backward(grad_out, x, y, mean, rstd, weight, relu, training,
                                                  want=(need[0], want_res and relu, need[2], need[3]))
        if want_res and not relu:
            dres = grad_out
        BN_GRAD_CALLS["backward"] += 1
        return dx, dres, dgamma, dbeta, None, None, None, None, None, None


# ------------------------------------------------------------------------------- warp_affine_simple of the gradient path
_WARP_GRAD_MODES = ("torch", "kernel")
_WARP_GRAD_MODE = "torch"


class warp_grad:
    """ops.warp_grad("kernel"): the warps into the ego frame of the gradient path (fusion_in_one.warp_to_ego, _warp_affine_simple,
    CoBEVT's inline warp) run as ops.WarpAffine on this library's kernels where ops.warp_affine_train_supported takes them;
    ops.warp_grad("torch") (the default): F.affine_grid + F.grid_sample under autograd.  A plain setter -- the mode is set when the
    object is made -- and a context manager, which puts the previous mode back on exit:
        ops.warp_grad("kernel")                 # from here on
        with ops.warp_grad("kernel"): ...       # for the block
    A process-wide Python setting, deliberately not an environment switch."""

    def __init__(self, mode):
        global _WARP_GRAD_MODE
        if mode not in _WARP_GRAD_MODES:
            raise ValueError(f"warp_grad: mode must be one of {_WARP_GRAD_MODES}, got {mode!r}")
        self.previous = _WARP_GRAD_MODE
        _WARP_GRAD_MODE = mode

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _WARP_GRAD_MODE
        _WARP_GRAD_MODE = self.previous
        return False


def warp_grad_enabled():
    """True in ops.warp_grad("kernel") mode."""
    return _WARP_GRAD_MODE == "kernel"


# what the gradient-path warps ran since the process started (tests and scripts/warp_grad_bench.py read it): WarpAffine forwards and
# backwards, and warps left to affine_grid + grid_sample (the default mode, CPU tensors, other dtypes, rows the backward refuses)
WARP_GRAD_CALLS = {"forward": 0, "backward": 0, "torch": 0}


def _warp_rows_host(affine_rows, n, who):
    """The n affine rows as a contiguous float64 host array [n, 6].  A CUDA tensor is brought to the host (48 n bytes, a
    synchronising copy: refused under stream capture)."""
    if isinstance(affine_rows, torch.Tensor):
        if affine_rows.is_cuda and torch.cuda.is_current_stream_capturing():
            raise _capi.HealAmdError(f"{who}: the affine rows are a device tensor and the backward's support rule is decided on the "
                                     "host; that copy cannot run under stream capture (pass host rows)")
        affine_rows = affine_rows.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(affine_rows, dtype=np.float64).reshape(-1, 6))
    if a.shape[0] != n:
        raise _capi.HealAmdError(f"{who}: expected {n} x (2,3) affine rows, got {a.shape}")
    return a


def _warp_map(x, name, who):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if x.dtype != torch.float32 or x.dim() != 4 or min(x.shape) < 1:
        raise _capi.HealAmdError(f"{who}: {name} must be a non-empty fp32 [n, C, H, W] map, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _warp_rows_supported(rows, H, W):
    """heal_warp_affine_backward_supported on every chunk of at most WARP_MAX_AGENTS rows of a host array [n, 6]."""
    L = _capi.lib()
    return all(bool(L.heal_warp_affine_backward_supported(rows[i:i + WARP_MAX_AGENTS].ctypes.data_as(ctypes.c_void_p),
                                                          int(min(WARP_MAX_AGENTS, rows.shape[0] - i)), H, W))
               for i in range(0, rows.shape[0], WARP_MAX_AGENTS))


def warp_affine(x, affine_rows, grid_f64=True):
    """warp_affine_simple(x, rows, (H, W)) for one scene in one launch (heal_warp_affine_forward): x [n,C,H,W] -> [n,C,H,W], agent a
    sampled with affine_rows[a] ([n,2,3]: a host array, or a CUDA tensor that is then read on the device at run time).  Bit-equal
    to warp_agent agent by agent.  More than WARP_MAX_AGENTS agents go in chunks."""
    who = "warp_affine"
    x = _need(_warp_map(x, "x", who), torch.float32, "x")
    n, C, H, W = (int(v) for v in x.shape)
    out = torch.empty_like(x)
    keep, ap, adev = _affine_args(affine_rows, n)
    for i in range(0, n, WARP_MAX_AGENTS):
        k = min(WARP_MAX_AGENTS, n - i)
        api = ctypes.c_void_p(ap.value + 48 * i) if ap.value else ap
        adi = ctypes.c_void_p(adev.value + 48 * i) if adev.value else adev
        with _Timed("warp_affine", 0.0, 8.0 * k * C * H * W, kernel_events=True):
            _capi.call("heal_warp_affine_forward", _ptr(x[i:i + k]), k, C, H, W, api, adi, int(bool(grid_f64)), _ptr(out[i:i + k]),
                       _stream())
    return out


def warp_affine_backward(grad_out, affine_rows, grid_f64=True):
    """The adjoint of warp_affine (heal_warp_affine_backward): grad_out [n,C,H,W] -> grad_x [n,C,H,W], every element written, no
    atomics (two calls are bit-equal).  affine_rows: host rows [n,2,3] that heal_warp_affine_backward_supported takes."""
    who = "warp_affine_backward"
    g = _warp_map(grad_out, "grad_out", who)
    n, C, H, W = (int(v) for v in g.shape)
    rows = _warp_rows_host(affine_rows, n, who)
    gx = torch.empty_like(g)
    for i in range(0, n, WARP_MAX_AGENTS):
        k = min(WARP_MAX_AGENTS, n - i)
        with _Timed("warp_affine_backward", 0.0, 8.0 * k * C * H * W, kernel_events=True):
            _capi.call("heal_warp_affine_backward", _ptr(g[i:i + k]), k, C, H, W, rows[i:i + k].ctypes.data_as(ctypes.c_void_p),
                       int(bool(grid_f64)), _ptr(gx[i:i + k]), _stream())
    return gx


def warp_affine_train_supported(x, affine_rows):
    """True if ops.WarpAffine takes the warp: x a fp32 CUDA map [n, C, H, W] (made contiguous by the operator), rows that carry no
    gradient, and the C-side rule of heal_warp_affine_backward_supported (finite, invertible, reach <= HEAL_WARP_BWD_MAX_REACH).
    Rows on the device are read back for the decision; under stream capture that is not possible and the answer is False."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and min(x.shape) >= 1):
        return False
    if isinstance(affine_rows, torch.Tensor):
        if affine_rows.requires_grad or (affine_rows.is_cuda and torch.cuda.is_current_stream_capturing()):
            return False
        affine_rows = affine_rows.detach().cpu().numpy()
    rows = np.asarray(affine_rows, dtype=np.float64)
    n, C, H, W = (int(v) for v in x.shape)
    if rows.size != 6 * n or H * W > 2 ** 30 or n * -(-C // 16) > 65535:
        return False
    return _warp_rows_supported(np.ascontiguousarray(rows.reshape(n, 6)), H, W)


class WarpAffine(torch.autograd.Function):
    """warp_affine_simple under autograd on this library's kernels: apply(x [n,C,H,W], affine_rows [n,2,3], grid_f64) -> [n,C,H,W].
    Gradient with respect to x only (the rows are poses, not parameters).  Rows that arrive as a CUDA tensor are brought to the
    host once, here in the forward: the backward's support rule is a host decision.  Nothing is saved but those 48 n bytes."""

    @staticmethod
    def forward(ctx, x, affine_rows, grid_f64=True):
        n = int(x.shape[0])
        rows = _warp_rows_host(affine_rows, n, "WarpAffine")
        if not _warp_rows_supported(rows, int(x.shape[2]), int(x.shape[3])):
            raise _capi.HealAmdError("WarpAffine: the backward kernel does not take these rows (singular, not finite or a reach above "
                                     "HEAL_WARP_BWD_MAX_REACH): ask ops.warp_affine_train_supported first")
        ctx.rows, ctx.grid_f64 = rows, bool(grid_f64)
        WARP_GRAD_CALLS["forward"] += 1
        return warp_affine(x, rows, grid_f64)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        WARP_GRAD_CALLS["backward"] += 1
        return warp_affine_backward(grad_out, ctx.rows, ctx.grid_f64), None, None


def channel_dot_supported(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and int(x.shape[2] * x.shape[3]) % 4 == 0


def channel_dot(x, weight, bias=None):
    """Pointwise convolution to one output channel: x [n,C,H,W], weight [1,C,1,1] (or [C]), bias [1] -> [n,1,H,W]."""
    x = _need(x, torch.float32, "x")
    n, C, H, W = (int(v) for v in x.shape)
    weight = _need(weight.reshape(-1), torch.float32, "weight")
    if int(weight.numel()) != C:
        raise _capi.HealAmdError(f"channel_dot: weight has {int(weight.numel())} elements for {C} channels")
    y = torch.empty((n, 1, H, W), dtype=torch.float32, device=x.device)
    with _Timed(f"channel_dot_{C}", 2.0 * n * C * H * W, 4.0 * n * (C + 1) * H * W):
        _capi.call("heal_channel_dot", _ptr(x), _ptr(weight), _ptr(_need(bias, torch.float32, "bias")) if bias is not None else None,
                   n, C, H * W, _ptr(y), _stream())
    return y


def layernorm_nchw(x, gamma, beta, eps):
    """LayerNorm over the channel axis of x [n,C,H,W] (biased variance, eps inside the sqrt)."""
    x = _need(x, torch.float32, "x")
    n, C, H, W = (int(v) for v in x.shape)
    y = torch.empty_like(x)
    _capi.call("heal_layernorm_nchw", _ptr(x), _ptr(_need(gamma, torch.float32, "gamma")),
               _ptr(_need(beta, torch.float32, "beta")), n, C, H * W, float(eps), _ptr(y), _stream())
    return y


def align_fused_enabled():
    """HEAL_ALIGN_FUSED as the library reads it (heal_align_fused_enabled: the variable is one of the library's own, declared as such
    in heal_amd/switches.py): False for "0" -- the aligners of AlignNet beyond ConvNeXt (sdta, resnet1x1, resnet3x3, scaligner, cbam,
    fanet) then run as the reference's torch composition on the device (A/B)."""
    v = int(_capi.lib().heal_align_fused_enabled())
    if v < 0:
        raise _capi.HealAmdError("HEAL_ALIGN_FUSED is not a valid setting: expected 0 or 1")
    return v == 1


XCA_CALLS = {"weights": 0}      # heal_xca_weights calls so far (tests: the gradient path must not take the kernel)


def xca_supported(C, heads, N):
    """Shapes heal_xca_weights takes: d = C / heads in {16, 32}, 16-byte pixel rows (N % 4 == 0), N >= 64."""
    return bool(_capi.lib().heal_xca_supported(int(C), int(heads), int(N)))


def xca_parts(B, heads, N):
    """(parts, pixels of one part) of the Gram pass for this grid (heal_xca_parts / heal_xca_range): the summation shape the
    tests' error bound needs."""
    return int(_capi.lib().heal_xca_parts(int(B), int(heads), int(N))), int(_capi.lib().heal_xca_range(int(B), int(heads), int(N)))


def xca_weights(qkv, temperature, proj_w_scaled, heads, want_attn=False, want_stats=False):
    """Cross-covariance attention folded into one pointwise weight per image (heal_xca_weights, include/heal_amd_align.h).
    qkv [B, 3C, H, W] (or [B, 3C, N]) f32 cuda, channel s C + h d + i = row i of head h of q / k / v; temperature [heads] (any
    trailing 1-dims); proj_w_scaled [C, C] = gamma_xca (.) W_proj.
    -> (W [B, C, C] with x + gamma_xca * xca(.) = x + W[b] v_b + gamma_xca (.) b_proj,
        A [B, heads, d, d] or None (want_attn),
        stats [B, heads, d d + 2 d] or None (want_stats): the Gram matrix, then the squared norms of the q rows and of the k rows)."""
    who = "xca_weights"
    qkv = _need(qkv, torch.float32, "qkv")
    if qkv.dim() not in (3, 4) or int(qkv.shape[1]) % 3:
        raise _capi.HealAmdError(f"{who}: qkv must be [B, 3C, H, W] or [B, 3C, N], got {tuple(qkv.shape)}")
    B, C = int(qkv.shape[0]), int(qkv.shape[1]) // 3
    N = int(qkv.numel()) // max(B * 3 * C, 1)
    heads = int(heads)
    if heads < 1 or not xca_supported(C, heads, N) or not 1 <= B <= 65535:
        raise _capi.HealAmdError(f"{who}: unsupported shape B={B} C={C} heads={heads} N={N}: d = C / heads must be 16 or 32, "
                                 "N % 4 == 0 and N >= 64")
    temperature = _need(temperature.reshape(-1), torch.float32, "temperature")
    pw = _need(proj_w_scaled, torch.float32, "proj_w_scaled")
    if temperature.numel() != heads or tuple(pw.shape) != (C, C) or temperature.device != qkv.device or pw.device != qkv.device:
        raise _capi.HealAmdError(f"{who}: temperature must hold {heads} values and proj_w_scaled be [{C}, {C}] on {qkv.device}")
    d, dev = C // heads, qkv.device
    W = torch.empty((B, C, C), dtype=torch.float32, device=dev)
    A = torch.empty((B, heads, d, d), dtype=torch.float32, device=dev) if want_attn else None
    stats = torch.empty((B, heads, d * d + 2 * d), dtype=torch.float32, device=dev) if want_stats else None
    ws = _workspace("xca_weights", _capi.query("heal_xca_workspace", B, C, heads, N), dev)
    XCA_CALLS["weights"] += 1
    with _Timed(f"xca_weights_{C}", 2.0 * B * d * C * N, 8.0 * B * C * N, kernel_events=True):
        _capi.call("heal_xca_weights", _ptr(qkv), _ptr(temperature), _ptr(pw), B, C, heads, N, _ptr(ws), ws.numel(), _ptr(W),
                   _ptr(A), _ptr(stats), _stream())
    return W, A, stats


def xca_fragments(W):
    """[B, C, C] device-made pointwise weights (xca_weights) -> their conv1x1_fragments layout in one copy: [B, C/16, C/16, 4, 16, 4],
    element [b][mt][kc][q][r][j] = W[b][16 mt + r][16 kc + 4 j + q] (lane 16 q + r, four k-steps per lane).  C % 64 == 0 (no padding)."""
    B, C = int(W.shape[0]), int(W.shape[1])
    if C % 64 or int(W.shape[2]) != C:
        raise _capi.HealAmdError(f"xca_fragments: weights must be [B, C, C] with C % 64 == 0, got {tuple(W.shape)}")
    return W.reshape(B, C // 16, 16, C // 16, 4, 4).permute(0, 1, 3, 5, 2, 4).contiguous()


def ssfa_fused_enabled():
    """HEAL_SSFA_FUSED as the library reads it (heal_ssfa_fused_enabled: the variable is one of the library's own, declared as such
    in heal_amd/switches.py): False for "0" -- SSFA then runs as the reference's torch composition on the device (A/B)."""
    v = int(_capi.lib().heal_ssfa_fused_enabled())
    if v < 0:
        raise _capi.HealAmdError("HEAL_SSFA_FUSED is not a valid setting: expected 0 or 1")
    return v == 1


SSFA_CALLS = {"deconv": 0, "blend": 0}      # kernel calls so far (tests: refusals launch nothing, the gradient path takes neither)


def deconv3x3_s2_supported(cin, cout, H, W):
    """Shapes heal_deconv3x3_s2 takes: cin and cout multiples of 32 in 32 .. 2048, any H, W >= 1 (up to 65535 tiles of 8 x 16)."""
    return bool(_capi.lib().heal_deconv3x3_s2_supported(int(cin), int(cout), int(H), int(W)))


def _deconv3x3_s2_pack(w):
    cin, cout = int(w.shape[0]), int(w.shape[1])
    return (w.detach().reshape(cin // 8, 2, 4, cout // 16, 16, 9).permute(3, 0, 5, 2, 4, 1).contiguous()
            .reshape(cout // 16, cin // 8, 9, 64, 2))


def deconv3x3_s2_fragments(w):
    """A ConvTranspose2d weight [Cin, Cout, 3, 3] in heal_deconv3x3_s2's fragment order [Cout/16, Cin/8, 9, 64, 2]: element
    [mt][kc][3 ky + kx][lane][j] = w[8 kc + 4 j + lane // 16][16 mt + lane % 16][ky][kx].  Cached per weight (heal_amd.derived)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or int(w.shape[0]) % 8 or int(w.shape[1]) % 16:
        raise _capi.HealAmdError(f"deconv3x3_s2_fragments: weight must be [Cin % 8 == 0, Cout % 16 == 0, 3, 3], got {tuple(w.shape)}")
    return _derived("deconv3x3_s2_fragments", (w,), lambda: _deconv3x3_s2_pack(w))


def deconv3x3_s2(x, w_frag_or_w, bias=None, relu=True, residual=None):
    """ConvTranspose2d(k 3, stride 2, padding 1, output_padding 1) with fused bias, ReLU and residual (heal_deconv3x3_s2,
    include/heal_amd_ssfa.h): x [n,Cin,H,W] f32 cuda; the weight [Cin,Cout,3,3] or its deconv3x3_s2_fragments; bias [Cout];
    residual [n,R,2H,2W], added AFTER the ReLU to the first R <= Cout output channels -> [n,Cout,2H,2W]."""
    who = "deconv3x3_s2"
    x = _need(x, torch.float32, "x")
    if x.dim() != 4:
        raise _capi.HealAmdError(f"{who}: x must be [n, Cin, H, W], got {tuple(x.shape)}")
    n, cin, H, W = (int(v) for v in x.shape)
    w = w_frag_or_w
    if not isinstance(w, torch.Tensor) or w.dim() not in (4, 5):
        raise _capi.HealAmdError(f"{who}: the weight must be [Cin, Cout, 3, 3] or its fragments [Cout/16, Cin/8, 9, 64, 2]")
    if w.dim() == 4:
        if int(w.shape[0]) != cin or tuple(w.shape[2:]) != (3, 3):
            raise _capi.HealAmdError(f"{who}: weight {tuple(w.shape)} does not fit the input {tuple(x.shape)}")
        cout = int(w.shape[1])
    else:
        cout = 16 * int(w.shape[0])
        if tuple(w.shape[1:]) != (cin // 8, 9, 64, 2) or cin % 8:
            raise _capi.HealAmdError(f"{who}: fragments {tuple(w.shape)} do not fit the input {tuple(x.shape)}")
    if not deconv3x3_s2_supported(cin, cout, H, W) or not 1 <= n <= 65535:
        raise _capi.HealAmdError(f"{who}: unsupported shape n={n} Cin={cin} Cout={cout} HxW={H}x{W}: Cin and Cout must be "
                                 "multiples of 32 in 32 .. 2048")
    frag = _need(deconv3x3_s2_fragments(w) if w.dim() == 4 else w, torch.float32, "weight")
    bias = _need_bias(bias, cout, who)
    res_channels = 0
    if residual is not None:
        residual = _need(residual, torch.float32, "residual")
        res_channels = int(residual.shape[1]) if residual.dim() == 4 else -1
        if (residual.dim() != 4 or tuple(residual.shape) != (n, res_channels, 2 * H, 2 * W) or not 1 <= res_channels <= cout
                or residual.device != x.device):
            raise _capi.HealAmdError(f"{who}: residual {tuple(residual.shape)} must be [{n}, 1 .. {cout}, {2 * H}, {2 * W}] "
                                     f"on {x.device}")
    if frag.device != x.device or (bias is not None and bias.device != x.device):
        raise _capi.HealAmdError(f"{who}: weight and bias must be on {x.device}")
    y = torch.empty((n, cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    with _Timed(f"deconv3x3_s2_{cin}_{cout}", 2.0 * 9 * n * cin * cout * H * W,
                4.0 * n * (cin * H * W + (cout + res_channels) * 4 * H * W), kernel_events=True):
        _capi.call("heal_deconv3x3_s2", _ptr(x), _ptr(frag), _ptr(bias), _ptr(residual), res_channels, n, cin, cout, H, W,
                   int(bool(relu)), _ptr(y), _stream())
    SSFA_CALLS["deconv"] += 1
    return y


def ssfa_blend_supported(C, HW):
    """Shapes heal_ssfa_blend takes: C in {64, 128}, 16-byte pixel rows (HW % 4 == 0)."""
    return bool(_capi.lib().heal_ssfa_blend_supported(int(C), int(HW)))


def ssfa_blend(a, b, wa, ba, wb, bb, want_weights=False):
    """SSFA's two-way attention in one pass (heal_ssfa_blend, include/heal_amd_ssfa.h): a, b [n,C,H,W] f32 cuda; wa, wb [C] (any
    trailing 1-dims) and ba, bb (a one-element device tensor, or a number) the w_0 / w_1 convolutions with their BatchNorm folded.
    pa = 1 / (1 + exp((wb . b + bb) - (wa . a + ba)));  -> a pa + b (1 - pa), and with want_weights also pa [n,1,H,W]."""
    who = "ssfa_blend"
    a, b = _need(a, torch.float32, "a"), _need(b, torch.float32, "b")
    if a.dim() != 4 or a.shape != b.shape or a.device != b.device:
        raise _capi.HealAmdError(f"{who}: a and b must be two [n, C, H, W] maps of one shape on one device, got "
                                 f"{tuple(a.shape)} and {tuple(b.shape)}")
    n, C, H, W = (int(v) for v in a.shape)
    if not ssfa_blend_supported(C, H * W) or not 1 <= n <= 65535:
        raise _capi.HealAmdError(f"{who}: unsupported shape n={n} C={C} HxW={H}x{W}: C must be 64 or 128 and H W a multiple of 4")
    vec = []
    for t, name in ((wa, "wa"), (wb, "wb")):
        t = _need(t, torch.float32, name).reshape(-1)
        if t.numel() != C or t.device != a.device:
            raise _capi.HealAmdError(f"{who}: {name} must hold {C} values on {a.device}")
        vec.append(t)
    for t, name in ((ba, "ba"), (bb, "bb")):
        if not isinstance(t, torch.Tensor):
            t = torch.full((1,), float(t), dtype=torch.float32, device=a.device)
        t = _need(t, torch.float32, name).reshape(-1)
        if t.numel() != 1 or t.device != a.device:
            raise _capi.HealAmdError(f"{who}: {name} must be one value on {a.device}")
        vec.append(t)
    out = torch.empty_like(a)
    pa = torch.empty((n, 1, H, W), dtype=torch.float32, device=a.device) if want_weights else None
    with _Timed(f"ssfa_blend_{C}", 6.0 * n * C * H * W, 12.0 * n * C * H * W, kernel_events=True):
        _capi.call("heal_ssfa_blend", _ptr(a), _ptr(b), _ptr(vec[0]), _ptr(vec[1]), _ptr(vec[2]), _ptr(vec[3]), n, C, H * W,
                   _ptr(out), _ptr(pa), _stream())
    SSFA_CALLS["blend"] += 1
    return (out, pa) if want_weights else out


def se_gate(mean, w_reduce, b_reduce, w_expand, b_expand, scale=1.0, tiles=1):
    """Squeeze-excite gate: mean [n,C] (any trailing 1-dims), w_reduce [S,C,1,1], w_expand [C,S,1,1] -> gate [n,C].
    tiles = T, scale = 1/(H*W): `mean` holds the per-tile sums [n,C,T] of depthwise_conv(channel_sums=True)."""
    n, C = int(mean.shape[0]), int(mean.shape[1])
    S = int(w_reduce.shape[0])
    mean = _need(mean.reshape(n, C, int(tiles)), torch.float32, "mean")
    w_expand = _need(w_expand, torch.float32, "w_expand")
    w_t = _derived("se_gate_expand_t", (w_expand,), lambda: w_expand.detach().reshape(C, S).t().contiguous())   # [S,C]
    gate = torch.empty((n, C), dtype=torch.float32, device=mean.device)
    _capi.call("heal_se_gate", _ptr(mean), _ptr(_need(w_reduce, torch.float32, "w_reduce")),
               _ptr(_need(b_reduce, torch.float32, "b_reduce")), _ptr(w_t),
               _ptr(_need(b_expand, torch.float32, "b_expand")), n, C, S, float(scale), int(tiles), _ptr(gate),
               _stream())
    return gate


def resnext_bottleneck(x, w1_frag, b1, w2, b2, w3_frag, b3):
    """Fused stride-1 ResNeXt bottleneck (K7b).  x [n,C,H,W] -> y [n,C,H,W]."""
    x = _need(x, torch.float32, "x")
    n, C, H, W = (int(v) for v in x.shape)
    y = torch.empty_like(x)
    with _Timed(f"resnext_bottleneck_c{C}"):
        _capi.call("heal_resnext_bottleneck", _ptr(x), _ptr(w1_frag), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3_frag),
                   _ptr(b3), n, C, H, W, _ptr(y), _stream())
    return y


def upsample2x_bilinear(x):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True).  x [n,C,H,W] -> [n,C,2H,2W]."""
    x = _need(x, torch.float32, "x")
    n, C, H, W = (int(v) for v in x.shape)
    y = torch.empty((n, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    _capi.call("heal_upsample2x_bilinear", _ptr(x), n, C, H, W, _ptr(y), _stream())
    return y


def depthwise_tiles(Ho, Wo):
    """Output tiles (32 x 8 pixels) of one depthwise_conv channel = the last dimension of its `channel_sums` argument."""
    return ((Wo + 31) // 32) * ((Ho + 7) // 8)


def depthwise_conv(x, weight, bias, stride, pad, act="none", channel_sums=None):
    """Depthwise k x k conv; pad = (left, right, top, bottom) zero padding; act in none|relu|silu.  channel_sums=True: also
    return the per-tile sums [n, C, T] of the outputs (the squeeze of an SE stage, folded into this launch) -> (y, sums)."""
    x = _need(x, torch.float32, "x")
    weight = _need(weight, torch.float32, "weight")
    n, C, H, W = (int(v) for v in x.shape)
    bias = _need_bias(bias, C, "depthwise_conv")
    k = int(weight.shape[-1])
    pl, pr, pt, pb = (int(v) for v in pad)
    Ho = (H + pt + pb - k) // stride + 1
    Wo = (W + pl + pr - k) // stride + 1
    y = torch.empty((n, C, Ho, Wo), dtype=torch.float32, device=x.device)
    sums = torch.empty((n, C, depthwise_tiles(Ho, Wo)), dtype=torch.float32, device=x.device) if channel_sums else None
    _capi.call("heal_depthwise_conv", _ptr(x), _ptr(weight), _ptr(bias), n, C, H, W, k, int(stride), pt, pl, Ho, Wo,
               {"none": 0, "relu": 1, "silu": 2}[act], _ptr(y), _ptr(sums) if sums is not None else None, _stream())
    return (y, sums) if channel_sums else y


def fill_bytes(t, byte):
    """t (contiguous CUDA tensor, size a multiple of 4 bytes) <- `byte` in every byte, by the library's fill KERNEL (heal_fill_bytes;
    include/heal_amd.h explains why not a memset)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
        raise _capi.HealAmdError("fill_bytes: a contiguous CUDA tensor is required")
    _capi.call("heal_fill_bytes", _ptr(t), int(byte), t.numel() * t.element_size(), _stream())
    return t


# ---- the index-building primitives of csrc/prims.hip as operators of their own (include/heal_amd_ext.h) ----------------------------
# The model path reaches them only through their clients (the sparse convolution's rulebook, heal_bev_pool's cell sort); these
# wrappers exist so that tests/test_gpu_prims.py can compare the primitives themselves with numpy.
def _need_words(t, name, who):
    """A 1-D int32 cuda tensor (made contiguous); for the sort the 32 bits of a word are an unsigned key / value."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.HealAmdError(f"{who}: {name} must be a CUDA/HIP tensor (heal_amd has no CPU path)")
    if t.dtype != torch.int32 or t.dim() != 1:
        raise _capi.HealAmdError(f"{who}: {name} must be a 1-D torch.int32 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def scan_exclusive(x, out=None, want_total=True):
    """Exclusive prefix sum of x [n] i32 cuda (heal_scan_exclusive): out[i] = x[0] + ... + x[i-1]; `out` may be x itself.
    -> (out, total [1] i32 on the device) or, with want_total=False, out."""
    x = _need_words(x, "x", "scan_exclusive")
    n = int(x.numel())
    if out is None:
        out = torch.empty_like(x)
    elif _need_words(out, "out", "scan_exclusive") is not out or int(out.numel()) != n:
        raise _capi.HealAmdError(f"scan_exclusive: out must be a contiguous i32 tensor of {n} elements")
    total = torch.empty((1,), dtype=torch.int32, device=x.device) if want_total else None
    need = _capi.query("heal_scan_exclusive_workspace", n)
    ws = _workspace("scan_exclusive", need, x.device)
    _capi.call("heal_scan_exclusive", _ptr(x), _ptr(out), n, _ptr(total), _ptr(ws), need, _stream())
    return (out, total) if want_total else out


def radix_sort_pairs(keys, vals, key_bits):
    """Stable ascending sort of the pairs (keys [n], vals [n]; i32 cuda, read as unsigned words) by the low 9 * ceil(key_bits / 9)
    bits of the keys (heal_radix_sort_pairs; all 32 bits of a key travel with it).  The inputs are left as they are: the sort runs
    on a ping-pong pair of its own.  -> (sorted keys, sorted vals), views of whichever half holds the result."""
    keys = _need_words(keys, "keys", "radix_sort_pairs")
    vals = _need_words(vals, "vals", "radix_sort_pairs")
    n = int(keys.numel())
    if int(vals.numel()) != n:
        raise _capi.HealAmdError(f"radix_sort_pairs: {n} keys but {int(vals.numel())} values")
    kbuf = torch.empty((2, n), dtype=torch.int32, device=keys.device)
    vbuf = torch.empty((2, n), dtype=torch.int32, device=keys.device)
    kbuf[0].copy_(keys)
    vbuf[0].copy_(vals)
    need = _capi.query("heal_radix_sort_pairs_workspace", n)
    ws = _workspace("radix_sort_pairs", need, keys.device)
    which = ctypes.c_int(-1)
    _capi.call("heal_radix_sort_pairs", _ptr(kbuf[0]), _ptr(kbuf[1]), _ptr(vbuf[0]), _ptr(vbuf[1]), n, int(key_bits),
               ctypes.byref(which), _ptr(ws), need, _stream())
    return kbuf[which.value], vbuf[which.value]


# ---- CoAlign's agent-object pose graph (include/heal_amd_pose.h) ---------------------------------------------------------------
POSE_CALLS = {"align": 0}                    # kernel calls so far (tests: a refusal launches nothing)
POSE_STATS = ("landmarks", "edges", "iterations", "status", "chi2_initial", "chi2_final", "lambda", "trials")
_POSE_OPTION_BITS = (("landmark_SE2", "HEAL_POSE_LANDMARK_SE2", True), ("adaptive_landmark", "HEAL_POSE_ADAPTIVE_LANDMARK", False),
                     ("normalize_uncertainty", "HEAL_POSE_NORMALIZE_UNCERTAINTY", False),
                     ("abandon_hard_cases", "HEAL_POSE_ABANDON_HARD_CASES", False),
                     ("drop_hard_boxes", "HEAL_POSE_DROP_HARD_BOXES", False), ("drop_unsure_edge", "HEAL_POSE_DROP_UNSURE_EDGE", False))


def pose_graph_limits():
    """(HEAL_POSE_MAX_AGENTS, HEAL_POSE_MAX_BOXES): per sample, read from include/heal_amd_pose.h."""
    return (_capi.header_define("HEAL_POSE_MAX_AGENTS", _capi.HEADER_POSE), _capi.header_define("HEAL_POSE_MAX_BOXES", _capi.HEADER_POSE))


def pose_graph_supported(max_agents_per_sample, max_boxes_per_sample):
    return bool(_capi.lib().heal_pose_graph_supported(int(max_agents_per_sample), int(max_boxes_per_sample)))


def pose_graph_align(corners_list, lidar_pose, uncertainty_list, record_len, return_stats=False, **box_align_args):
    """CoAlign's box alignment for a batch of samples in one call (heal_pose_graph_align, include/heal_amd_pose.h): the device
    counterpart of box_align_v2.box_alignment_relative_np.
      corners_list      per agent (all samples, in order) a CUDA tensor [n_i, 8, 3] of box corners in the agent's own frame, fp32 or
                        fp64 (fp32 is converted); None or an empty tensor for an agent without boxes
      lidar_pose        [sum(record_len), 6] x, y, z, roll, yaw, pitch in degrees (tensor or array, moved to the boxes' device)
      uncertainty_list  per agent [n_i, 3] log sigma^2 of (x, y, yaw), or None (no uncertainties)
      record_len        agents per sample; the first agent of a sample is its ego
      box_align_args    the reference's options: landmark_SE2, adaptive_landmark, normalize_uncertainty, abandon_hard_cases,
                        drop_hard_boxes, drop_unsure_edge, use_uncertainty, thres, yaw_var_thres, max_iterations
    -> refined [sum(record_len), 3] f64: x, y, yaw in degrees.  return_stats=True: (refined, stats, cluster_of_box) with stats a
    dict of [samples] tensors named POSE_STATS and cluster_of_box i32 [total boxes] (-1 or the landmark within its sample).
    A sample beyond HEAL_POSE_MAX_AGENTS / HEAL_POSE_MAX_BOXES raises before anything is launched.  No CPU path: the numpy
    function is the host path."""
    who = "pose_graph_align"
    args = dict(box_align_args)
    options = 0
    for name, define, default in _POSE_OPTION_BITS:
        if bool(args.pop(name, default)):
            options |= _capi.header_define(define, _capi.HEADER_POSE)
    use_unc = bool(args.pop("use_uncertainty", True))
    thres, yaw_var_thres = float(args.pop("thres", 1.5)), float(args.pop("yaw_var_thres", 0.2))
    max_iterations = int(args.pop("max_iterations", 1000))
    if args:
        raise _capi.HealAmdError(f"{who}: unknown option(s) {sorted(args)}")
    rec = [int(v) for v in (record_len.tolist() if hasattr(record_len, "tolist") else record_len)]
    total_agents = sum(rec)
    if not rec or min(rec) < 1 or len(corners_list) != total_agents:
        raise _capi.HealAmdError(f"{who}: record_len {rec} does not split {len(corners_list)} agents into samples of at least one")
    device = next((c.device for c in corners_list if isinstance(c, torch.Tensor) and c.is_cuda), None)
    if device is None and isinstance(lidar_pose, torch.Tensor) and lidar_pose.is_cuda:
        device = lidar_pose.device
    if device is None:
        raise _capi.HealAmdError(f"{who}: needs CUDA/HIP tensors (heal_amd has no CPU path; the host path is "
                                 "box_align_v2.box_alignment_relative_np)")
    counts, parts = [], []
    for a, c in enumerate(corners_list):
        k = 0 if c is None else int(len(c))
        if k:
            if not isinstance(c, torch.Tensor) or not c.is_cuda or c.device != device or tuple(c.shape[1:]) != (8, 3):
                raise _capi.HealAmdError(f"{who}: corners_list[{a}] must be a [n, 8, 3] tensor on {device}")
            if c.dtype not in (torch.float32, torch.float64):
                raise _capi.HealAmdError(f"{who}: corners_list[{a}] must be float32 or float64, got {c.dtype}")
            parts.append(c.detach().to(torch.float64).reshape(k, 24))
        counts.append(k)
    M = sum(counts)
    unc = None
    if use_unc and uncertainty_list is not None:
        if len(uncertainty_list) != total_agents:
            raise _capi.HealAmdError(f"{who}: {len(uncertainty_list)} uncertainty entries for {total_agents} agents")
        uparts = []
        for a, u in enumerate(uncertainty_list):
            k = 0 if u is None else int(len(u))
            if k != counts[a]:
                raise _capi.HealAmdError(f"{who}: uncertainty_list[{a}] has {k} rows for {counts[a]} boxes")
            if k:
                if not isinstance(u, torch.Tensor) or u.device != device or tuple(u.shape[1:]) != (3,):
                    raise _capi.HealAmdError(f"{who}: uncertainty_list[{a}] must be a [n, 3] tensor on {device}")
                uparts.append(u.detach().to(torch.float64))
        unc = torch.cat(uparts).contiguous() if uparts else torch.zeros((0, 3), dtype=torch.float64, device=device)
    pose = torch.as_tensor(lidar_pose).detach().to(device=device, dtype=torch.float64).contiguous()
    if tuple(pose.shape) != (total_agents, 6):
        raise _capi.HealAmdError(f"{who}: lidar_pose has shape {tuple(pose.shape)}, want [{total_agents}, 6]")
    S = len(rec)
    agent_off = np.concatenate([[0], np.cumsum(rec)]).astype(np.int32)
    box_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    per_sample = [int(box_off[agent_off[s + 1]] - box_off[agent_off[s]]) for s in range(S)]
    max_agents, max_boxes = max(rec), max(per_sample)
    if not pose_graph_supported(max_agents, max_boxes):
        lim = pose_graph_limits()
        raise _capi.HealAmdError(f"{who}: a sample of {max_agents} agents and {max_boxes} boxes is out of range (at most {lim[0]} "
                                 f"agents and {lim[1]} boxes per sample)")
    need = _capi.query("heal_pose_graph_workspace", S, total_agents, M)
    if need == 0:
        raise _capi.HealAmdError(f"{who}: unsupported batch ({S} samples, {total_agents} agents, {M} boxes)")
    corners = torch.cat(parts).contiguous() if parts else torch.zeros((0, 24), dtype=torch.float64, device=device)
    offsets = torch.from_numpy(np.concatenate([box_off, agent_off])).to(device)
    refined = torch.empty((total_agents, 3), dtype=torch.float64, device=device)
    cluster = torch.empty((M,), dtype=torch.int32, device=device) if return_stats else None
    nstat = _capi.header_define("HEAL_POSE_STATS", _capi.HEADER_POSE)
    stats = torch.empty((S, nstat), dtype=torch.float64, device=device) if return_stats else None
    ws = _workspace("pose_graph_align", need, device)
    with _Timed(f"pose_graph_align_s{S}"):
        _capi.call("heal_pose_graph_align", _ptr(corners), _ptr(offsets), _ptr(offsets[total_agents + 1:]), _ptr(pose), _ptr(unc), S,
                   total_agents, M, max_agents, max_boxes, options, thres, yaw_var_thres, max_iterations, _ptr(refined),
                   _ptr(cluster), _ptr(stats), _ptr(ws), need, _stream())
    POSE_CALLS["align"] += 1
    if not return_stats:
        return refined
    return refined, {name: stats[:, k] for k, name in enumerate(POSE_STATS)}, cluster
