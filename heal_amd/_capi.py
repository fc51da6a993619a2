"""ctypes binding of libheal_amd.so -- the C ABI declared in include/heal_amd.h.

This is the only place the package touches the native library.  There is NO fallback: if the
library is missing or a call fails, an exception is raised.
"""
import ctypes
import functools
import os
import re

from heal_amd import switches

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = switches.get("HEAL_AMD_LIB") or os.path.join(HERE, "lib", "libheal_amd.so")  # env: A/B a rebuilt library
HEADER = os.path.join(os.path.dirname(HERE), "include", "heal_amd.h")
HEADER_EXPERIMENTAL = os.path.join(os.path.dirname(HERE), "include", "heal_amd_experimental.h")
HEADER_TRAIN = os.path.join(os.path.dirname(HERE), "include", "heal_amd_train.h")
HEADER_EXT = os.path.join(os.path.dirname(HERE), "include", "heal_amd_ext.h")
HEADER_TRAIN_ATTN = os.path.join(os.path.dirname(HERE), "include", "heal_amd_train_attn.h")
HEADER_TRAIN_BN = os.path.join(os.path.dirname(HERE), "include", "heal_amd_train_bn.h")
HEADER_TRAIN_WARP = os.path.join(os.path.dirname(HERE), "include", "heal_amd_train_warp.h")
HEADER_CENTER = os.path.join(os.path.dirname(HERE), "include", "heal_amd_center.h")
HEADER_COMM = os.path.join(os.path.dirname(HERE), "include", "heal_amd_comm.h")
HEADER_UNC = os.path.join(os.path.dirname(HERE), "include", "heal_amd_unc.h")
HEADER_ROI = os.path.join(os.path.dirname(HERE), "include", "heal_amd_roi.h")
HEADER_ALIGN = os.path.join(os.path.dirname(HERE), "include", "heal_amd_align.h")
HEADER_SSFA = os.path.join(os.path.dirname(HERE), "include", "heal_amd_ssfa.h")
HEADER_POSE = os.path.join(os.path.dirname(HERE), "include", "heal_amd_pose.h")

_lib = None


class HealAmdError(RuntimeError):
    pass


# The headers are the only place a prototype is written: the ctypes signatures are read from them.  The mapping is closed --
# a parameter with a `*` is a pointer, a scalar is one of _SCALARS, and anything else (a struct by value, a function pointer,
# `...`, an unknown type) is an error: an argument list that is guessed hands a kernel a wrong pointer or stride silently.
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_NOT_PROTOTYPE = re.compile(r"#ifdef __cplusplus.*?#endif|^[ \t]*#[^\n]*|typedef\s+struct\b[^{;]*\{[^}]*\}[^;]*;", re.S | re.M)
_PROTOTYPE = re.compile(r"(.*?)\b(heal_[a-z0-9_]+)\s*\((.*)\)", re.S)


def _ctype(symbol, text, restype=False):
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if restype:
        found = ctypes.c_char_p if words == ["char", "*"] else _SCALARS.get(" ".join(words))
    elif "*" in words and "(" not in text:
        found = ctypes.c_void_p
    else:                                              # `type name` or `type`
        found = _SCALARS.get(" ".join(words)) or (words[-1:] and words[-1].isidentifier() and _SCALARS.get(" ".join(words[:-1])))
    if not found:
        raise HealAmdError(f"{symbol}: cannot map the {'return type' if restype else 'parameter'} `{text.strip()}` to ctypes")
    return found


def parse_prototypes(text):
    """{name: (restype, argtypes)} of every `ret heal_xxx(params);` in the text of a C header.  Comments, preprocessor lines,
    the extern "C" bracket and struct bodies are dropped; whatever else is not such a prototype raises HealAmdError."""
    out = {}
    for statement in _NOT_PROTOTYPE.sub(" ", _COMMENT.sub(" ", text)).split(";"):
        statement = " ".join(statement.split())
        if not statement:
            continue
        m = _PROTOTYPE.fullmatch(statement)
        if not m:
            raise HealAmdError(f"not a prototype of an entry point: `{statement}`")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(name, ret, restype=True), [_ctype(name, p) for p in params])
    return out


@functools.lru_cache(maxsize=None)
def signatures(experimental=None):
    """{name: (restype, argtypes)} of include/heal_amd.h (experimental=False), of include/heal_amd_experimental.h (True: the
    measured-negative kernels of a HEAL_BUILD_EXPERIMENTAL=1 library), or of both (None)."""
    if experimental is None:
        return {**signatures(False), **signatures(True)}
    with open(HEADER_EXPERIMENTAL if experimental else HEADER) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_train():
    """{name: (restype, argtypes)} of include/heal_amd_train.h: the training-side entry points (the dense convolutions' weight
    gradient).  Every build exports them; they are not part of the versioned inference ABI that signatures() describes."""
    with open(HEADER_TRAIN) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_ext():
    """{name: (restype, argtypes)} of include/heal_amd_ext.h: inference entry points added outside the versioned table of
    signatures() (heal_warp_mha_fuse; the scan and radix-sort primitives as test surfaces).  Every build exports them."""
    with open(HEADER_EXT) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_train_attn():
    """{name: (restype, argtypes)} of include/heal_amd_train_attn.h: the training side of CoBEVT's agent-window attention (its
    backward kernel).  Every build exports them; like signatures_train() they are outside the versioned inference ABI."""
    with open(HEADER_TRAIN_ATTN) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_train_bn():
    """{name: (restype, argtypes)} of include/heal_amd_train_bn.h: the gradient path's fused BatchNorm (+ residual) (+ ReLU) --
    batch statistics, apply and backward.  Every build exports them; like signatures_train() they are outside the versioned
    inference ABI."""
    with open(HEADER_TRAIN_BN) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_train_warp():
    """{name: (restype, argtypes)} of include/heal_amd_train_warp.h: warp_affine_simple as a differentiable operator -- the forward
    of all agents of a scene, its gather-form backward and the host-side support rule.  Every build exports them; like
    signatures_train() they are outside the versioned inference ABI."""
    with open(HEADER_TRAIN_WARP) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_center():
    """{name: (restype, argtypes)} of include/heal_amd_center.h: the anchor-free centre head -- CenterPointLoss with its target
    assignment, the box map and the decode + NMS front end.  Every build exports them; like signatures_ext() they are outside
    the versioned inference ABI."""
    with open(HEADER_CENTER) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_comm():
    """{name: (restype, argtypes)} of include/heal_amd_comm.h: Where2comm's communication mask (heal_comm_mask with its host-side
    support and workspace rules) and the masked form of the multiscale warp + attention fusion.  Every build exports them; like
    signatures_ext() they are outside the versioned inference ABI."""
    with open(HEADER_COMM) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_unc():
    """{name: (restype, argtypes)} of include/heal_amd_unc.h: CoAlign's uncertainty detector -- PointPillarUncertaintyLoss in one
    pass (heal_unc_loss with its host-side support and workspace rules) and the pooled decode + NMS that returns the kept boxes'
    uncertainty.  Every build exports them; like signatures_ext() they are outside the versioned inference ABI."""
    with open(HEADER_UNC) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_roi():
    """{name: (restype, argtypes)} of include/heal_amd_roi.h: the per-image region-of-interest launches of the pointwise and the
    small-group 3x3 convolution, and the reader of HEAL_PYRAMID_ROI.  Every build exports them; like signatures_ext() they are
    outside the versioned inference ABI."""
    with open(HEADER_ROI) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_align():
    """{name: (restype, argtypes)} of include/heal_amd_align.h: the SDTA aligner's cross-covariance attention folded into one
    pointwise weight per image (heal_xca_weights with its host-side support, parts and workspace rules).  Every build exports
    them; like signatures_ext() they are outside the versioned inference ABI."""
    with open(HEADER_ALIGN) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_ssfa():
    """{name: (restype, argtypes)} of include/heal_amd_ssfa.h: the dense neck of the SECOND + SSFA detectors -- the 3x3 stride-2
    transposed convolution (heal_deconv3x3_s2) and the attention blend (heal_ssfa_blend) with their host-side support rules, and
    the reader of HEAL_SSFA_FUSED.  Every build exports them; like signatures_ext() they are outside the versioned inference ABI."""
    with open(HEADER_SSFA) as f:
        return parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def signatures_pose():
    """{name: (restype, argtypes)} of include/heal_amd_pose.h: CoAlign's agent-object pose graph -- clustering of every agent's
    boxes and the Levenberg-Marquardt solve for a batch of samples (heal_pose_graph_align with its host-side support and
    workspace rules).  Every build exports them; like signatures_ext() they are outside the versioned inference ABI."""
    with open(HEADER_POSE) as f:
        return parse_prototypes(f.read())


def declared_symbols(experimental=False):
    """Function names declared in include/heal_amd.h (the shipped C ABI), or with experimental=True in
    include/heal_amd_experimental.h."""
    return sorted(signatures(bool(experimental)))


def header_define(name, header=None):
    """The value of `#define name <integer>` in include/heal_amd.h (or in `header`): the ABI version and the kernels'
    compile-time limits."""
    header = header or HEADER
    with open(header) as f:
        m = re.search(rf"^[ \t]*#define\s+{name}\s+(\d+)\b", f.read(), re.M)
    if not m:
        raise HealAmdError(f"{header} does not define {name}")
    return int(m.group(1))


def abi_version_of_header():
    return header_define("HEAL_AMD_ABI_VERSION")


def lib():
    """Load libheal_amd.so (raises if it has not been built: python -m heal_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HealAmdError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -m heal_amd.build`); heal_amd has no CPU fallback")
        # torch ships its own libamdhip64; it must be the HIP runtime of the process, so make sure it
        # is loaded before libheal_amd.so pulls in a second copy from /opt/rocm (two runtimes in one
        # process do not share devices, streams or allocations).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**signatures(), **signatures_train(), **signatures_ext(), **signatures_train_attn(),
                                  **signatures_train_bn(), **signatures_train_warp(), **signatures_center(),
                                  **signatures_comm(), **signatures_unc(), **signatures_roi(), **signatures_align(),
                                  **signatures_ssfa(), **signatures_pose()}.items():
            if not hasattr(L, name):
                continue  # declared but not built yet -> surfaces in call() / the symbol test
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        # The argument lists belong to ONE version of the C ABI: a stale library paired with newer Python (or the reverse)
        # would be called with the wrong arguments and corrupt memory silently.
        want = abi_version_of_header()
        got = int(L.heal_abi_version()) if hasattr(L, "heal_abi_version") else -1
        if got != want:
            raise HealAmdError(f"{LIB_PATH} has C-ABI version {got}, include/heal_amd.h declares {want}: rebuild it "
                               "(python -m heal_amd.build --force)")
        _lib = L
    return _lib


# HEAL_TRACE_CALLS=1: debugging aid for GPU memory faults (a fault kills the process without a Python traceback).  Every C-ABI call
# is announced on stderr BEFORE it is issued and the device is synchronised AFTER it (outside stream captures), so the last line
# printed names the faulting operator.  =2 also prints the pointer / integer arguments.
_TRACE = switches.number("HEAL_TRACE_CALLS")


def _trace_call(name, args):
    import sys
    import torch
    cap = torch.cuda.is_current_stream_capturing()
    extra = ""
    if _TRACE >= 2:
        extra = " " + " ".join(hex(a.value or 0) if isinstance(a, ctypes.c_void_p) else str(a) for a in args
                               if isinstance(a, (int, float, ctypes.c_void_p)))
    print(f"[heal pid {os.getpid()}] {'capture ' if cap else ''}{name}{extra}", file=sys.stderr, flush=True)


def _trace_done(name):
    import sys
    import torch
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize()
        print(f"[heal pid {os.getpid()}]   ok {name}", file=sys.stderr, flush=True)


# ---- HEAL_GRAPH_GUARD=1: pointer ownership of captured graphs ---------------------------------------------------------
# A captured HIP graph has every address it was handed baked in; nothing in the runtime notices when one of them is later freed (scratch
# (ops._workspace) and weight-derived tensors (heal_amd/derived.py) a graph may read are retired, never freed).  In guard mode every device address passed through the C ABI
# DURING a capture is logged; whoever owns the graph takes the log (guard_take) and has it verified before replays (guard_check): each
# address must still lie in memory the caching allocator has handed out -- an active block of the ordinary pool, or any block of a
# graph-private pool that is still mapped (tensors allocated and released inside a capture live there for the life of their graph).
_GUARD = switches.on("HEAL_GRAPH_GUARD")
_guard_log = []


def _segments():
    import torch
    segs = []
    for seg in torch.cuda.memory_snapshot():
        blocks, addr = [], seg["address"]
        for b in seg["blocks"]:
            a = b.get("address", addr)
            blocks.append((a, a + b["size"], b["state"]))
            addr = a + b["size"]
        pool = tuple(seg.get("segment_pool_id", (0, 0)))
        segs.append((seg["address"], seg["address"] + seg["total_size"], pool != (0, 0), blocks))
    segs.sort()
    return segs


def _locate(segs, addr):
    """-> None (no mapped segment: a host pointer or freed memory) | (private_pool, block_state)."""
    import bisect
    i = bisect.bisect_right(segs, (addr, float("inf"), True, [])) - 1
    if i < 0 or not (segs[i][0] <= addr < segs[i][1]):
        return None
    for lo, hi, state in segs[i][3]:
        if lo <= addr < hi:
            return segs[i][2], state
    return segs[i][2], "unknown"


def guard_begin():
    """Start of an OWNING capture (and every failure path of one): drop whatever earlier captures left in the log.  A capture that
    failed or was aborted never reaches guard_take(); without this its addresses -- tensors legitimately freed since -- would be
    inherited by the next owner and reported as 'freed' on its replays, and the log would grow without bound."""
    global _guard_log
    _guard_log = []


def guard_take():
    """The device addresses logged by captures since the last call: [(entry point, address)] (empty when the guard is off)."""
    global _guard_log
    log, _guard_log = _guard_log, []
    if not log:
        return []
    segs = _segments()
    seen, out = set(), []
    for name, addr in log:
        if addr not in seen and _locate(segs, addr) is not None:     # (host arrays also travel as void*: not guarded)
            seen.add(addr)
            out.append((name, addr))
    return out


def guard_check(entries, what="captured graph"):
    """Raise HealAmdError if any logged address no longer belongs to live allocator memory (see above).  One allocator snapshot."""
    if not entries:
        return
    segs = _segments()
    for name, addr in entries:
        where = _locate(segs, addr)
        if where is None:
            raise HealAmdError(f"{what}: {name} was captured with device address {addr:#x}, which is no longer mapped "
                               "(its tensor was freed and the memory returned to the driver)")
        private, state = where
        if not private and state != "active_allocated":
            raise HealAmdError(f"{what}: {name} was captured with device address {addr:#x}, whose block is now '{state}' "
                               "(its tensor was freed: a replay would read or overwrite somebody else's memory)")


def guard_note(name, addresses):
    """Log device addresses that reach an entry point inside a HOST array of pointers (the *_levels / *_agents entries), which
    call() cannot see among its arguments."""
    if _GUARD:
        import torch
        if torch.cuda.is_current_stream_capturing():
            _guard_log.extend((name, int(a)) for a in addresses if a)


def call(name, *args):
    """Call an int-returning entry point; raise HealAmdError with heal_last_error() on failure."""
    L = lib()
    if not hasattr(L, name):
        raise HealAmdError(f"libheal_amd.so does not export {name}")
    if _TRACE:
        _trace_call(name, args)
    if _GUARD:
        import torch
        if torch.cuda.is_current_stream_capturing():
            _guard_log.extend((name, a.value) for a in args if isinstance(a, ctypes.c_void_p) and a.value)
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise HealAmdError(f"{name} failed: {L.heal_last_error().decode(errors='replace')}")
    if _TRACE:
        _trace_done(name)


def query(name, *args):
    """Call a size_t-returning workspace query."""
    L = lib()
    if not hasattr(L, name):
        raise HealAmdError(f"libheal_amd.so does not export {name}")
    return int(getattr(L, name)(*args))
