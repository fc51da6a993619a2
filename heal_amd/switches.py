"""Every HEAL_* environment switch, declared once, and the only code of the package that reads one.

SWITCHES maps a name to (kind, default, choices, where); README.md ("Switches") says what each one does.

  kind    "flag"   "0" | "1"                                              -> on(name)
          "choice" one of `choices`; "" among them stands for "not set"    -> get(name)
          "path"   any text                                                -> get(name)
          "int"    an integer, one of `choices` (a tuple or a range) if given  -> number(name)
          "float"  a number                                                -> number(name)
  where   "python"  read by this package          "build"  read by heal_amd/build.py
          "library" read by getenv / HEAL_DEBUG_ENV in csrc/: named here so that it counts as known, never read or validated
          "bench"   read by bench.py alone: likewise

The accessors read os.environ when they are called.  A variable that is set to the empty string counts as not set.  A value
outside the declared set raises HealAmdError; asking for a name that is not declared (or not Python's to read) is a KeyError.
The first call also warns, once per process, about HEAL_* variables in the environment that are not declared here: a mistyped
name would otherwise select nothing, silently.
"""
import collections
import os
import warnings

Switch = collections.namedtuple("Switch", "kind default choices where")

_ON = Switch("flag", "1", ("0", "1"), "python")
_OFF = Switch("flag", "0", ("0", "1"), "python")
_LIBRARY = Switch(None, None, None, "library")
_BENCH = Switch(None, None, None, "bench")

SWITCHES = {
    # process-wide, read once when heal_amd._capi / heal_amd.build are imported
    "HEAL_AMD_LIB": Switch("path", "", None, "python"),
    "HEAL_TRACE_CALLS": Switch("int", 0, (0, 1, 2), "python"),
    "HEAL_GRAPH_GUARD": _OFF,
    "HEAL_BUILD_EXPERIMENTAL": Switch("flag", "0", ("0", "1"), "build"),
    # dense convolutions
    "HEAL_CONV1X1": _ON,
    "HEAL_CONV3X3": _ON,
    "HEAL_CONV_GEMM": _ON,
    "HEAL_CONV_GRAD": Switch("choice", "", ("", "kernel", "torch"), "python"),
    "HEAL_C1_KSPLIT": Switch("int", None, range(0, 65536), "python"),
    "HEAL_C1_TILED": Switch("choice", "0", ("0", "1", "force"), "python"),
    "HEAL_ARITH": Switch("choice", "", ("", "f32", "bf16x6", "bf16x9"), "python"),
    "HEAL_C3_ALGO": Switch("choice", "", ("", "direct", "winograd", "winograd4"), "python"),
    "HEAL_C3_KSPLIT": Switch("int", None, range(0, 65536), "python"),
    "HEAL_WG_WAVES": Switch("int", None, (4, 8), "python"),
    "HEAL_WG_KC": Switch("int", 8, (8, 16), "python"),
    "HEAL_GCONV_MFMA": Switch("choice", "1", ("1", "s", "0", "16", "8"), "python"),
    "HEAL_FUSED_BOTTLENECK": _OFF,
    "HEAL_STAGE_CHUNK_MB": Switch("float", 0.0, None, "python"),
    # encoders
    "HEAL_PILLAR_STEM": Switch("choice", "2", ("1", "2"), "python"),
    "HEAL_K2_POOLED": _ON,
    "HEAL_K2_BACKWARD": _ON,
    "HEAL_LSS_PATH": Switch("choice", "", ("", "fused", "walk", "sorted"), "python"),
    "HEAL_K4_POOLED": _ON,
    "HEAL_K4_BACKWARD": _ON,
    "HEAL_K4_MULTI": _OFF,
    "HEAL_PARALLEL_MODALITIES": _ON,
    "HEAL_DEFER_VOXELIZE": _OFF,
    "HEAL_INFERENCE_ONLY": _OFF,
    # sparse 3-D convolutions
    "HEAL_SP_TILES": _ON,
    "HEAL_SP_RULEBOOK": Switch("choice", "rank", ("rank", "hash"), "python"),
    "HEAL_SP_ROOT": Switch("choice", "rank", ("rank", "sort"), "python"),
    "HEAL_SP_SLOT_SITES": Switch("int", 64, (64, 128), "python"),
    "HEAL_SP_WGRAD": _ON,
    "HEAL_SP_GRAD": Switch("choice", "sparse", ("sparse", "dense"), "python"),
    # fusion
    "HEAL_K5_LEVELS": _ON,
    "HEAL_K5_BACKWARD": _ON,
    "HEAL_PYRAMID_CAMCROP": _ON,
    "HEAL_PYRAMID_LEAN": _ON,
    "HEAL_ATTN_GRAD": Switch("choice", "kernel", ("kernel", "torch"), "python"),
    "HEAL_WATTN_GRAD": Switch("choice", "torch", ("torch", "kernel"), "python"),
    "HEAL_V2XVIT_FUSED": _ON,
    "HEAL_V2XVIT_EGO_TAIL": _ON,
    "HEAL_V2XVIT_STRIPES": _ON,
    "HEAL_COBEVT_FUSED": _ON,
    "HEAL_V2VNET_FUSED": _ON,
    "HEAL_V2V_TH": Switch("int", None, (4, 8, 16), "python"),
    "HEAL_V2V_SPLIT": Switch("int", None, None, "python"),
    "HEAL_MSATT_FUSED": _ON,
    "HEAL_DISCO_FUSED": _ON,
    # losses, evaluation, post-processing
    "HEAL_LOSS_FUSED": _ON,
    "HEAL_KD_FUSED": _ON,
    "HEAL_EVAL_FUSED": _ON,
    "HEAL_LATE_FUSED": _ON,
    # agent-sharded path
    "HEAL_COLLECTIVE": Switch("choice", "gather", ("gather", "all_gather", "p2p"), "python"),
    "HEAL_SPLIT": Switch("choice", "levels", ("levels", "compressed"), "python"),
    # csrc/
    "HEAL_ALIGN_FUSED": _LIBRARY,       # heal_align_fused_enabled(); the aligners ask the library (ops.align_fused_enabled)
    "HEAL_C1_CFG": _LIBRARY,
    "HEAL_C3_TH": _LIBRARY,
    "HEAL_CANVAS_CG": _LIBRARY,
    "HEAL_CANVAS_NT": _LIBRARY,
    "HEAL_COMM_FUSED": _LIBRARY,
    "HEAL_GC3_DBG": _LIBRARY,
    "HEAL_GCONV_1PX": _LIBRARY,
    "HEAL_GS_TH": _LIBRARY,
    "HEAL_K4_CSPLIT": _LIBRARY,
    "HEAL_K4_DBG": _LIBRARY,
    "HEAL_K5_BLOCKS": _LIBRARY,
    "HEAL_K5_DBG": _LIBRARY,
    "HEAL_PFN_1PW": _LIBRARY,
    "HEAL_PS_DBG": _LIBRARY,
    "HEAL_PYRAMID_ROI": _LIBRARY,       # heal_roi_enabled(); the lean walk asks the library (ops.pyramid_roi_enabled)
    "HEAL_SSFA_FUSED": _LIBRARY,        # heal_ssfa_fused_enabled(); SSFA asks the library (ops.ssfa_fused_enabled)
    "HEAL_SPLIT_DBG": _LIBRARY,
    "HEAL_SPLIT_TILE": _LIBRARY,
    "HEAL_SP_CONV": _LIBRARY,
    "HEAL_SP_DB": _LIBRARY,
    "HEAL_SP_DBG": _LIBRARY,
    "HEAL_SP_M": _LIBRARY,
    "HEAL_SP_TILES_D": _LIBRARY,
    "HEAL_SP_TILES_DBG": _LIBRARY,
    "HEAL_SP_TPSX": _LIBRARY,
    "HEAL_VOX_DENSE": _LIBRARY,
    # bench.py
    "HEAL_DIST_BACKEND": _BENCH,
    "HEAL_FRAMES_IN_FLIGHT": _BENCH,
    "HEAL_MIOPEN_BENCHMARK": _BENCH,
    "HEAL_PREFLIGHT_S": _BENCH,
    "HEAL_WIRE": _BENCH,
}

_names_checked = False


def _value(name, kinds):
    """(declaration, text or default) of a switch this package reads; the text is still unchecked."""
    global _names_checked
    sw = SWITCHES[name]
    if sw.kind not in kinds:
        raise KeyError(f"{name} is a {sw.kind or sw.where} switch: not read with this accessor")
    if not _names_checked:
        _names_checked = True
        unknown = sorted(k for k in os.environ if k.startswith("HEAL_") and k not in SWITCHES)
        if unknown:
            warnings.warn(f"heal_amd: {', '.join(unknown)} in the environment: no such switch (heal_amd/switches.py)",
                          RuntimeWarning, stacklevel=3)
    text = os.environ.get(name, "")
    return sw, (sw.default if text == "" else text)


def _invalid(name, value, allowed):
    from heal_amd._capi import HealAmdError       # here, not at the top: _capi reads its own switches when it is imported
    raise HealAmdError(f"{name}={value!r} is not a valid setting: expected {allowed}")


def on(name):
    """A flag: True for "1", False for "0"."""
    sw, v = _value(name, ("flag",))
    if v not in sw.choices:
        _invalid(name, v, "0 or 1")
    return v == "1"


def get(name):
    """A choice (one of the declared strings; the default when not set) or a path (any text, "" when not set)."""
    sw, v = _value(name, ("choice", "path"))
    if sw.kind == "choice" and v not in sw.choices:
        _invalid(name, v, "one of " + ", ".join(c or "(not set)" for c in sw.choices))
    return v


def number(name):
    """An int or float switch: its value, its default when not set, None when it has neither."""
    sw, v = _value(name, ("int", "float"))
    if v is None or not isinstance(v, str):
        return v
    try:
        n = int(v) if sw.kind == "int" else float(v)
    except ValueError:
        _invalid(name, v, "an integer" if sw.kind == "int" else "a number")
    if sw.choices is not None and n not in sw.choices:
        c = sw.choices
        _invalid(name, v, f"{c.start} .. {c.stop - 1}" if isinstance(c, range) else "one of " + ", ".join(map(str, c)))
    return n
