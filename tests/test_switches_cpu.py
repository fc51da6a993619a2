"""heal_amd/switches.py is the one declaration and the one reader of the HEAL_* environment switches: the package's sources, the
library's getenv sites and README.md's table are checked against it, and its answers against the decisions the code took before
the switches were gathered there (transcribed by hand, with the file:line of the expression they were read from at commit
02dcf47).  No GPU, no library."""
import glob
import os
import re
import warnings

import pytest

from heal_amd import switches
from heal_amd._capi import HealAmdError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heal_amd")
READERS = ("python", "build")


def _python_sources():
    return sorted(p for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)
                  if os.path.abspath(p) != os.path.abspath(switches.__file__))


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _clear(monkeypatch):
    for k in [k for k in os.environ if k.startswith("HEAL_")]:
        monkeypatch.delenv(k)


# ------------------------------------------------------------------------------------------------------------- 1. single reader
def test_no_other_file_reads_a_heal_variable():
    direct = re.compile(r"""(?:environ|getenv\s*\()[^\n]*["']HEAL_""")
    found = [f"{os.path.relpath(p, ROOT)}:{i}" for p in _python_sources()
             for i, line in enumerate(_text(p).splitlines(), 1) if direct.search(line)]
    assert found == []


def test_accessor_names_are_declared_and_every_declared_name_is_read():
    call = re.compile(r"switches\.(on|get|number)\(\s*([^),]*)")
    literal = re.compile(r'"(HEAL_[A-Z0-9_]+)"')
    kinds = {"on": ("flag",), "get": ("choice", "path"), "number": ("int", "float")}
    read = set()
    for p in _python_sources():
        for fn, arg in call.findall(_text(p)):
            m = literal.fullmatch(arg.strip())
            assert m, f"{os.path.relpath(p, ROOT)}: switches.{fn}({arg}...) does not name its switch literally"
            name = m.group(1)
            assert name in switches.SWITCHES, f"{os.path.relpath(p, ROOT)}: {name} is not declared"
            sw = switches.SWITCHES[name]
            assert sw.where in READERS and sw.kind in kinds[fn], (name, fn, sw)
            read.add(name)
    assert read == {n for n, sw in switches.SWITCHES.items() if sw.where in READERS}


def test_table_is_well_formed():
    for name, sw in switches.SWITCHES.items():
        assert re.fullmatch(r"HEAL_[A-Z0-9_]+", name) and sw.where in ("python", "build", "library", "bench"), name
        if sw.where not in READERS:
            assert sw.kind is None, name
        elif sw.kind == "flag":
            assert sw.choices == ("0", "1") and sw.default in sw.choices, name
        elif sw.kind == "choice":
            assert sw.default in sw.choices and all(isinstance(c, str) for c in sw.choices), name
        elif sw.kind == "int":
            assert sw.default is None or sw.choices is None or sw.default in sw.choices, name
        else:
            assert sw.kind in ("float", "path"), name


# ------------------------------------------------------------------------------------------------------------- 2. library names
def test_library_names_are_the_getenv_sites_of_csrc():
    site = re.compile(r'(?:getenv|HEAL_DEBUG_ENV)\s*\(\s*"(HEAL_[A-Z0-9_]+)"')
    found = set()
    for pat in ("*.hip", "*.h"):
        for p in glob.glob(os.path.join(PKG, "csrc", "**", pat), recursive=True):
            found |= set(site.findall(_text(p)))
    assert found == {n for n, sw in switches.SWITCHES.items() if sw.where == "library"}


# -------------------------------------------------------------------------------------------------------------------- 3. README
def _readme_table():
    rows, inside = [], False
    for line in _text(os.path.join(ROOT, "README.md")).splitlines():
        if line.startswith("## "):
            inside = line.startswith("## Switches")
        elif inside and line.startswith("|"):
            rows.append(line)
    assert len(rows) > 10
    return "\n".join(rows)


def test_readme_table_and_declaration_agree():
    tokens = set(re.findall(r"HEAL_[A-Z0-9_]+", _readme_table()))
    defines = set()
    for p in glob.glob(os.path.join(ROOT, "include", "heal_amd*.h")):
        defines |= set(re.findall(r"^[ \t]*#\s*define\s+(HEAL_[A-Z0-9_]+)", _text(p), re.M))
    assert sorted(set(switches.SWITCHES) - tokens) == []
    assert sorted(tokens - set(switches.SWITCHES) - defines) == []


# ------------------------------------------------------------------------------------------- 4. same decisions as before
T, F = True, False
# (switch, value | None for unset, what on / get / number returns).  A flag's answer is "the switch is on", i.e. the truth of the
# former comparison; a choice's answer is the text the former comparison saw, with the former default when unset.
ANSWERS = [
    ("HEAL_AMD_LIB", None, ""), ("HEAL_AMD_LIB", "/x/lib.so", "/x/lib.so"),                     # _capi.py:12   get(..) or <default path>
    ("HEAL_TRACE_CALLS", None, 0), ("HEAL_TRACE_CALLS", "0", 0), ("HEAL_TRACE_CALLS", "1", 1),  # _capi.py:135  int(get(.., "0") or 0)
    ("HEAL_TRACE_CALLS", "2", 2),
    ("HEAL_GRAPH_GUARD", None, F), ("HEAL_GRAPH_GUARD", "0", F), ("HEAL_GRAPH_GUARD", "1", T),  # _capi.py:163  get(.., "0") == "1"
    ("HEAL_BUILD_EXPERIMENTAL", None, F), ("HEAL_BUILD_EXPERIMENTAL", "0", F),                  # build.py:40   get(.., "0") == "1"
    ("HEAL_BUILD_EXPERIMENTAL", "1", T),
    ("HEAL_CONV1X1", None, T), ("HEAL_CONV1X1", "0", F), ("HEAL_CONV1X1", "1", T),              # bev_blocks.py:40   get(.., "1") == "1"
    ("HEAL_CONV3X3", None, T), ("HEAL_CONV3X3", "0", F), ("HEAL_CONV3X3", "1", T),              # bev_blocks.py:41   get(.., "1") == "1"
    ("HEAL_CONV_GEMM", None, T), ("HEAL_CONV_GEMM", "0", F), ("HEAL_CONV_GEMM", "1", T),        # ops.py:2920, 2945  get(.., "1") == "1"
    ("HEAL_CONV_GRAD", None, ""), ("HEAL_CONV_GRAD", "kernel", "kernel"),                       # ops.py:3040   get(.., "") == "kernel"
    ("HEAL_CONV_GRAD", "torch", "torch"),
    ("HEAL_C1_KSPLIT", None, None), ("HEAL_C1_KSPLIT", "0", 0), ("HEAL_C1_KSPLIT", "7", 7),     # ops.py:2612-2613  int(env) if set
    ("HEAL_C1_KSPLIT", "1000", 1000),
    ("HEAL_C1_TILED", None, "0"), ("HEAL_C1_TILED", "0", "0"), ("HEAL_C1_TILED", "1", "1"),     # ops.py:2658   get(.., "0")
    ("HEAL_C1_TILED", "force", "force"),
    ("HEAL_ARITH", None, ""), ("HEAL_ARITH", "f32", "f32"), ("HEAL_ARITH", "bf16x6", "bf16x6"),  # ops.py:2671   get(.., "")
    ("HEAL_ARITH", "bf16x9", "bf16x9"),
    ("HEAL_C3_ALGO", None, ""), ("HEAL_C3_ALGO", "direct", "direct"),                           # ops.py:2903, 2910  get(.., "")
    ("HEAL_C3_ALGO", "winograd", "winograd"), ("HEAL_C3_ALGO", "winograd4", "winograd4"),
    ("HEAL_C3_KSPLIT", None, None), ("HEAL_C3_KSPLIT", "1", 1), ("HEAL_C3_KSPLIT", "64", 64),   # ops.py:2975-2976  int(env) if set
    ("HEAL_WG_WAVES", None, None), ("HEAL_WG_WAVES", "4", 4), ("HEAL_WG_WAVES", "8", 8),        # ops.py:2841-2843  "4" | "8" -> int
    ("HEAL_WG_KC", None, 8), ("HEAL_WG_KC", "8", 8), ("HEAL_WG_KC", "16", 16),                  # ops.py:2852-2853, 2863  get(.., "8") == "16"
    ("HEAL_GCONV_MFMA", None, "1"), ("HEAL_GCONV_MFMA", "1", "1"), ("HEAL_GCONV_MFMA", "s", "s"),  # ops.py:2524   get(.., "1")
    ("HEAL_GCONV_MFMA", "0", "0"), ("HEAL_GCONV_MFMA", "16", "16"), ("HEAL_GCONV_MFMA", "8", "8"),
    ("HEAL_FUSED_BOTTLENECK", None, F), ("HEAL_FUSED_BOTTLENECK", "0", F),                      # bev_blocks.py:259  get(.., "0") != "1": off
    ("HEAL_FUSED_BOTTLENECK", "1", T),
    ("HEAL_STAGE_CHUNK_MB", None, 0.0), ("HEAL_STAGE_CHUNK_MB", "0", 0.0),                      # bev_blocks.py:325  float(get(.., "0"))
    ("HEAL_STAGE_CHUNK_MB", "110", 110.0), ("HEAL_STAGE_CHUNK_MB", "62.5", 62.5),
    ("HEAL_PILLAR_STEM", None, "2"), ("HEAL_PILLAR_STEM", "1", "1"), ("HEAL_PILLAR_STEM", "2", "2"),  # ops.py:452   get(.., "2") == "1"
    ("HEAL_K2_POOLED", None, T), ("HEAL_K2_POOLED", "0", F), ("HEAL_K2_POOLED", "1", T),        # heter_encoders.py:45   get(.., "1") == "1"
    ("HEAL_K2_BACKWARD", None, T), ("HEAL_K2_BACKWARD", "0", F), ("HEAL_K2_BACKWARD", "1", T),  # heter_encoders.py:92   get(.., "1") == "1"
    ("HEAL_LSS_PATH", None, ""), ("HEAL_LSS_PATH", "fused", "fused"), ("HEAL_LSS_PATH", "walk", "walk"),  # ops.py:1431  get(.., "") != "sorted"
    ("HEAL_LSS_PATH", "sorted", "sorted"),
    ("HEAL_K4_POOLED", None, T), ("HEAL_K4_POOLED", "0", F), ("HEAL_K4_POOLED", "1", T),        # heter_encoders.py:257  get(.., "1") == "1"
    ("HEAL_K4_BACKWARD", None, T), ("HEAL_K4_BACKWARD", "0", F), ("HEAL_K4_BACKWARD", "1", T),  # heter_encoders.py:298  get(.., "1") == "1"
    ("HEAL_K4_MULTI", None, F), ("HEAL_K4_MULTI", "0", F), ("HEAL_K4_MULTI", "1", T),           # _heter_common.py:148   get(.., "0") == "1"
    ("HEAL_PARALLEL_MODALITIES", None, T), ("HEAL_PARALLEL_MODALITIES", "0", F),                # _heter_common.py:167   get(.., "1") != "1": off
    ("HEAL_PARALLEL_MODALITIES", "1", T),
    ("HEAL_DEFER_VOXELIZE", None, F), ("HEAL_DEFER_VOXELIZE", "0", F),                          # sp_voxel_preprocessor.py:34, voxel_postprocessor.py:48
    ("HEAL_DEFER_VOXELIZE", "1", T),                                                            #   get(.., "0") == "1"
    ("HEAL_INFERENCE_ONLY", None, F), ("HEAL_INFERENCE_ONLY", "0", F),                          # voxel_postprocessor.py:51  get(.., "0") == "1"
    ("HEAL_INFERENCE_ONLY", "1", T),
    ("HEAL_SP_TILES", None, T), ("HEAL_SP_TILES", "0", F), ("HEAL_SP_TILES", "1", T),           # ops.py:1694   get(.., "1") != "0"
    ("HEAL_SP_RULEBOOK", None, "rank"), ("HEAL_SP_RULEBOOK", "rank", "rank"),                   # ops.py:1738, 1829  get(.., "rank")
    ("HEAL_SP_RULEBOOK", "hash", "hash"),
    ("HEAL_SP_ROOT", None, "rank"), ("HEAL_SP_ROOT", "rank", "rank"), ("HEAL_SP_ROOT", "sort", "sort"),  # ops.py:1738  get(.., "rank")
    ("HEAL_SP_SLOT_SITES", None, 64), ("HEAL_SP_SLOT_SITES", "64", 64),                         # ops.py:1797   int(get(.., 0)) or 64
    ("HEAL_SP_SLOT_SITES", "128", 128),
    ("HEAL_SP_WGRAD", None, T), ("HEAL_SP_WGRAD", "0", F), ("HEAL_SP_WGRAD", "1", T),           # sparse_backbone_3d.py:73   get(.., "1") == "1"
    ("HEAL_SP_GRAD", None, "sparse"), ("HEAL_SP_GRAD", "sparse", "sparse"),                     # sparse_backbone_3d.py:202  get(.., "sparse") != "dense"
    ("HEAL_SP_GRAD", "dense", "dense"),
    ("HEAL_K5_LEVELS", None, T), ("HEAL_K5_LEVELS", "0", F), ("HEAL_K5_LEVELS", "1", T),        # pyramid_fuse.py:270, 389  get(.., "1") == "1"
    ("HEAL_K5_BACKWARD", None, T), ("HEAL_K5_BACKWARD", "0", F), ("HEAL_K5_BACKWARD", "1", T),  # pyramid_fuse.py:72   get(.., "1") == "1"
    ("HEAL_PYRAMID_CAMCROP", None, T), ("HEAL_PYRAMID_CAMCROP", "0", F),                        # pyramid_fuse.py:220  get(.., "1") != "1": off
    ("HEAL_PYRAMID_CAMCROP", "1", T),
    ("HEAL_PYRAMID_LEAN", None, T), ("HEAL_PYRAMID_LEAN", "0", F), ("HEAL_PYRAMID_LEAN", "1", T),  # pyramid_fuse.py:270  get(.., "1") != "1": off
    ("HEAL_ATTN_GRAD", None, "kernel"), ("HEAL_ATTN_GRAD", "kernel", "kernel"),                 # v2xvit_basic.py:145, fusion_in_one.py:74
    ("HEAL_ATTN_GRAD", "torch", "torch"),                                                       #   get(.., "kernel") != "torch"
    ("HEAL_WATTN_GRAD", None, "torch"), ("HEAL_WATTN_GRAD", "torch", "torch"),                  # v2xvit_basic.py:238  get(.., "torch") == "kernel"
    ("HEAL_WATTN_GRAD", "kernel", "kernel"),
    ("HEAL_V2XVIT_FUSED", None, T), ("HEAL_V2XVIT_FUSED", "0", F), ("HEAL_V2XVIT_FUSED", "1", T),  # v2xvit_basic.py:38   get(.., "1") == "0": off
    ("HEAL_V2XVIT_EGO_TAIL", None, T), ("HEAL_V2XVIT_EGO_TAIL", "0", F),                        # v2xvit_basic.py:431  get(.., "1") == "1"
    ("HEAL_V2XVIT_EGO_TAIL", "1", T),
    ("HEAL_V2XVIT_STRIPES", None, T), ("HEAL_V2XVIT_STRIPES", "0", F),                          # dist.py:891   get(.., "1") != "0"
    ("HEAL_V2XVIT_STRIPES", "1", T),
    ("HEAL_COBEVT_FUSED", None, T), ("HEAL_COBEVT_FUSED", "0", F), ("HEAL_COBEVT_FUSED", "1", T),  # swap_fusion_modules.py:30  get(.., "1") == "0": off
    ("HEAL_V2VNET_FUSED", None, T), ("HEAL_V2VNET_FUSED", "0", F), ("HEAL_V2VNET_FUSED", "1", T),  # fusion_in_one.py:384  get(.., "1") != "0"
    ("HEAL_V2V_TH", None, None), ("HEAL_V2V_TH", "4", 4), ("HEAL_V2V_TH", "8", 8), ("HEAL_V2V_TH", "16", 16),  # ops.py:1255-1257
    ("HEAL_V2V_SPLIT", None, None), ("HEAL_V2V_SPLIT", "1", 1), ("HEAL_V2V_SPLIT", "3", 3),     # ops.py:1265-1266  int(env) if set
    ("HEAL_MSATT_FUSED", None, T), ("HEAL_MSATT_FUSED", "0", F), ("HEAL_MSATT_FUSED", "1", T),  # fusion_in_one.py:496  get(.., "1") != "0"
    ("HEAL_DISCO_FUSED", None, T), ("HEAL_DISCO_FUSED", "0", F), ("HEAL_DISCO_FUSED", "1", T),  # fusion_in_one.py:248  get(.., "1") != "0"
    ("HEAL_LOSS_FUSED", None, T), ("HEAL_LOSS_FUSED", "0", F), ("HEAL_LOSS_FUSED", "1", T),     # ops.py:2099   get(.., "1") != "0"
    ("HEAL_KD_FUSED", None, T), ("HEAL_KD_FUSED", "0", F), ("HEAL_KD_FUSED", "1", T),           # ops.py:2038   get(.., "1") != "0"
    ("HEAL_EVAL_FUSED", None, T), ("HEAL_EVAL_FUSED", "0", F), ("HEAL_EVAL_FUSED", "1", T),     # eval_utils.py:70  get(.., "1") != "0"
    ("HEAL_LATE_FUSED", None, T), ("HEAL_LATE_FUSED", "0", F), ("HEAL_LATE_FUSED", "1", T),     # voxel_postprocessor.py:263  get(.., "1") == "0": off
    ("HEAL_COLLECTIVE", None, "gather"), ("HEAL_COLLECTIVE", "gather", "gather"),               # dist.py:180-181  get(.., "gather") in (...)
    ("HEAL_COLLECTIVE", "all_gather", "all_gather"), ("HEAL_COLLECTIVE", "p2p", "p2p"),
    ("HEAL_SPLIT", None, "levels"), ("HEAL_SPLIT", "levels", "levels"),                         # dist.py:381-382  get(.., "levels") == "compressed"
    ("HEAL_SPLIT", "compressed", "compressed"),
]


def _ask(name):
    kind = switches.SWITCHES[name].kind
    return {"flag": switches.on, "choice": switches.get, "path": switches.get}.get(kind, switches.number)(name)


def test_answers_table_covers_every_switch_and_value():
    seen = {}
    for name, value, _ in ANSWERS:
        seen.setdefault(name, set()).add(value)
    readers = {n: sw for n, sw in switches.SWITCHES.items() if sw.where in READERS}
    assert set(seen) == set(readers)
    for name, sw in readers.items():
        assert None in seen[name], name
        if isinstance(sw.choices, tuple):
            assert {str(c) for c in sw.choices if c != ""} <= seen[name], name
        else:
            assert len(seen[name]) >= 2, name


@pytest.mark.parametrize("name,value,want", ANSWERS, ids=[f"{n}={'unset' if v is None else v}" for n, v, _ in ANSWERS])
def test_accessor_gives_the_former_decision(name, value, want, monkeypatch):
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv(name, value)
    got = _ask(name)
    assert got == want and type(got) is type(want)


def test_empty_text_counts_as_unset(monkeypatch):
    """scripts/split_gemm_bench.py restores HEAL_ARITH with "": exact fp32, as ops.py:2671-2672 answered."""
    from heal_amd import ops
    _clear(monkeypatch)
    monkeypatch.setenv("HEAL_ARITH", "")
    monkeypatch.setenv("HEAL_LOSS_FUSED", "")
    assert switches.get("HEAL_ARITH") == "" and ops.arith_products() == 0 and switches.on("HEAL_LOSS_FUSED") is True


# the switches that were read at more than one place, or through a function that other modules and tests call: one row per meaning
def _site_cases():
    from heal_amd import ops
    from heal_amd.opencood.models.sub_modules import bev_blocks
    from heal_amd.opencood.utils import eval_utils
    small, big = (1, 16, 16, 16), (1, 64, 256, 256)           # 1 and 256 Winograd blocks: below and above the 96-block crossover
    wg4 = lambda: ops.conv3x3_winograd4_ok(*small)            # noqa: E731
    rows = []
    # HEAL_C3_ALGO  ops.py:2910-2916 (conv3x3_algo), ops.py:2903 (conv3x3_winograd4_ok, in an experimental build)
    for value, s1_small, s1_big, w4 in ((None, "direct", "winograd", F), ("direct", "direct", "direct", F),
                                        ("winograd", "winograd", "winograd", F), ("winograd4", "winograd", "winograd", T)):
        env = {"HEAL_C3_ALGO": value}
        rows += [(env, lambda: ops.conv3x3_algo(1, *small), s1_small), (env, lambda: ops.conv3x3_algo(1, *big), s1_big),
                 (env, lambda: ops.conv3x3_algo(2, *big), "direct"), (env, wg4, w4)]
    # HEAL_SP_RULEBOOK x HEAL_SP_ROOT  ops.py:1738 (root: rank only if both say rank), ops.py:1829 (layers: rank unless hash)
    for book, root, root_rank, layer_rank in ((None, None, T, T), ("rank", None, T, T), ("rank", "rank", T, T), (None, "rank", T, T),
                                              (None, "sort", F, T), ("rank", "sort", F, T), ("hash", None, F, F),
                                              ("hash", "rank", F, F), ("hash", "sort", F, F)):
        env = {"HEAL_SP_RULEBOOK": book, "HEAL_SP_ROOT": root}
        rows += [(env, ops.sp_root_rank_enabled, root_rank), (env, ops.sp_rank_enabled, layer_rank)]
    for value, want in ((None, T), ("0", F), ("1", T)):
        rows += [({"HEAL_LOSS_FUSED": value}, ops.loss_fused_enabled, want),                          # ops.py:2099
                 ({"HEAL_SP_TILES": value}, ops.sp_tiles_enabled, want),                              # ops.py:1694
                 ({"HEAL_EVAL_FUSED": value}, eval_utils.fused_enabled, want),                        # eval_utils.py:70
                 ({"HEAL_CONV_GEMM": value}, lambda: ops.conv_gemm_supported(32, 128, 8), want),      # ops.py:2920
                 ({"HEAL_CONV_GEMM": value}, lambda: ops.conv7x7_s2_supported(32, 64, 16), want),     # ops.py:2945
                 ({"HEAL_CONV1X1": value}, bev_blocks.conv1x1_enabled, want),                         # bev_blocks.py:40
                 ({"HEAL_CONV3X3": value}, bev_blocks.conv3x3_enabled, want)]                         # bev_blocks.py:41
    for value, want in ((None, F), ("torch", F), ("kernel", T)):
        rows.append(({"HEAL_CONV_GRAD": value}, ops.conv_grad_enabled, want))                         # ops.py:3040
    for value, want in ((None, 0), ("f32", 0), ("bf16x6", 6), ("bf16x9", 9)):
        rows.append(({"HEAL_ARITH": value}, ops.arith_products, want))                                # ops.py:2671-2672
    for value, want in ((None, T), ("fused", T), ("walk", T), ("sorted", F)):
        rows.append(({"HEAL_LSS_PATH": value}, lambda: ops.bev_pool_pm_supported(48, 42, 64), want))  # ops.py:1431
    for value, small_grid, big_grid in ((None, 4, 8), ("4", 4, 4), ("8", 8, 8)):                      # ops.py:2841-2845
        rows += [({"HEAL_WG_WAVES": value}, lambda: ops.conv3x3_winograd_waves(*small), small_grid),
                 ({"HEAL_WG_WAVES": value}, lambda: ops.conv3x3_winograd_waves(8, 64, 128, 128), big_grid)]
    for value, mean, mx in ((None, 8, 4), ("4", 4, 4), ("8", 8, 8), ("16", 16, 16)):                  # ops.py:1255-1258
        rows += [({"HEAL_V2V_TH": value}, lambda: ops.v2v_message_tile_h(1, 64, 16, 16, 0), mean),
                 ({"HEAL_V2V_TH": value}, lambda: ops.v2v_message_tile_h(1, 64, 16, 16, 1), mx)]
    for value, want in ((None, 2), ("1", 1), ("3", 3), ("9", 5)):                                     # ops.py:1264-1268: 256 blocks, 5 agents
        rows.append(({"HEAL_V2V_SPLIT": value}, lambda: ops.v2v_message_nsplit(1, 5, 64, 128, 256, 8), want))
    for value, want in ((None, 18), ("0", 1), ("1", 1), ("2", 2), ("5", 5), ("1000", 36)):            # ops.py:2610-2617: 36 chunks, 3 blocks
        rows.append(({"HEAL_C1_KSPLIT": value}, lambda: ops.conv1x1_ksplit(1, 1152, 64, 192), want))
    for value, want in ((None, 4), ("0", 1), ("1", 1), ("2", 2), ("1000", 54)):                       # ops.py:2973-2980: 54 chunks, 192 blocks
        rows.append(({"HEAL_C3_KSPLIT": value}, lambda: ops.conv3x3_winograd_ksplit(4, 432, 512, 24, 32, 4), want))
    for value, want in ((None, 8), ("8", 8), ("16", 16)):                                             # ops.py:2852-2854 (experimental build)
        rows.append(({"HEAL_WG_KC": value}, lambda: ops.conv3x3_winograd_kc(32, 8, 16, 16), want))
    for value, want in ((None, F), ("0", F), ("1", F), ("force", T)):                                 # ops.py:2658-2665: 2 blocks, cin 32
        rows.append(({"HEAL_C1_TILED": value}, lambda: ops.conv1x1_tiled_ok(1, 32, 64, 256), want))
    for value, want in ((None, F), ("0", F), ("1", T), ("force", T)):                                 # ... 256 blocks, cin 128
        rows.append(({"HEAL_C1_TILED": value}, lambda: ops.conv1x1_tiled_ok(1, 128, 128, 256 * 128), want))
    return rows


def test_sites_take_the_former_decisions(monkeypatch):
    from heal_amd import ops
    monkeypatch.setattr(ops, "experimental_build", lambda: True)     # no library here; winograd4 / kc 16 / tiled also ask for one
    for i, (env, probe, want) in enumerate(_site_cases()):
        _clear(monkeypatch)
        for k, v in env.items():
            if v is not None:
                monkeypatch.setenv(k, v)
        got = probe()
        assert got == want and type(got) is type(want), (i, env, got, want)


# -------------------------------------------------------------------------------------------------------------- 5. loud failure
@pytest.mark.parametrize("name,value", [("HEAL_LOSS_FUSED", "true"), ("HEAL_K5_LEVELS", "true"), ("HEAL_WG_WAVES", "6"),
                                        ("HEAL_C1_KSPLIT", "abc"), ("HEAL_SP_RULEBOOK", "foo"), ("HEAL_SP_SLOT_SITES", "x"),
                                        ("HEAL_STAGE_CHUNK_MB", "lots"), ("HEAL_ARITH", "bf16")])
def test_value_outside_the_declared_set_raises(name, value, monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv(name, value)
    with pytest.raises(HealAmdError) as e:
        _ask(name)
    assert name in str(e.value) and value in str(e.value)


def test_invalid_value_raises_inside_the_routing_functions(monkeypatch):
    from heal_amd import ops
    _clear(monkeypatch)
    monkeypatch.setenv("HEAL_C1_KSPLIT", "abc")
    with pytest.raises(HealAmdError, match="HEAL_C1_KSPLIT"):
        ops.conv1x1_ksplit(1, 1152, 64, 192)
    monkeypatch.setenv("HEAL_C3_ALGO", "winograd3")
    with pytest.raises(HealAmdError, match="winograd3"):
        ops.conv3x3_algo(1, 1, 16, 16, 16)


def test_undeclared_name_is_a_key_error_and_so_is_a_name_python_does_not_read():
    for ask in (switches.on, switches.get, switches.number):
        with pytest.raises(KeyError):
            ask("HEAL_NO_SUCH_SWITCH")
        with pytest.raises(KeyError):
            ask("HEAL_SP_CONV")          # the library's
        with pytest.raises(KeyError):
            ask("HEAL_WIRE")             # bench.py's
    with pytest.raises(KeyError):
        switches.on("HEAL_C3_ALGO")      # a choice, not a flag


def test_unknown_name_in_the_environment_warns_once_per_process(monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv("HEAL_TYPO", "1")
    monkeypatch.setenv("HEAL_SP_CONV", "v1")         # the library's: known
    monkeypatch.setenv("HEAL_WIRE", "fp16")          # bench.py's: known
    monkeypatch.setattr(switches, "_names_checked", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        switches.on("HEAL_LOSS_FUSED")
        switches.get("HEAL_C3_ALGO")
        switches.number("HEAL_WG_WAVES")
        switches.on("HEAL_LOSS_FUSED")
    seen = [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(seen) == 1 and "HEAL_TYPO" in str(seen[0].message)
    assert "HEAL_SP_CONV" not in str(seen[0].message) and "HEAL_WIRE" not in str(seen[0].message)


def test_no_warning_without_unknown_names(monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setattr(switches, "_names_checked", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        switches.on("HEAL_LOSS_FUSED")
    assert [w for w in seen if issubclass(w.category, RuntimeWarning)] == []


# ---------------------------------------------------------------------------------------------------------- 6. call-time reading
def test_switches_are_read_when_asked_not_when_imported(monkeypatch):
    from heal_amd import ops
    from heal_amd.opencood.models.sub_modules import bev_blocks
    _clear(monkeypatch)
    assert switches.on("HEAL_LOSS_FUSED") and switches.get("HEAL_C3_ALGO") == "" and ops.conv3x3_algo(1, 1, 16, 16, 16) == "direct"
    assert bev_blocks.conv1x1_enabled() and bev_blocks.conv3x3_enabled()
    monkeypatch.setenv("HEAL_LOSS_FUSED", "0")
    monkeypatch.setenv("HEAL_C3_ALGO", "winograd")
    monkeypatch.setenv("HEAL_CONV1X1", "0")
    monkeypatch.setenv("HEAL_CONV3X3", "0")
    assert not switches.on("HEAL_LOSS_FUSED") and switches.get("HEAL_C3_ALGO") == "winograd"
    assert ops.conv3x3_algo(1, 1, 16, 16, 16) == "winograd"
    assert not bev_blocks.conv1x1_enabled() and not bev_blocks.conv3x3_enabled()
    monkeypatch.delenv("HEAL_CONV1X1")
    assert bev_blocks.conv1x1_enabled() and not bev_blocks.conv3x3_enabled()
