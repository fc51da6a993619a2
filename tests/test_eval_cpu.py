"""AP evaluation without a GPU: the committed fixture keeps its margins and coverage; the numpy restatement of the reference's
greedy match, voc_ap / calculate_ap / eval_final_results reproduce what the reference recorded; the C ABI declares and exports
the matcher; install_as_opencood exposes the module."""
import os
import sys

import numpy as np
import pytest

from heal_amd import _capi
from heal_amd.opencood.utils import eval_utils as E
from tests.golden import eval_margins as M

NEW_SYMBOLS = ("heal_eval_match_workspace", "heal_eval_match")
FRAMES = ("a", "b")


@pytest.fixture(scope="module")
def g(golden):
    return golden("eval_match")


def frame(g, tag):
    return g[f"{tag}_det"], g[f"{tag}_det_score"], g[f"{tag}_gt_boxes"]


def recorded_stat(g, tag):
    return {thr: {"tp": g[f"{tag}_tp"][t].tolist(), "fp": g[f"{tag}_fp"][t].tolist(), "score": g[f"{tag}_score"][t].tolist(),
                  "gt": int(g[f"{tag}_gt"][t])} for t, thr in enumerate(M.THRESHOLDS)}


def test_fixture_shapes_cover_both_sides_of_one_wave(g):
    assert tuple(g["thresholds"]) == M.THRESHOLDS
    (na, ma), (nb, mb) = [(len(g[f"{t}_det"]), len(g[f"{t}_gt_boxes"])) for t in FRAMES]
    assert 100 <= na <= 160 and 30 <= ma <= 64 and 250 <= nb <= 350 and 64 < mb <= 128


@pytest.mark.parametrize("tag", FRAMES)
def test_fixture_keeps_margins_and_coverage(g, tag):
    cov = M.check(*frame(g, tag), E._greedy_match)
    assert cov["tp_counts"] == g[f"{tag}_tp"].sum(axis=1).tolist()


@pytest.mark.parametrize("tag", FRAMES)
def test_greedy_match_reproduces_reference_lists(g, tag):
    det, score, gt = frame(g, tag)
    order, tp, gi = E._greedy_match(M.iou_matrix(det, gt).astype(np.float32), M.THRESHOLDS, score)
    assert np.array_equal(order, g[f"{tag}_order"]) and np.array_equal(gi, g[f"{tag}_gt_index"])
    for t in range(len(M.THRESHOLDS)):
        assert np.array_equal(tp[t], g[f"{tag}_tp"][t]) and np.array_equal(1 - tp[t].astype(int), g[f"{tag}_fp"][t])
        assert score[order].tolist() == g[f"{tag}_score"][t].tolist()
    assert ((gi >= 0) == (tp == 1)).all()
    for t in range(len(M.THRESHOLDS)):                     # a ground-truth box is matched at most once
        hit = gi[t][gi[t] >= 0]
        assert len(set(hit.tolist())) == len(hit)


def test_greedy_match_differs_from_the_voc_variant(g):
    """The VOC matcher looks at a detection's best box only: on the fixture it must give another answer (the 'pop' cases)."""
    det, score, gt = frame(g, "a")
    iou = M.iou_matrix(det, gt).astype(np.float32)
    order, tp, _ = E._greedy_match(iou, (0.3,), score)
    used, voc = set(), []
    for i in order:
        j = int(np.argmax(iou[i]))
        ok = iou[i, j] >= np.float32(0.3) and j not in used
        used.add(j) if ok else None
        voc.append(int(ok))
    assert voc != tp[0].tolist() and sum(voc) < int(tp[0].sum())


def test_greedy_match_edges():
    iou = np.array([[0.6, 0.6, 0.1], [0.6, 0.6, 0.1], [0.6, 0.6, 0.1], [np.nan, np.nan, 0.2]], np.float32)
    order, tp, gi = E._greedy_match(iou, (0.5, 0.2), np.array([0.5, 0.9, 0.9, 0.1], np.float32))
    assert order.tolist() == [1, 2, 0, 3]                  # equal scores by ascending index
    # the first maximum goes first; a later detection takes the next box; NaN counts as 0; an IoU equal to the threshold
    # (compared in fp32) is a TP: `<` decides
    assert tp.tolist() == [[1, 1, 0, 0], [1, 1, 0, 1]]
    assert gi.tolist() == [[0, 1, -1, -1], [0, 1, -1, 2]]
    order, tp, gi = E._greedy_match(np.zeros((2, 0), np.float32), (0.3,))
    assert tp.tolist() == [[0, 0]] and gi.tolist() == [[-1, -1]]
    order, tp, gi = E._greedy_match(np.zeros((0, 3), np.float32), (0.3,))
    assert tp.shape == (1, 0) and order.shape == (0,)


@pytest.mark.parametrize("tag", FRAMES + ("run",))
def test_calculate_ap_reproduces_reference(g, tag):
    stat = recorded_stat(g, tag)
    for t, thr in enumerate(M.THRESHOLDS):
        ap, mrec, mpre = E.calculate_ap(stat, thr)
        assert ap == float(g[f"{tag}_ap"][t])
        assert mrec == g[f"{tag}_mrec"][t].tolist() and mpre == g[f"{tag}_mpre"][t].tolist()
    assert stat[0.3]["tp"] == g[f"{tag}_tp"][0].tolist()   # calculate_ap leaves result_stat alone


def test_voc_ap_small_case():
    ap, mrec, mpre = E.voc_ap([0.5, 0.5, 1.0], [1.0, 0.5, 2 / 3])
    assert mrec == [0.0, 0.5, 0.5, 1.0, 1.0] and mpre == [1.0, 1.0, 2 / 3, 2 / 3, 0.0]
    assert ap == 0.5 * 1.0 + 0.5 * (2 / 3)


def test_eval_final_results_writes_the_reference_keys(g, tmp_path, capsys):
    import yaml
    stat = recorded_stat(g, "run")
    aps = E.eval_final_results(stat, str(tmp_path))
    assert aps == tuple(float(v) for v in g["run_ap"])
    assert "The Average Precision at IOU 0.3 is" in capsys.readouterr().out
    dumped = yaml.load(open(tmp_path / "eval.yaml"), Loader=yaml.Loader)
    assert set(dumped) == {"ap30", "ap_50", "ap_70", "mpre_50", "mrec_50", "mpre_70", "mrec_70"}
    assert dumped["ap_50"] == aps[1] and dumped["mrec_70"] == g["run_mrec"][2].tolist()
    E.eval_final_results(stat, str(tmp_path), infer_info="late")
    assert os.path.exists(tmp_path / "eval_late.yaml")


def test_gt_only_frame_and_result_stat_layout():
    stat = E.new_result_stat()
    assert stat == {0.3: {"tp": [], "fp": [], "gt": 0, "score": []}, 0.5: {"tp": [], "fp": [], "gt": 0, "score": []},
                    0.7: {"tp": [], "fp": [], "gt": 0, "score": []}}
    E.caluclate_tp_fp(None, None, np.zeros((7, 8, 3), np.float32), stat, 0.5)          # det_boxes None: no device work at all
    E.caluclate_tp_fp_multi(None, None, np.zeros((2, 8, 3), np.float32), stat)
    assert [stat[t]["gt"] for t in (0.3, 0.5, 0.7)] == [2, 9, 2] and stat[0.5]["tp"] == []


def test_abi_declares_and_exports_the_eval_entry_points():
    declared = _capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/heal_amd.h"
        assert name in _capi.signatures(), f"{name} has no ctypes signature"
    assert _capi.abi_version_of_header() == 13             # (12 when these were added, additively; 13: heal_voxelize_layout)
    from heal_amd import build
    build.build()
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libheal_amd.so does not export {name}"
    header = open(_capi.HEADER).read()
    assert "eval_utils.py:40-91" in header and "common_utils.py:230-270" in header
    # the workspace query is host arithmetic: the [n, m_pad] fp32 matrix (m_pad = 64 / 128 / 256) + one maximum per 64 columns
    assert _capi.query("heal_eval_match_workspace", 1024, 256) == 1024 * 256 * 4 + 1024 * 4 * 4
    assert _capi.query("heal_eval_match_workspace", 100, 30) == 100 * 64 * 4 + 512
    assert _capi.query("heal_eval_match_workspace", 100, 65) == 100 * 128 * 4 + 1024
    assert _capi.query("heal_eval_match_workspace", 0, 0) == 512


def test_ops_refuse_cpu_tensors_and_sizes_beyond_the_limits():
    import torch
    from heal_amd import ops
    with pytest.raises(_capi.HealAmdError, match="CUDA"):
        ops.eval_match(torch.zeros(2, 8, 3), torch.zeros(2), torch.zeros(1, 8, 3), (0.5,))
    assert ops.eval_match_supported(1024, 256, 8) and ops.eval_match_supported(0, 0, 1)
    assert not ops.eval_match_supported(1025, 1, 1) and not ops.eval_match_supported(1, 257, 1)
    assert not ops.eval_match_supported(1, 1, 9) and not ops.eval_match_supported(1, 1, 0)


def test_install_as_opencood_exposes_eval_utils():
    from heal_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "opencood" or k.startswith("opencood.")}
    try:
        for k in saved:
            del sys.modules[k]
        compat.install_as_opencood()
        import importlib
        mod = importlib.import_module("opencood.utils.eval_utils")
        assert mod is E
        for name in ("voc_ap", "caluclate_tp_fp", "calculate_ap", "eval_final_results"):
            assert callable(getattr(mod, name))
        assert "utils.eval_utils" in compat._OVERLAY_LEAVES
    finally:
        for k in [k for k in sys.modules if k == "opencood" or k.startswith("opencood.")]:
            del sys.modules[k]
        sys.modules.update(saved)
