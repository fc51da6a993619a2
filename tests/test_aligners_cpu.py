"""AlignNet's six aligners beyond identity / convnext on the CPU: construction, the reference's state-dict keys in its order, the
reference's recorded outputs (tests/golden/gen_golden_aligners.py; the same composition in the same precision), the gradient path,
and the plumbing of the new entry points (header, ctypes table, switch, README row)."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch

from heal_amd import _capi, configs, switches
from heal_amd.opencood.models.heter_pyramid_collab import HeterPyramidCollab
from heal_amd.opencood.models.sub_modules.bev_blocks import AlignNet
from tests.golden import aligner_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = list(A.CASES)
SYMBOLS = ("heal_align_fused_enabled", "heal_xca_supported", "heal_xca_parts", "heal_xca_range", "heal_xca_workspace", "heal_xca_weights")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "aligners_small.npz"))


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLD, "aligners_state_dict_keys.json")) as f:
        return json.load(f)


def golden_state(gold, name):
    head = name + "/sd/"
    return {k[len(head):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(head)}


def golden_io(gold, name):
    x = gold["input_fanet" if name == "fanet" else "input"]
    y = gold["sdta/hook/1"] if name == "sdta" else gold[name + "/output"]
    return torch.from_numpy(x), y


@pytest.mark.parametrize("name", NAMES)
def test_constructs_with_the_reference_keys_in_order(name, ref_keys):
    model = AlignNet(A.aligner_args(name))
    assert list(model.state_dict()) == ref_keys[name]


@pytest.mark.parametrize("name", NAMES)
def test_reproduces_the_reference_recording(name, gold):
    model = AlignNet(A.aligner_args(name)).eval()
    model.load_state_dict(golden_state(gold, name), strict=True)
    x, want = golden_io(gold, name)
    got = model(x).numpy()
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    print(f"{name}: {err:.3e} of the largest magnitude")
    assert got.shape == want.shape and err <= 1e-5


def test_sdta_blocks_reproduce_the_hooked_outputs(gold):
    model = AlignNet(A.aligner_args("sdta")).eval()
    model.load_state_dict(golden_state(gold, "sdta"), strict=True)
    x = torch.from_numpy(gold["input"])
    for i, block in enumerate(model.channel_align.model):
        x = block(x)
        want = gold[f"sdta/hook/{i}"]
        assert float(np.abs(x.numpy() - want).max()) <= 1e-5 * float(np.abs(want).max()), i


@pytest.mark.parametrize("name", ["convnext", "resnet1x1", "resnet3x3"])
def test_deformable_variants_stay_out_of_scope(name):
    with pytest.raises(NotImplementedError):
        AlignNet({"core_method": name, "args": {"num_of_blocks": 1, "dim": 64, "deform": True}})


def test_unknown_name_and_spatial_align_raise():
    with pytest.raises(NotImplementedError):
        AlignNet({"core_method": "no_such_aligner", "args": {}})
    with pytest.raises(NotImplementedError):
        AlignNet(dict(A.aligner_args("cbam"), spatial_align=True))


def test_collab_model_takes_the_sdta_aligner(ref_keys):
    args = copy.deepcopy(configs.lidar_pyramid([-25.6, -25.6, -3, 25.6, 25.6, 1])["model"]["args"])
    args["m1"]["aligner_args"] = A.aligner_args("sdta")
    model = HeterPyramidCollab(args)
    mine = [k for k in model.state_dict() if k.startswith("aligner_m1.")]
    assert mine == ["aligner_m1." + k for k in ref_keys["sdta"]]


@pytest.mark.grad
@pytest.mark.parametrize("name", NAMES)
def test_backward_gives_finite_gradients_on_every_parameter(name, gold):
    model = AlignNet(A.aligner_args(name)).train()
    model.load_state_dict(golden_state(gold, name), strict=True)
    x, _ = golden_io(gold, name)
    model(x.clone().requires_grad_(True)).square().mean().backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert float(p.grad.abs().max()) > 0, k


def test_align_header_is_bound():
    sig = _capi.signatures_align()
    assert sorted(sig) == sorted(SYMBOLS)
    with open(_capi.HEADER_ALIGN) as f:
        text = f.read()
    assert sorted(set(re.findall(r"\b(heal_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))) == sorted(SYMBOLS)
    import ctypes
    res, args = sig["heal_xca_weights"]
    assert res is ctypes.c_int and len(args) == 13 and args[3:7] == [ctypes.c_int] * 4 and args[8] is ctypes.c_size_t
    assert sig["heal_xca_workspace"][0] is ctypes.c_size_t


def test_switch_is_declared_documented_and_read_by_the_library(monkeypatch):
    """HEAL_ALIGN_FUSED is one of the library's own variables (heal_align_fused_enabled reads it when called)."""
    from heal_amd import ops
    assert switches.SWITCHES["HEAL_ALIGN_FUSED"].where == "library"
    monkeypatch.delenv("HEAL_ALIGN_FUSED", raising=False)
    assert ops.align_fused_enabled() is True
    for text, want in (("0", False), ("1", True), ("", True)):
        monkeypatch.setenv("HEAL_ALIGN_FUSED", text)
        assert ops.align_fused_enabled() is want
    monkeypatch.setenv("HEAL_ALIGN_FUSED", "yes")
    with pytest.raises(_capi.HealAmdError, match="HEAL_ALIGN_FUSED"):
        ops.align_fused_enabled()
    with open(os.path.join(ROOT, "README.md")) as f:
        assert any(line.startswith("| `HEAL_ALIGN_FUSED=0`") for line in f.read().splitlines())
