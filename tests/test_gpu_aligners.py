"""AlignNet's six aligners beyond identity / convnext on the device, against the reference's recording
(tests/golden/gen_golden_aligners.py): the library-operator path (default), the composition under HEAL_ALIGN_FUSED=0, the `sdta`
blocks one by one, graph capture, and the gradient path."""
import os

import numpy as np
import pytest
import torch

from heal_amd import ops
from heal_amd.opencood.models.sub_modules.bev_blocks import AlignNet
from tests.golden import aligner_cases as A

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(A.CASES)
RTOL = 1e-3                 # the project's bound for fp32 features, of the largest magnitude


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "aligners_small.npz"))


def load(gold, name):
    head = name + "/sd/"
    model = AlignNet(A.aligner_args(name)).eval()
    model.load_state_dict({k[len(head):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(head)}, strict=True)
    x = torch.from_numpy(gold["input_fanet" if name == "fanet" else "input"])
    want = gold["sdta/hook/1"] if name == "sdta" else gold[name + "/output"]
    return model.cuda(), x.cuda(), want


def rel(got, want):
    return float(np.abs(got.detach().cpu().numpy() - want).max()) / float(np.abs(want).max())


@pytest.mark.parametrize("name", NAMES)
def test_library_path_reproduces_the_reference(name, gold, monkeypatch):
    monkeypatch.delenv("HEAL_ALIGN_FUSED", raising=False)
    model, x, want = load(gold, name)
    calls = ops.XCA_CALLS["weights"]
    err = rel(model(x), want)
    print(f"{name}: library path {err:.3e} of the largest magnitude")
    assert err <= RTOL
    assert ops.XCA_CALLS["weights"] - calls == (1 if name == "sdta" else 0)      # the kernel path was the one taken


@pytest.mark.parametrize("name", NAMES)
def test_composition_switch_reproduces_the_reference(name, gold, monkeypatch):
    monkeypatch.setenv("HEAL_ALIGN_FUSED", "0")
    model, x, want = load(gold, name)
    calls = ops.XCA_CALLS["weights"]
    err = rel(model(x), want)
    print(f"{name}: HEAL_ALIGN_FUSED=0 {err:.3e} of the largest magnitude")
    assert err <= RTOL and ops.XCA_CALLS["weights"] == calls


def test_sdta_blocks_one_by_one(gold, monkeypatch):
    monkeypatch.delenv("HEAL_ALIGN_FUSED", raising=False)
    model, x, _ = load(gold, "sdta")
    for i, block in enumerate(model.channel_align.model):
        y = block(torch.from_numpy(gold["input"] if i == 0 else gold[f"sdta/hook/{i - 1}"]).cuda())
        err = rel(y, gold[f"sdta/hook/{i}"])
        print(f"sdta block {i} ({type(block).__name__}): {err:.3e}")
        assert err <= RTOL


def test_sdta_graph_replay_equals_eager(gold, monkeypatch):
    monkeypatch.delenv("HEAL_ALIGN_FUSED", raising=False)
    model, x, _ = load(gold, "sdta")
    gen = torch.Generator().manual_seed(5)
    inputs = [torch.randn(x.shape, generator=gen).cuda() for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static_x = x.clone()
        for _ in range(2):
            model(static_x)              # weight-derived tensors and workspaces exist before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_y = model(static_x)
        for xi in inputs:
            static_x.copy_(xi)
            graph.replay()
            side.synchronize()
            assert torch.equal(static_y, model(xi))
    torch.cuda.synchronize()


@pytest.mark.grad
@pytest.mark.parametrize("name", NAMES)
def test_gradient_path_on_the_device(name, gold, monkeypatch):
    monkeypatch.delenv("HEAL_ALIGN_FUSED", raising=False)
    model, x, want = load(gold, name)
    calls = ops.XCA_CALLS["weights"]
    y = model(x.clone().requires_grad_(True))       # eval mode, parameters require gradient: the gradient path
    assert y.grad_fn is not None and rel(y, want) <= RTOL
    y.square().mean().backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert ops.XCA_CALLS["weights"] == calls        # the fused path stayed untaken
