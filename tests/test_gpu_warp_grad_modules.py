"""The fusion modules' gradient path with ops.warp_grad("kernel") against the default ("torch") and a float64 copy of the module.

One scene of 3 agents, C = 64, 32 x 48, rigid rows.  Per module the gradients with respect to the input(s) and every parameter are
computed three times with the same weights: kernel mode, torch mode, and the module in float64 (the yardstick).  The kernel mode's
error against float64 may be at most twice the torch mode's plus 1e-6 max|reference| (the margin allows for reordered fp32 sums).
Kernel-mode runs must go through ops.WarpAffine (forward and backward), default-mode runs must not; a scene whose padded agent has a
singular row falls back to affine_grid + grid_sample and still matches."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from heal_amd import ops
from heal_amd.opencood.models.fuse_modules import fusion_in_one as fio
from heal_amd.pipeline import fill_deterministic
from tests import warp_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = torch.device("cuda:0")
N, C, H, W = 3, 64, 32, 48
COBEVT_ARGS = {"input_dim": C, "mlp_dim": 64, "agent_size": 3, "window_size": 4, "dim_head": 32, "drop_out": 0.0, "depth": 2}


def _affine(n_real=N, singular_pad=False):
    """[1, 3, 3, 2, 3] float64: row [0, 0, j] warps agent j into the ego frame (the ego's own row is the identity)."""
    rows = np.concatenate([R.rigid(0, 0, 0, H, W)[None], R.random_rigid(2, H, W, 17, 0.1)])
    aff = np.tile(R.rigid(0, 0, 0, H, W).reshape(1, 1, 1, 2, 3), (1, 3, 3, 1, 1))
    aff[0, 0] = rows.reshape(3, 2, 3)
    if singular_pad:
        aff[0, :, n_real:] = 0.0
        aff[0, n_real:] = 0.0
    return aff


def _inputs(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float32) for s in shapes]


class _Levels(nn.Module):
    """fuse_levels with AttFusion at two levels, as HeterModelBaselineMs calls it."""

    def __init__(self):
        super().__init__()
        self.net = nn.ModuleList([fio.AttFusion(C), fio.AttFusion(2 * C)])

    def forward(self, x0, x1, record_len, aff):
        return fio.fuse_levels(self.net, [x0, x1], record_len, aff)


def _make(kind):
    """The module with the project's deterministic weights (non-trivial BatchNorm statistics: no dead ReLU in eval mode)."""
    makers = {"max": fio.MaxFusion, "att": lambda: fio.AttFusion(C), "disco": lambda: fio.DiscoFusion(C),
              "cobevt": lambda: fio.CoBEVT(dict(COBEVT_ARGS)), "cobevt_padded": lambda: fio.CoBEVT(dict(COBEVT_ARGS)),
              "who2com": lambda: fio.Who2comFusion(C), "levels": _Levels}
    return fill_deterministic(makers[kind](), 3)


def _run(model, xs, aff, n_real, mode, dtype):
    """Gradients of sum(out * G) with respect to the inputs and every parameter -> (list of CPU float64 tensors, call deltas).
    The modules are in eval mode (the input requires gradient, so they are on their gradient path all the same): with batch
    statistics the true gradient of a convolution bias in front of a BatchNorm is identically zero, and holding one run's
    rounding noise to twice another's says nothing about the warp.  With fill_deterministic's weights every parameter that takes
    part has a non-zero gradient, which the test asserts."""
    model = copy.deepcopy(model).to(DEV).to(dtype).eval()
    xs = [x.to(DEV).to(dtype).requires_grad_(True) for x in xs]
    before = dict(ops.WARP_GRAD_CALLS)
    with ops.warp_grad(mode):
        out = model(*xs, torch.tensor([n_real]), aff)
        outs = out if isinstance(out, (list, tuple)) else [out]
        g = torch.Generator().manual_seed(99)
        loss = sum((o * torch.randn(*o.shape, generator=g, dtype=torch.float32).to(DEV).to(dtype)).sum() for o in outs)
        loss.backward()
    torch.cuda.synchronize()
    grads = [x.grad for x in xs] + [p.grad for _, p in sorted(model.named_parameters())]
    names = [f"input{i}" for i in range(len(xs))] + [k for k, _ in sorted(model.named_parameters())]
    delta = {k: ops.WARP_GRAD_CALLS[k] - before[k] for k in before}
    return {k: v.detach().double().cpu() for k, v in zip(names, grads) if v is not None}, delta


@pytest.mark.parametrize("kind", ["max", "att", "disco", "cobevt", "who2com", "levels", "cobevt_padded"])
def test_kernel_mode_matches_torch_mode_against_float64(kind):
    padded = kind == "cobevt_padded"
    n_real = 2 if padded else N
    aff = _affine(n_real, singular_pad=padded)
    shapes = [(n_real, C, H, W)] + ([(n_real, 2 * C, H // 2, W // 2)] if kind == "levels" else [])
    xs = _inputs(shapes, 31)
    model = _make(kind)
    ref, d_ref = _run(model, xs, aff, n_real, "torch", torch.float64)
    tor, d_tor = _run(model, xs, aff, n_real, "torch", torch.float32)
    ker, d_ker = _run(model, xs, aff, n_real, "kernel", torch.float32)
    assert d_tor["forward"] == 0 and d_tor["backward"] == 0 and d_tor["torch"] > 0
    assert d_ref["forward"] == 0 and d_ref["backward"] == 0
    if padded:       # the padded agent's all-zero row is singular: the whole warp stays on affine_grid + grid_sample
        assert d_ker == d_tor
    else:
        assert d_ker["forward"] > 0 and d_ker["backward"] == d_ker["forward"] and d_ker["torch"] == 0
    assert set(ref) == set(tor) == set(ker) and "input0" in ref
    worst = 0.0
    for k, want in ref.items():
        e_ker, e_tor = float((ker[k] - want).abs().max()), float((tor[k] - want).abs().max())
        top = float(want.abs().max())
        print(f"{kind} {k}: kernel {e_ker:.3e} torch {e_tor:.3e} max|ref| {top:.3e}")
        assert top > 0, k                  # every compared gradient is a real one
        assert e_ker <= 2.0 * e_tor + 1e-6 * top, (k, e_ker, e_tor, top)
        worst = max(worst, top)
    assert worst > 0 and float(ref["input0"].abs().max()) > 0
