"""Host side of the agent-window attention backward (include/heal_amd_train_attn.h, ops.AgentWindowAttention, Attention.grad_kernel):
the fourth header and its ctypes signatures, the exported symbols, the shape / parts / workspace arithmetic, and the CPU behaviour
of the opt-in module path.  Needs the built library, no GPU."""
import ctypes

import pytest
import torch

from heal_amd import _capi

I, P, Z, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
EXPECTED = {
    "heal_agent_window_attention_backward_supported": (I, [I] * 5),            # n_agents, window, dim_head, H, W
    "heal_agent_window_attention_backward_parts": (I, [I] * 4),                # n_agents, H, W, heads
    "heal_agent_window_attention_backward_workspace": (Z, [I] * 5),            # n_agents, H, W, heads, parts
    # qkv, bias, grad_out | n_agents, n_valid, H, W, heads, dim_head, window, mode | scale | parts | grad_qkv, grad_bias, ws |
    # ws_bytes | stream
    "heal_agent_window_attention_backward": (I, [P] * 3 + [I] * 8 + [F, I] + [P] * 3 + [Z, P]),
}


def test_train_attn_header_declares_the_four_entry_points():
    sig = _capi.signatures_train_attn()
    assert set(sig) == set(EXPECTED)
    for name, (res, args) in EXPECTED.items():
        assert sig[name][0] is res, name
        assert list(sig[name][1]) == args, name


def test_it_is_disjoint_from_the_other_tables_and_part_of_every_build():
    from heal_amd import build
    mine = set(_capi.signatures_train_attn())
    assert not mine & set(_capi.signatures())
    assert not mine & set(_capi.signatures_train())
    assert not mine & set(_capi.signatures_ext())
    assert _capi.HEADER_TRAIN_ATTN in build._deps()               # an edit of the header rebuilds the objects


def test_library_exports_and_binds_them():
    L = _capi.lib()
    for name, (res, args) in EXPECTED.items():
        assert hasattr(L, name), name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name


MAX_AGENTS = _capi.header_define("HEAL_AGENT_WINDOW_MAX_AGENTS")


@pytest.mark.parametrize("n_agents,window,dim_head,H,W,ok", [
    (1, 4, 32, 4, 4, 1), (5, 4, 32, 128, 128, 1), (8, 4, 32, 8, 12, 1), (3, 4, 32, 100, 252, 1),
    (5, 5, 32, 20, 20, 0),              # window 5
    (5, 4, 64, 16, 16, 0),              # dim_head 64
    (5, 4, 32, 18, 16, 0), (5, 4, 32, 16, 6, 0),     # H, W not multiples of 4
    (9, 4, 32, 16, 16, 0), (0, 4, 32, 16, 16, 0),    # agents outside 1..8
    (5, 4, 32, 0, 16, 0),
])
def test_supported_takes_the_forward_shapes(n_agents, window, dim_head, H, W, ok):
    from heal_amd import ops
    assert MAX_AGENTS == 8
    assert _capi.lib().heal_agent_window_attention_backward_supported(n_agents, window, dim_head, H, W) == ok
    if H > 0 and W > 0:
        assert bool(ops.agent_window_attention_supported(n_agents, window, dim_head, H, W)) == bool(ok)
        assert ops.agent_window_attention_train_supported(n_agents, window, dim_head, H, W) == bool(ok)


@pytest.mark.parametrize("heads", [1, 2, 8, 16, 2048])
def test_parts_and_workspace_are_the_arithmetic_the_header_states(heads):
    """parts = min(G, max(1, 1024 / heads)) with G = (H / 4)(W / 4): a pure function of the shape, never more parts than groups (no
    empty part); workspace = parts * heads * T * T * 4 bytes for more than one part, nothing for one; parts = 0 asks for the
    policy's value."""
    L = _capi.lib()
    for n_agents, H, W in [(1, 4, 4), (2, 8, 12), (3, 16, 16), (5, 32, 32), (5, 128, 128), (8, 100, 252)]:
        G, T = (H // 4) * (W // 4), 16 * n_agents
        parts = L.heal_agent_window_attention_backward_parts(n_agents, H, W, heads)
        assert parts == min(G, max(1, 1024 // heads)), (n_agents, H, W)
        assert 1 <= parts <= G
        assert L.heal_agent_window_attention_backward_parts(n_agents, H, W, heads) == parts
        for p in {1, 2, parts, G}:
            if p > G:
                continue
            want = p * heads * T * T * 4 if p > 1 else 0
            assert _capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, p) == want, (n_agents, H, W, p)
        assert (_capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, 0)
                == _capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, parts))
        # more parts than groups, or a negative count: no such launch, no workspace
        assert _capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, G + 1) == 0
        assert _capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, -1) == 0


def test_queries_refuse_unsupported_shapes():
    L = _capi.lib()
    for n_agents, H, W, heads in [(9, 16, 16, 8), (5, 18, 16, 8), (5, 16, 6, 8), (0, 16, 16, 8), (5, 16, 16, 0)]:
        assert L.heal_agent_window_attention_backward_parts(n_agents, H, W, heads) == 0
        assert _capi.query("heal_agent_window_attention_backward_workspace", n_agents, H, W, heads, 0) == 0


def test_backward_refuses_cpu_tensors():
    from heal_amd import ops
    qkv, out = torch.zeros(2, 8, 8, 192), torch.zeros(2, 8, 8, 64)
    with pytest.raises(_capi.HealAmdError):
        ops.agent_window_attention_backward(qkv, None, out, 1, "window", 2, 32, 4, 1.0)


@pytest.mark.grad
def test_grad_kernel_is_inert_on_the_cpu(monkeypatch):
    """A CoBEVT built with grad_kernel: true gives, on the CPU, output and gradients bit-equal to one built without it: CPU tensors
    never reach ops.AgentWindowAttention and the reference composition runs unchanged."""
    from heal_amd import ops
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import CoBEVT
    from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import Attention
    assert Attention.grad_kernel is False

    def never(*a, **k):
        raise AssertionError("the kernel path was taken on the CPU")
    monkeypatch.setattr(ops, "agent_window_attention", never)               # AgentWindowAttention.forward goes through it
    args = {"input_dim": 64, "mlp_dim": 64, "agent_size": 3, "window_size": 4, "dim_head": 32, "drop_out": 0.0, "depth": 2}
    x = torch.randn((4, 64, 8, 12), generator=torch.Generator().manual_seed(3))
    aff = torch.eye(2, 3)[None, None, None].repeat(2, 3, 3, 1, 1)
    res = {}
    for flag in (True, False):
        torch.manual_seed(17)
        model = CoBEVT(dict(args, grad_kernel=flag) if flag else dict(args)).train()
        assert model.grad_kernel is flag
        assert all(b.window_attention.fn.grad_kernel is flag and b.grid_attention.fn.grad_kernel is flag for b in model.layers)
        xi = x.clone().requires_grad_(True)
        out = model(xi, torch.tensor([3, 1]), aff)
        out.square().mean().backward()
        res[flag] = [out.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in model.parameters()]
    assert len(res[True]) == len(res[False])
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
