"""CoBEVT's swap fusion (reference: opencood/models/fuse_modules/swap_fusion_modules.py:11-152 Attention / SwapFusionBlockMask,
sub_modules/base_transformer.py:17-39 PreNormResidual / FeedForward, fusion_in_one.py:374-430 CoBEVT).

Module / parameter layout mirrors the reference so that checkpoints load (the persistent `relative_position_index` buffer
included).  CoBEVT itself (Regroup, warp, blocks, mlp_head) is in fusion_in_one.py.  Three execution paths:
  * the reference's torch arithmetic on x [B, L, C, H, W] with einops' rearranges restated as view / permute -- on the CPU and
    whenever autograd records (the default gradient path: the library's composition, no HIP kernel);
  * opt-in (Attention.grad_kernel, CoBEVT's `grad_kernel` argument), when autograd records on the device: the block token-major
    [B, L, H, W, C] with the torch LayerNorm / Linear / FeedForward modules around ops.AgentWindowAttention (the forward kernel +
    heal_agent_window_attention_backward per scene; no [groups, heads, T, T] tensor is kept for the backward);
  * inference on the device: one scene token-major [L, H, W, C] through all blocks.  Each attention half-block is heal_ln_stats ->
    heal_linear (LayerNorm folded, 256 -> 768) -> heal_agent_window_attention (window or grid grouping, per-head 3-D relative
    position bias, keys of padded agents skipped) -> heal_linear (to_out + x); each feed-forward is two heal_linear launches
    (v2xvit_basic.FeedForward.fused_residual); mlp_head is heal_agent_mean -> heal_ln_stats -> heal_linear.
"""

import torch
import torch.nn as nn

from heal_amd import ops, switches
from heal_amd.derived import derived
from heal_amd.opencood.models.sub_modules.v2xvit_basic import FeedForward, _fold_ln


def _grad_path(x, module):
    return torch.is_grad_enabled() and (x.requires_grad or module.training)


def fused_ok(x, module, L, H, W, C):
    """Inference on the device of x with a scene of L agents, H x W maps and C channels, shapes the HIP kernels take.
    HEAL_COBEVT_FUSED=0 keeps the torch composition on the device (A/B)."""
    if not x.is_cuda or x.dtype != torch.float32 or _grad_path(x, module) or not switches.on("HEAL_COBEVT_FUSED"):
        return False
    return all(ops.agent_window_attention_supported(L, b.window_size, b.window_attention.fn.dim_head, H, W)
               and b.window_attention.fn.heads * b.window_attention.fn.dim_head == C for b in module.layers) \
        and C % 4 == 0 and ops.linear_supported(L * H * W, C, 3 * C) and ops.linear_supported(L * H * W, C, C)


class PreNormResidual(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward(self, x, **kwargs):
        return self.fn(self.norm(x), **kwargs) + x


def _relative_position_index(agent_size, window_size):
    """swap_fusion_modules.py:58-83: [T, T] index into the (2L-1)(2ws-1)^2 table for tokens in (l w1 w2) order."""
    ws = [agent_size, window_size, window_size]
    coords = torch.stack(torch.meshgrid(torch.arange(ws[0]), torch.arange(ws[1]), torch.arange(ws[2]), indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws[0] - 1
    rel[:, :, 1] += ws[1] - 1
    rel[:, :, 2] += ws[2] - 1
    rel[:, :, 0] *= (2 * ws[1] - 1) * (2 * ws[2] - 1)
    rel[:, :, 1] *= 2 * ws[2] - 1
    return rel.sum(-1)


class Attention(nn.Module):
    grad_kernel = False     # True: under autograd on the device the attention core is ops.AgentWindowAttention (SwapFusionBlockMask)

    def __init__(self, dim, dim_head=32, dropout=0.0, agent_size=6, window_size=7):
        super().__init__()
        assert dim % dim_head == 0, "dimension should be divisible by dimension per head"
        self.heads = dim // dim_head
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.window_size = [agent_size, window_size, window_size]
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(dim, dim, bias=False), nn.Dropout(dropout))
        self.relative_position_bias_table = nn.Embedding(
            (2 * agent_size - 1) * (2 * window_size - 1) * (2 * window_size - 1), self.heads)
        self.register_buffer("relative_position_index", _relative_position_index(agent_size, window_size))

    def forward(self, x, key_mask=None):
        """x [b, l, X, Y, w1, w2, c], key_mask [b, l] (nonzero = real agent) -> same shape (swap_fusion_modules.py:86-131)."""
        b, L, X, Y, w1, w2, c = x.shape
        h, d = self.heads, self.dim_head
        x = x.permute(0, 2, 3, 1, 4, 5, 6).reshape(b * X * Y, L * w1 * w2, c)
        q, k, v = self.to_qkv(x).chunk(3, dim=-1)
        q, k, v = (t.reshape(b * X * Y, L * w1 * w2, h, d).permute(0, 2, 1, 3) for t in (q, k, v))
        q = q * self.scale
        sim = torch.einsum("bhid,bhjd->bhij", q, k)
        sim = sim + self.relative_position_bias_table(self.relative_position_index).permute(2, 0, 1)
        if key_mask is not None:
            m = key_mask[:, None, None, :, None].expand(b, X, Y, L, w1 * w2).reshape(b * X * Y, 1, 1, L * w1 * w2)
            sim = sim.masked_fill(m == 0, -float("inf"))
        attn = sim.softmax(dim=-1)
        out = torch.einsum("bhij,bhjd->bhid", attn, v)
        out = out.permute(0, 2, 1, 3).reshape(b * X * Y, L, w1, w2, h * d)
        out = self.to_out(out)
        return out.reshape(b, X, Y, L, w1, w2, c).permute(0, 3, 1, 2, 4, 5, 6)

    def position_bias(self):
        """[heads, T, T] f32: the table looked up once per weight version (inference; a captured graph keeps its address while
        the table is unchanged)."""
        tab = self.relative_position_bias_table.weight
        return derived("agent_window_position_bias", (tab, self.relative_position_index),
                       lambda: tab.detach()[self.relative_position_index].permute(2, 0, 1).contiguous().float())

    def grad_kernel_ok(self, x):
        """The opt-in device gradient path takes x [b, L, C, H, W]: grad_kernel set, autograd recording, CUDA fp32 and a shape
        heal_agent_window_attention_backward takes."""
        if not (self.grad_kernel and x.is_cuda and x.dtype == torch.float32 and _grad_path(x, self) and x.dim() == 5):
            return False
        b, L, C, H, W = x.shape
        return C == self.heads * self.dim_head and ops.agent_window_attention_train_supported(L, self.window_size[1], self.dim_head,
                                                                                              H, W)

    def kernel_residual(self, x, norm, n_valid, mode):
        """x token-major [b, L, H, W, C] -> to_out(attention(to_qkv(norm(x)))) + x under autograd: the torch modules around
        ops.AgentWindowAttention per scene.  The bias is looked up from the table through autograd: its gradient reaches the table."""
        qkv = self.to_qkv(norm(x))
        bias = self.relative_position_bias_table(self.relative_position_index).permute(2, 0, 1).contiguous()
        att = torch.stack([ops.AgentWindowAttention.apply(qkv[i], bias, n_valid[i], mode, self.heads, self.dim_head,
                                                          self.window_size[1], self.scale) for i in range(x.shape[0])])
        return self.to_out(att) + x

    def fused_residual(self, x, norm, n_valid, mode):
        """x token-major [L, H, W, C] -> x + to_out(attention(norm(x))): LayerNorm folded into the 256 -> 768 heal_linear, the
        agent-window kernel writing [L, H, W, C], to_out + x in the epilogue of the second heal_linear."""
        L, H, W, C = x.shape
        w, b = self._f_qkv(norm)
        qkv = ops.linear(x, w, b, stats=ops.ln_stats(x, norm.eps)).view(L, H, W, 3 * C)
        att = ops.agent_window_attention(qkv, self.position_bias(), n_valid, mode, self.heads, self.dim_head,
                                         self.window_size[1], self.scale)
        return ops.linear(att, self.to_out[0].weight, None, residual=x.reshape(-1, C)).view(L, H, W, C)

    def _f_qkv(self, norm):
        return derived("fold_ln", (self.to_qkv.weight, None, norm.weight, norm.bias), lambda: _fold_ln(self.to_qkv.weight, None, norm))


def _prefix_counts(key_mask, b, m):
    """key_mask [b, m] (nonzero = real agent) -> the number of real agents of every scene, or None when a mask is not a non-empty
    prefix of the agents (the kernels mask the trailing agents; Regroup pads at the end).  Reads the mask on the host."""
    if key_mask is None:
        return [m] * b
    rows = (key_mask != 0).tolist()
    counts = [sum(r) for r in rows]
    if any(n < 1 or r != [True] * n + [False] * (m - n) for r, n in zip(rows, counts)):
        return None
    return counts


class SwapFusionBlockMask(nn.Module):
    def __init__(self, input_dim, mlp_dim, dim_head, window_size, agent_size, drop_out):
        super().__init__()
        self.window_size = window_size
        self.window_attention = PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, agent_size, window_size))
        self.window_ffd = PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out))
        self.grid_attention = PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, agent_size, window_size))
        self.grid_ffd = PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out))

    def forward(self, x, key_mask):
        """x [b, m, d, H, W], key_mask [b, m] -> [b, m, d, H, W] (swap_fusion_modules.py:135-152)."""
        b, m, d, H, W = x.shape
        if self.window_attention.fn.grad_kernel_ok(x) and self.grid_attention.fn.grad_kernel_ok(x):
            n_valid = _prefix_counts(key_mask, b, m)
            if n_valid is not None:
                return self.grad_kernel_forward(x, n_valid)
        ws = self.window_size
        X, Y = H // ws, W // ws
        # 'b m d (x w1) (y w2) -> b m x y w1 w2 d'
        x = x.reshape(b, m, d, X, ws, Y, ws).permute(0, 1, 3, 5, 4, 6, 2)
        x = self.window_attention(x, key_mask=key_mask)
        x = self.window_ffd(x)
        x = x.permute(0, 1, 6, 2, 4, 3, 5).reshape(b, m, d, H, W)
        # 'b m d (w1 x) (w2 y) -> b m x y w1 w2 d'
        x = x.reshape(b, m, d, ws, X, ws, Y).permute(0, 1, 4, 6, 3, 5, 2)
        x = self.grid_attention(x, key_mask=key_mask)
        x = self.grid_ffd(x)
        return x.permute(0, 1, 6, 4, 2, 5, 3).reshape(b, m, d, H, W)

    def grad_kernel_forward(self, x, n_valid):
        """The same block under autograd with the attention kernels: token-major [b, m, H, W, d] through both half-blocks and
        both feed-forwards, permuted back so that the caller sees [b, m, d, H, W]."""
        x = x.permute(0, 1, 3, 4, 2).contiguous()
        x = self.window_attention.fn.kernel_residual(x, self.window_attention.norm, n_valid, "window")
        x = self.window_ffd(x)
        x = self.grid_attention.fn.kernel_residual(x, self.grid_attention.norm, n_valid, "grid")
        x = self.grid_ffd(x)
        return x.permute(0, 1, 4, 2, 3)

    def fused(self, x, n_valid):
        """The same block on one scene token-major [L, H, W, C] (inference on the device)."""
        x = self.window_attention.fn.fused_residual(x, self.window_attention.norm, n_valid, "window")
        x = self.window_ffd.fn.fused_residual(x, self.window_ffd.norm)
        x = self.grid_attention.fn.fused_residual(x, self.grid_attention.norm, n_valid, "grid")
        return self.grid_ffd.fn.fused_residual(x, self.grid_ffd.norm)


class _NoParams(nn.Module):
    """Placeholder for the einops Reduce / Rearrange layers of the reference's mlp_head (keeps the Sequential indices)."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what
