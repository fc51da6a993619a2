"""Single-scale fusion operators used by HeterModelBaseline (reference: opencood/models/fuse_modules/
fusion_in_one.py): MaxFusion (:87-124), AttFusion (:126-151, :14-45), DiscoFusion (:153-201), V2VNetFusion (:203-318),
V2XViTFusion (:320-372), CoBEVT (:374-430), Where2commFusion (:431-484), Who2comFusion (:486-539).  Warping to the ego frame is
heal_warp_affine_forward (K5's sampling code, every agent of a scene in one launch; on the gradient path, in
ops.warp_grad("kernel") mode, ops.WarpAffine with the gather-form heal_warp_affine_backward instead of affine_grid + grid_sample);
the per-pixel attention is K6; CoBEVT's agent-window attention is heal_agent_window_attention
(swap_fusion_modules.py; with `grad_kernel` its backward is heal_agent_window_attention_backward); V2VNet's masked message
aggregation is heal_v2v_message; DiscoNet's warp + pixel-weight MLP + softmax is heal_disco_fuse; Where2comm's warp + multi-head attention over agents is heal_warp_mha_fuse."""

import numpy as np
import torch
import torch.nn as nn

from heal_amd import ops, switches
from heal_amd.opencood.models._heter_common import record_len_to_list


def regroup(x, record_len):
    """fusion_in_one.py:48-51: split the agent dimension by scene."""
    lens = record_len_to_list(record_len)
    return torch.split(x, lens)


def warp_to_ego(x, affine_rows, grid_f64=True):
    """warp_affine_simple(x, t_matrix[0, :], (H, W)) for one scene: x [n,C,H,W] -> [n,C,H,W]."""
    if isinstance(affine_rows, (list, tuple)) and len(affine_rows) and isinstance(affine_rows[0], torch.Tensor):
        affine_rows = torch.stack(list(affine_rows))      # per-agent rows (the agent-sharded runner): one [n, 2, 3] tensor
    if torch.is_grad_enabled() and x.requires_grad:   # gradient path
        if ops.warp_grad_enabled() and ops.warp_affine_train_supported(x, affine_rows):
            return ops.WarpAffine.apply(x, affine_rows, grid_f64)     # ops.warp_grad("kernel"): forward + gather-form backward kernels
        # affine_grid + grid_sample (torch_transformation_utils.py:323-332)
        import torch.nn.functional as F
        ops.WARP_GRAD_CALLS["torch"] += 1
        M = torch.as_tensor(affine_rows, dtype=x.dtype, device=x.device)
        return F.grid_sample(x, F.affine_grid(M, list(x.shape), align_corners=False), align_corners=False)
    return ops.warp_affine(x, affine_rows, grid_f64)     # every agent of the scene in one launch (bit-equal to warp_agent per agent)


def _host_affine(affine_matrix):
    """-> (affine matrix, grid_is_f64).  CUDA tensors stay on the device (read by the warp kernel at run time)."""
    if isinstance(affine_matrix, torch.Tensor):
        if affine_matrix.is_cuda:
            return affine_matrix.detach(), affine_matrix.dtype == torch.float64
        a = affine_matrix.detach().numpy()
    else:
        a = np.asarray(affine_matrix)
    return a, a.dtype == np.float64


def _torch_affine(affine_matrix, like):
    """The affine matrix as a tensor on `like`'s device, in its own dtype (the torch compositions follow it as the reference does)."""
    aff = affine_matrix if isinstance(affine_matrix, torch.Tensor) else torch.from_numpy(np.asarray(affine_matrix))
    return aff.to(like.device)


class _WarpThenFuse(nn.Module):
    """The operators share one shape: warp every agent of a scene into the ego frame (K5), then reduce the
    ego-frame stack with `fuse_warped` ([n,C,H,W] -> [C,H,W]).  The agent-sharded path (heal_amd/dist.py) warps on the
    owning rank and calls `fuse_warped` on the gathered stack."""

    def forward(self, x, record_len, affine_matrix):
        aff, f64 = _host_affine(affine_matrix)
        out = []
        for b, feats in enumerate(regroup(x, record_len)):
            n = feats.shape[0]
            out.append(self.fuse_warped(warp_to_ego(feats, aff[b][0, :n], f64)))
        return torch.stack(out)


class MaxFusion(_WarpThenFuse):
    def fuse_warped(self, ego):
        return ego.max(dim=0)[0]


class AttFusion(_WarpThenFuse):
    def __init__(self, feature_dims):
        super().__init__()
        self.sqrt_dim = float(np.sqrt(feature_dims))
        self.feature_dims = feature_dims

    def fuse_warped(self, ego):
        n, C, H, W = ego.shape
        x = ego.reshape(n, C, H * W).permute(2, 0, 1).contiguous()      # [HW, n, C]
        if torch.is_grad_enabled() and ego.requires_grad:
            # gradient path (fusion_in_one.py:14-45,126-151): softmax(x x^T / sqrt(C)) x per pixel, the ego row
            if (n <= ops.AGENT_ATTENTION_MAX_AGENTS and ops.agent_attention_train_supported(x, 1)
                    and switches.get("HEAL_ATTN_GRAD") != "torch"):
                # K6 forward (ego row) + heal_agent_attention_backward; x enters as q, k and v: autograd sums the three gradients
                return ops.AgentAttention.apply(x, x, x, 1, 1.0 / self.sqrt_dim, 1, False)[:, 0, :].t().reshape(C, H, W)
            attn = torch.softmax(torch.bmm(x, x.transpose(1, 2)) / self.sqrt_dim, dim=-1)
            return torch.bmm(attn, x)[:, 0, :].t().reshape(C, H, W)
        h = ops.agent_attention(x, x, x, heads=1, scale=1.0 / self.sqrt_dim, out_rows=1)  # ego row only
        return h[:, 0, :].t().reshape(C, H, W)


class V2XViTFusion(_WarpThenFuse):
    def __init__(self, args):
        super().__init__()
        from heal_amd.opencood.models.sub_modules.v2xvit_basic import V2XTransformer
        self.fusion_net = V2XTransformer(args["transformer"])

    def fuse_warped(self, ego):
        fused = self.fusion_net(ego.permute(0, 2, 3, 1).contiguous())       # [n,H,W,C] -> [H,W,C]; the 3 prior channels are zero
        return fused.permute(2, 0, 1)

    def forward(self, x, record_len, affine_matrix):
        if not x.is_cuda or x.shape[1] % 4 or (torch.is_grad_enabled() and x.requires_grad):
            return super().forward(x, record_len, affine_matrix)
        # inference on the device: every agent of a scene warped straight into the transformer's token-major layout (one launch;
        # no per-agent warp + stack + permute copy)
        aff, f64 = _host_affine(affine_matrix)
        out = []
        for b, feats in enumerate(regroup(x, record_len)):
            n = feats.shape[0]
            out.append(self.fusion_net(ops.warp_agents_pm(feats, aff[b][0, :n], f64)).permute(2, 0, 1))
        return torch.stack(out)


class CoBEVT(_WarpThenFuse):
    """fusion_in_one.py:374-430.  Regroup pads every scene to L = agent_size agents with zero maps and masks their keys; the
    warp of a zero map is zero, so the real agents are warped and `fuse_warped` pads.  The mlp_head's mean runs over all L agents,
    padded ones included (their rows are not zero after the first block: they attend to the real agents' keys) -- as the
    reference computes it."""

    def __init__(self, args):
        super().__init__()
        from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import SwapFusionBlockMask, _NoParams
        self.depth = args["depth"]
        self.agent_size = args["agent_size"]
        self.window_size = args["window_size"]
        input_dim = args["input_dim"]
        self.layers = nn.ModuleList([SwapFusionBlockMask(input_dim, args["mlp_dim"], args["dim_head"], args["window_size"],
                                                         args["agent_size"], args["drop_out"]) for _ in range(self.depth)])
        # opt-in: under autograd on the device the blocks run ops.AgentWindowAttention (forward + backward kernels) instead of the
        # library's composition
        self.grad_kernel = bool(args.get("grad_kernel", False))
        for stage in self.layers:
            stage.window_attention.fn.grad_kernel = stage.grid_attention.fn.grad_kernel = self.grad_kernel
        self.mlp_head = nn.Sequential(_NoParams("Reduce('b m d h w -> b d h w', 'mean')"),
                                      _NoParams("Rearrange('b d h w -> b h w d')"),
                                      nn.LayerNorm(input_dim), nn.Linear(input_dim, input_dim),
                                      _NoParams("Rearrange('b h w d -> b d h w')"))

    def _check(self, n):
        if n > self.agent_size:
            raise ValueError(f"CoBEVT: a scene has {n} agents, more than agent_size = {self.agent_size} (max_cav) the fusion "
                             "was built for")

    def fuse_warped(self, ego):
        """ego [n, C, H, W] (ego-frame maps of one scene's real agents) -> [C, H, W]."""
        n = ego.shape[0]
        self._check(n)
        from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import fused_ok
        if fused_ok(ego, self, self.agent_size, ego.shape[2], ego.shape[3], ego.shape[1]):
            return self.fuse_warped_pm(ego.permute(0, 2, 3, 1)).permute(2, 0, 1)
        x = ego.new_zeros((1, self.agent_size) + tuple(ego.shape[1:]))
        x[0, :n] = ego
        key_mask = (torch.arange(self.agent_size, device=ego.device) < n).to(torch.int64)[None]
        return self.transformer(x, key_mask)[0]

    def transformer(self, x, key_mask):
        """x [B, L, C, H, W] (padded agents zero), key_mask [B, L] -> [B, C, H, W]: the reference's torch arithmetic (the CPU and
        gradient path)."""
        for stage in self.layers:
            x = stage(x, key_mask)
        x = x.mean(dim=1).permute(0, 2, 3, 1)
        return self.mlp_head[3](self.mlp_head[2](x)).permute(0, 3, 1, 2)

    def fuse_warped_pm(self, x):
        """x token-major [n, H, W, C] (one scene's real agents) -> [H, W, C] on the HIP path: padded to L once, token-major through
        every block, agent mean + LayerNorm + Linear at the end."""
        from heal_amd.derived import derived
        from heal_amd.opencood.models.sub_modules.v2xvit_basic import _fold_ln
        n, H, W, C = x.shape
        self._check(n)
        if n < self.agent_size:
            xp = torch.zeros((self.agent_size, H, W, C), dtype=x.dtype, device=x.device)
            xp[:n].copy_(x)
            x = xp
        else:
            x = x.contiguous()
        for stage in self.layers:
            x = stage.fused(x, n)
        mean = ops.agent_mean(x)                          # [H, W, C]: every agent, padded ones included
        norm, lin = self.mlp_head[2], self.mlp_head[3]
        w, b = derived("fold_ln", (lin.weight, lin.bias, norm.weight, norm.bias), lambda: _fold_ln(lin.weight, lin.bias, norm))
        return ops.linear(mean, w, b, stats=ops.ln_stats(mean, norm.eps)).view(H, W, C)

    def forward(self, x, record_len, affine_matrix):
        from heal_amd.opencood.models.fuse_modules.swap_fusion_modules import fused_ok
        lens = record_len_to_list(record_len)
        self._check(max(lens))
        C, H, W = x.shape[1:]
        L = self.agent_size
        if not fused_ok(x, self, L, H, W, C):
            # the reference's arithmetic (fusion_in_one.py:412-430): Regroup's zero padding, warp_affine_simple of all L maps
            # (the grid built in the affine matrix's dtype, then cast; ops.WarpAffine in ops.warp_grad("kernel") mode unless a
            # padded agent's row is singular), the blocks on [B, L, C, H, W]
            aff = _torch_affine(affine_matrix, x)
            warped = []
            for b, feats in enumerate(regroup(x, lens)):
                pad = torch.cat([feats, feats.new_zeros((L - feats.shape[0],) + tuple(feats.shape[1:]))])
                warped.append(_warp_affine_simple(pad, aff[b, 0, :L], (H, W)))
            key_mask = (torch.arange(L, device=x.device)[None, :] < torch.tensor(lens, device=x.device)[:, None]).to(torch.int64)
            return self.transformer(torch.stack(warped), key_mask)
        # inference on the device: the real agents warped straight into the token-major layout (one launch per scene)
        aff, f64 = _host_affine(affine_matrix)
        out = []
        for b, feats in enumerate(regroup(x, lens)):
            n = feats.shape[0]
            out.append(self.fuse_warped_pm(ops.warp_agents_pm(feats, aff[b][0, :n], f64)).permute(2, 0, 1))
        return torch.stack(out)


def _warp_affine_simple(src, M, dsize):
    """torch_transformation_utils.py:323-332: affine_grid (in M's dtype, then cast) + bilinear grid_sample, zero padding."""
    import torch.nn.functional as F
    if (ops.warp_grad_enabled() and torch.is_grad_enabled() and src.requires_grad and tuple(dsize) == tuple(src.shape[2:])
            and M.dtype in (torch.float32, torch.float64) and ops.warp_affine_train_supported(src, M)):
        return ops.WarpAffine.apply(src, M, M.dtype == torch.float64)      # ops.warp_grad("kernel")
    if torch.is_grad_enabled() and src.requires_grad:
        ops.WARP_GRAD_CALLS["torch"] += 1
    grid = F.affine_grid(M, [src.shape[0], src.shape[1], dsize[0], dsize[1]], align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


class DiscoFusion(nn.Module):
    """fusion_in_one.py:153-201 (with fuse_modules/disco_fuse.py).  Per scene: every agent warped into the ego frame, one logit per
    (agent, pixel) from PixelWeightLayer(cat(warped neighbour, unwarped ego)), softmax over agents, weighted sum of the warped maps.

    On the CPU, under autograd, in training mode (BatchNorm batch statistics) and for shapes the kernel does not take, the
    reference's torch arithmetic runs (`forward_torch`).  Inference on the device is one heal_conv1x1 + one heal_disco_fuse launch
    per scene, with these identities (DiscoNet):
      1. inference BatchNorm folds into the convolution before it;
      2. conv1_1(cat(nbr_j, x_0)) = W1n nbr_j + (W1e x_0 + b1): the ego term E0 is computed once per scene;
      3. the softmax of one logit is 1: a single agent's output is its warped map, the MLP is skipped.
    HEAL_DISCO_FUSED=0 runs the torch arithmetic on the device too (the A/B switch of scripts/disconet_bench.py)."""

    def __init__(self, feature_dims):
        super().__init__()
        from heal_amd.opencood.models.fuse_modules.disco_fuse import PixelWeightLayer
        self.pixel_weight_layer = PixelWeightLayer(feature_dims)

    # ---- the reference's arithmetic ----------------------------------------------------------------------------------------
    def forward_torch(self, x, record_len, affine_matrix):
        """fusion_in_one.py:175-201 as written (the CPU, gradient, training and unsupported-shape path)."""
        _, C, H, W = x.shape
        lens = record_len_to_list(record_len)
        aff = _torch_affine(affine_matrix, x)
        out = []
        for b, feats in enumerate(regroup(x, lens)):
            N = lens[b]
            t_matrix = aff[b][:N, :N, :, :]
            neighbor = _warp_affine_simple(feats, t_matrix[0, :, :, :], (H, W))
            ego = feats[0].view(1, C, H, W).expand(N, -1, -1, -1)
            weight = self.pixel_weight_layer(torch.cat((neighbor, ego), dim=1))        # [N, 1, H, W]
            weight = torch.softmax(weight, dim=0).expand(-1, C, -1, -1)
            out.append(torch.sum(weight * neighbor, dim=0))
        return torch.stack(out)

    # ---- inference on the device -------------------------------------------------------------------------------------------
    def fused_ok(self, x, lens):
        C, H, W = (int(v) for v in x.shape[1:])
        ego_ok = (H * W) % 4 == 0 or ops.linear_supported(H * W, C, ops.DISCO_WIDTHS[0])     # how E0 is computed
        return (x.is_cuda and x.dtype == torch.float32 and not self.training
                and not (torch.is_grad_enabled() and x.requires_grad) and max(lens) <= ops.DISCO_MAX_AGENTS
                and C % 4 == 0 and C == self.pixel_weight_layer.conv1_1.in_channels // 2 and ego_ok
                and switches.on("HEAL_DISCO_FUSED"))

    def _weights(self):
        """(W1n in A-fragment order, W1e [128, C, 1, 1], b1, W2, b2, W3, b3, w4, b4) with the BatchNorms folded, from the parameters
        and running statistics (derived store: rebuilt when one of them changes, capture-safe)."""
        from heal_amd.derived import derived
        pw = self.pixel_weight_layer
        pairs = ((pw.conv1_1, pw.bn1_1), (pw.conv1_2, pw.bn1_2), (pw.conv1_3, pw.bn1_3))
        srcs = tuple(t for conv, bn in pairs for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var))
        srcs += (pw.conv1_4.weight, pw.conv1_4.bias)

        def build():
            folded = []
            for conv, bn in pairs:
                scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
                w = conv.weight.reshape(conv.out_channels, conv.in_channels) * scale[:, None]
                folded.append((w, (conv.bias - bn.running_mean) * scale + bn.bias))
            (w1, b1), (w2, b2), (w3, b3) = folded
            C = w1.shape[1] // 2
            return (ops.mfma_a_fragments(w1[:, :C].contiguous()), w1[:, C:].reshape(-1, C, 1, 1).contiguous(), b1.contiguous(),
                    w2.contiguous(), b2.contiguous(), w3.contiguous(), b3.contiguous(),
                    pw.conv1_4.weight.reshape(-1).contiguous(), pw.conv1_4.bias.reshape(-1).contiguous())
        return derived("disco_fold", srcs, build, tuple(float(bn.eps) for _, bn in pairs))

    def _ego_term(self, x0, w1e, b1):
        """E0 = W1e x_0 + b1 [128, H, W]: heal_conv1x1 on NCHW (heal_linear on the token-major copy when H * W % 4)."""
        C, H, W = (int(v) for v in x0.shape)
        if (H * W) % 4 == 0:
            return ops.conv1x1(x0.unsqueeze(0), w1e, b1)[0]
        y = ops.linear(x0.reshape(C, H * W).t().contiguous(), w1e.view(-1, C), b1)
        return y.t().contiguous().view(-1, H, W)

    def fuse_scene(self, feats, rows, f64, return_scores=False):
        """feats [n, C, H, W] (one scene), rows [n, 2, 3] the affine rows t[0, :n] -> [C, H, W] (and the logits [n, H, W])."""
        feats = feats.contiguous()
        if feats.shape[0] == 1 and not return_scores:       # (3)
            return ops.disco_fuse(feats, rows, f64, None, None, None, None, None, None, None, None)
        w1n, w1e, b1, w2, b2, w3, b3, w4, b4 = self._weights()
        e0 = self._ego_term(feats[0], w1e, b1)               # (2)
        return ops.disco_fuse(feats, rows, f64, e0, w1n, w2, b2, w3, b3, w4, b4, return_scores=return_scores)

    def forward(self, x, record_len, affine_matrix):
        lens = record_len_to_list(record_len)
        if not self.fused_ok(x, lens):
            return self.forward_torch(x, record_len, affine_matrix)
        aff, f64 = _host_affine(affine_matrix)
        out = []
        for b, feats in enumerate(regroup(x, lens)):
            n = feats.shape[0]
            out.append(self.fuse_scene(feats, aff[b][0, :n], f64))
        return torch.stack(out)


class Where2commFusion(nn.Module):
    """fusion_in_one.py:431-484 (with where2comm_attn.py:64-103).  Per scene: every agent warped into the ego frame (the ego too),
    then per pixel an nn.MultiheadAttention of the ego over the agents (no key mask: an agent that misses the pixel is a zero vector
    and keeps its share), out-projection + residual (the WARPED ego) + LayerNorm, feed-forward + residual + LayerNorm.  One agent
    is not the identity: the projections, both LayerNorms and the feed-forward still run.

    On the CPU, under autograd, for more agents than the kernel takes and for shapes the kernels refuse, the reference's torch
    arithmetic runs (`forward_torch`).  Inference on the device (Where2comm) rests on W warp(x) = warp(W x): the K | V
    projection of all agents and the Q projection of the egos are two heal_conv1x1 launches on the UNWARPED maps without bias,
    heal_warp_mha_fuse samples them, adds the biases and attends (one launch per scene), and the tail runs once on the stacked
    batch in NCHW (heal_conv1x1 with fused residual / ReLU, heal_layernorm_nchw).
    `fused` (class attribute; set it on an instance for an A/B, scripts/where2comm_bench.py) = False keeps the torch arithmetic on
    the device too."""
    fused = True

    def __init__(self, feature_dims):
        super().__init__()
        from heal_amd.opencood.models.fuse_modules.where2comm_attn import EncodeLayer
        self.mha_fusion = EncodeLayer(feature_dims)

    # ---- the reference's arithmetic ----------------------------------------------------------------------------------------
    def forward_torch(self, x, record_len, affine_matrix):
        """fusion_in_one.py:442-484 as written (the CPU, gradient and unsupported-shape path)."""
        _, C, H, W = x.shape
        lens = record_len_to_list(record_len)
        aff = _torch_affine(affine_matrix, x)
        out = []
        for b, feats in enumerate(regroup(x, lens)):
            N = lens[b]
            t_matrix = aff[b][:N, :N, :, :]
            neighbor = _warp_affine_simple(feats, t_matrix[0, :, :, :], (H, W))
            tokens = neighbor.permute(0, 2, 3, 1).flatten(1, 2)                     # [N, HW, C]
            fused = self.mha_fusion(tokens[0:1], tokens, tokens)                    # [1, HW, C]
            out.append(fused.permute(0, 2, 1).reshape(C, H, W))
        return torch.stack(out)

    # ---- inference on the device -------------------------------------------------------------------------------------------
    def fused_ok(self, x, lens):
        C, H, W = (int(v) for v in x.shape[1:])
        attn = self.mha_fusion.attn
        return (self.fused and x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad)
                and C == attn.embed_dim and C % attn.num_heads == 0 and ops.conv1x1_supported(C, 2 * C, H * W)
                and max(lens) <= ops.W2C_MAX_AGENTS)

    def _weights(self):
        """(Wq [C,C,1,1], Wkv [2C,C,1,1], bq, bk, bv, Wo, W1, W2 as [C,C,1,1]) split and reshaped from the parameters (derived store:
        rebuilt when one of them changes in place, capture-safe)."""
        from heal_amd.derived import derived
        e = self.mha_fusion
        srcs = (e.attn.in_proj_weight, e.attn.in_proj_bias, e.attn.out_proj.weight, e.linear1.weight, e.linear2.weight)

        def build():
            C = e.attn.embed_dim
            w, b = e.attn.in_proj_weight, e.attn.in_proj_bias
            as_conv = lambda m: m.reshape(-1, C, 1, 1).contiguous()      # noqa: E731
            return (as_conv(w[:C]), as_conv(w[C:]), b[:C].contiguous(), b[C:2 * C].contiguous(), b[2 * C:].contiguous(),
                    as_conv(e.attn.out_proj.weight), as_conv(e.linear1.weight), as_conv(e.linear2.weight))
        return derived("where2comm_split", srcs, build)

    def forward(self, x, record_len, affine_matrix):
        lens = record_len_to_list(record_len)
        if not self.fused_ok(x, lens):
            return self.forward_torch(x, record_len, affine_matrix)
        aff, f64 = _host_affine(affine_matrix)
        e = self.mha_fusion
        wq, wkv, bq, bk, bv, wo, w1, w2 = self._weights()
        x = x.contiguous()
        starts = [sum(lens[:b]) for b in range(len(lens))]
        egos = x[:1] if len(lens) == 1 else torch.stack([x[s] for s in starts])
        kv = ops.conv1x1(x, wkv)                          # [sum n, 2C, H, W]: K over V of every agent, unwarped, no bias
        q = ops.conv1x1(egos, wq)                         # [B, C, H, W]: the egos only
        ctx, ego_w = [], []
        for b, (s, n) in enumerate(zip(starts, lens)):
            c, w = ops.warp_mha_fuse(q[b], kv[s:s + n], egos[b], bq, bk, bv, e.attn.num_heads, aff[b][0, :n], f64)
            ctx.append(c)
            ego_w.append(w)
        ctx = ctx[0].unsqueeze(0) if len(lens) == 1 else torch.stack(ctx)
        ego_w = ego_w[0].unsqueeze(0) if len(lens) == 1 else torch.stack(ego_w)
        o1 = ops.layernorm_nchw(ops.conv1x1(ctx, wo, e.attn.out_proj.bias, residual=ego_w), e.norm1.weight, e.norm1.bias, e.norm1.eps)
        h = ops.conv1x1(o1, w1, e.linear1.bias, act=1)
        return ops.layernorm_nchw(ops.conv1x1(h, w2, e.linear2.bias, residual=o1), e.norm2.weight, e.norm2.bias, e.norm2.eps)


class ScaledDotProductAttention(nn.Module):
    """fusion_in_one.py:14-45: softmax(q k^T / sqrt(dim)) v.  No parameters."""

    def __init__(self, dim):
        super().__init__()
        self.sqrt_dim = float(np.sqrt(dim))

    def forward(self, query, key, value):
        score = torch.bmm(query, key.transpose(1, 2)) / self.sqrt_dim
        return torch.bmm(torch.softmax(score, -1), value)


class Who2comFusion(nn.Module):
    """fusion_in_one.py:486-539.  Per scene: AttFusion's ego row (every agent warped into the ego frame, softmax(x_0 . x_j /
    sqrt(feature_dims)) weights), concatenated BEHIND the ego's UNWARPED map, then a 3x3 convolution 2C to C.

    Inference on the device: heal_warp_att_fuse_levels (one level) per scene, the concatenation, and ONE heal_conv3x3 on the stacked
    batch; otherwise the reference's torch arithmetic (`forward_torch`).  `fused` as on Where2commFusion."""
    fused = True

    def __init__(self, feature_dims):
        super().__init__()
        self.att = ScaledDotProductAttention(feature_dims)
        self.decode_layer = nn.Conv2d(feature_dims * 2, feature_dims, kernel_size=3, stride=1, padding=1)

    def forward_torch(self, x, record_len, affine_matrix):
        """fusion_in_one.py:493-539 as written (the CPU, gradient and unsupported-shape path)."""
        _, C, H, W = x.shape
        lens = record_len_to_list(record_len)
        aff = _torch_affine(affine_matrix, x)
        out = []
        for b, feats in enumerate(regroup(x, lens)):
            N = lens[b]
            t_matrix = aff[b][:N, :N, :, :]
            neighbor = _warp_affine_simple(feats, t_matrix[0, :, :, :], (H, W))
            ego = feats[0]
            neighbor = neighbor.view(N, C, -1).permute(2, 0, 1)
            neighbor = self.att(neighbor, neighbor, neighbor)
            neighbor = neighbor.permute(1, 2, 0).view(N, C, H, W)[0, ...]
            out.append(self.decode_layer(torch.cat((ego, neighbor), dim=0).unsqueeze(0)))
        return torch.cat(out, dim=0)

    def fused_ok(self, x, lens):
        return (self.fused and x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad)
                and int(x.shape[1]) == self.decode_layer.out_channels and max(lens) <= ops.WARP_ATT_MAX_AGENTS)

    def forward(self, x, record_len, affine_matrix):
        lens = record_len_to_list(record_len)
        if not self.fused_ok(x, lens):
            return self.forward_torch(x, record_len, affine_matrix)
        aff, f64 = _host_affine(affine_matrix)
        x = x.contiguous()
        cat, start = [], 0
        for b, n in enumerate(lens):
            fused = ops.warp_att_fuse_levels([x[start:start + n]], aff[b][0, :n], f64, "att", [self.att.sqrt_dim])[0]
            cat.append(torch.cat((x[start], fused), dim=0))
            start += n
        cat = cat[0].unsqueeze(0) if len(lens) == 1 else torch.stack(cat)
        return ops.conv3x3(cat, self.decode_layer.weight, self.decode_layer.bias)


class V2VNetFusion(nn.Module):
    """fusion_in_one.py:203-318 (with sub_modules/convgru.py).  num_iteration Jacobi rounds of message passing: every node i
    warps every node j into its frame, msg_ij = msg_cnn(cat(nbr_ij, x_i)) * roi_mask_ij, agg_i = mean_j | max_j msg_ij, then
    x_i' = ConvGRU(cat(x_i, agg_i)) (zero hidden state, one step) or x_i + agg_i; the output is mlp(node 0) per scene.

    On the CPU, under autograd and for shapes the kernels do not take, the reference's torch arithmetic runs.  Inference on
    the device uses these identities:
      1. only node 0 of the last round reaches the output: the last round computes ego 0 only;
      2. msg_cnn(cat(nbr, x_i)) = W_n * nbr + (W_e * x_i + b): the ego term E_i once per ego, and
         mean: agg_i = (sum_j m_ij (W_n * nbr_ij) + (sum_j m_ij) E_i) / N;  max: agg_i = max_j m_ij (W_n * nbr_ij + E_i);
      3. with h = 0, reset * h = 0 and every hidden-channel slice multiplies zeros: h' = sigmoid(beta) * tanh(can), from the beta
         half of conv_gates and the input half of conv_can;
      4. the x_i parts of msg_cnn, beta and can are one stacked 3x3 convolution C -> 3C; the agg_i parts one C -> 2C.
    The one divergence: where a gate is NaN or Inf, the reference's (1 - u) * h = (1 - u) * 0 propagates a NaN that (3) does
    not form (and the reset gate, which the reference computes but multiplies by zero, is never evaluated).
    HEAL_V2VNET_FUSED=0 runs the torch arithmetic on the device too (the A/B switch of scripts/v2vnet_bench.py)."""

    def __init__(self, args):
        super().__init__()
        from heal_amd.opencood.models.sub_modules.convgru import ConvGRU
        in_channels = args["in_channels"]
        H, W = args["conv_gru"]["H"], args["conv_gru"]["W"]
        kernel_size = args["conv_gru"]["kernel_size"]
        num_gru_layers = args["conv_gru"]["num_layers"]
        self.num_iteration = args["num_iteration"]
        self.gru_flag = args["gru_flag"]
        self.agg_operator = args["agg_operator"]
        self.msg_cnn = nn.Conv2d(in_channels * 2, in_channels, kernel_size=3, stride=1, padding=1)
        self.conv_gru = ConvGRU(input_size=(H, W), input_dim=in_channels * 2, hidden_dim=[in_channels] * num_gru_layers,
                                kernel_size=kernel_size, num_layers=num_gru_layers, batch_first=True, bias=True,
                                return_all_layers=False)
        self.mlp = nn.Linear(in_channels, in_channels)

    def _check(self, H, W):
        if self.agg_operator not in ("avg", "max"):
            raise ValueError("agg_operator has wrong value")
        if self.gru_flag and (H, W) != (self.conv_gru.height, self.conv_gru.width):
            raise ValueError(f"V2VNetFusion: the fusion map is {H}x{W} but conv_gru was built for {self.conv_gru.height}x"
                             f"{self.conv_gru.width} (conv_gru.H / W in the YAML must equal the map size)")

    # ---- the reference's arithmetic ----------------------------------------------------------------------------------------
    def forward_torch(self, x, record_len, affine_matrix):
        """fusion_in_one.py:238-318 as written (the CPU, gradient and unsupported-shape path)."""
        _, C, H, W = x.shape
        lens = record_len_to_list(record_len)
        aff = _torch_affine(affine_matrix, x)
        B, L = aff.shape[:2]
        split_x = regroup(x, lens)
        roi_mask = torch.zeros((B, L, L, 1, H, W)).to(x)
        for b in range(B):
            for i in range(lens[b]):
                roi_mask[b, i] = _warp_affine_simple(torch.ones((L, 1, H, W)).to(x), aff[b][i], (H, W))
        batch_node_features = split_x
        for _ in range(self.num_iteration):
            batch_updated = []
            for b in range(B):
                N = lens[b]
                t_matrix = aff[b][:N, :N, :, :]
                updated = []
                for i in range(N):
                    mask = roi_mask[b, i, :N, ...]
                    neighbor = _warp_affine_simple(batch_node_features[b], t_matrix[i], (H, W))
                    ego = batch_node_features[b][i].unsqueeze(0).repeat(N, 1, 1, 1)
                    message = self.msg_cnn(torch.cat([neighbor, ego], dim=1)) * mask
                    agg = torch.mean(message, dim=0) if self.agg_operator == "avg" else torch.max(message, dim=0)[0]
                    if self.gru_flag:
                        cat_feature = torch.cat([batch_node_features[b][i, ...], agg], dim=0)
                        gru_out = self.conv_gru(cat_feature.unsqueeze(0).unsqueeze(0))[0][0].squeeze(0).squeeze(0)
                    else:
                        gru_out = batch_node_features[b][i, ...] + agg
                    updated.append(gru_out.unsqueeze(0))
                batch_updated.append(torch.cat(updated, dim=0))
            batch_node_features = batch_updated
        out = torch.cat([itm[0, ...].unsqueeze(0) for itm in batch_node_features], dim=0)
        return self.mlp(out.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)

    # ---- inference on the device -------------------------------------------------------------------------------------------
    def fused_ok(self, x, lens):
        C, H, W = (int(v) for v in x.shape[1:])
        ks_ok = all(tuple(k) == (3, 3) for k in (c.conv_gates.kernel_size for c in self.conv_gru.cell_list))
        mlp_ok = (H * W) % 4 == 0 or ops.linear_supported(H * W, C, C)
        return (x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad) and ks_ok and mlp_ok
                and max(lens) <= ops.V2V_MAX_AGENTS and switches.on("HEAL_V2VNET_FUSED"))

    def _weights(self):
        """(W_n, stacked x_i weight, stacked bias, agg weight | None, [(layer weight, layer bias)] for GRU layers >= 1), from the
        parameters by slicing (derived store: rebuilt when a parameter changes)."""
        from heal_amd.derived import derived
        C = self.mlp.in_features
        cells = list(self.conv_gru.cell_list) if self.gru_flag else []
        srcs = (self.msg_cnn.weight, self.msg_cnn.bias) + tuple(t for c in cells[:1] for t in (c.conv_gates.weight, c.conv_gates.bias,
                                                                                               c.conv_can.weight, c.conv_can.bias))

        def build():
            wm, bm = self.msg_cnn.weight, self.msg_cnn.bias
            w_n = wm[:, :C].contiguous()
            if not cells:
                return w_n, wm[:, C:].contiguous(), bm.contiguous(), None
            g, c0 = cells[0].conv_gates, cells[0].conv_can
            w_x = torch.cat([wm[:, C:], g.weight[C:2 * C, :C], c0.weight[:, :C]]).contiguous()
            b_x = torch.cat([bm, g.bias[C:2 * C], c0.bias]).contiguous()
            w_a = torch.cat([g.weight[C:2 * C, C:2 * C], c0.weight[:, C:2 * C]]).contiguous()
            return w_n, w_x, b_x, w_a
        w_n, w_x, b_x, w_a = derived("v2vnet_stack", srcs, build, (C, bool(cells)))
        layers = []
        for c in cells[1:]:
            g, cc = c.conv_gates, c.conv_can
            layers.append(derived("v2vnet_gru_layer", (g.weight, g.bias, cc.weight, cc.bias), lambda g=g, cc=cc: (
                torch.cat([g.weight[C:2 * C, :C], cc.weight[:, :C]]).contiguous(), torch.cat([g.bias[C:2 * C], cc.bias]).contiguous()),
                (C,)))
        return w_n, w_x, b_x, w_a, layers

    def _masks(self, n, n_ego, rows, H, W, dev, f64):
        """roi_mask[i, j] = warp_affine_simple(ones, t[i, j]) for egos i < n_ego, j < n -> [n_ego, n, H, W] (heal_warp_agent)."""
        ones = torch.ones((1, H, W), dtype=torch.float32, device=dev)
        zeros = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
        score = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        masks = torch.empty((n_ego, n, H, W), dtype=torch.float32, device=dev)
        for i in range(n_ego):
            for j in range(n):
                ops.warp_agent(ones, zeros, rows[i][j], f64, out=(masks[i, j], score))
        return masks

    def fuse_scene(self, feats, rows, f64):
        """feats [n, C, H, W] (one scene), rows[i][j] the (2, 3) affine of t[i, j] -> node 0 after num_iteration rounds [1, C, H, W]."""
        n, C, H, W = (int(v) for v in feats.shape)
        dev = feats.device
        w_n, w_x, b_x, w_a, layers = self._weights()
        mode = "mean" if self.agg_operator == "avg" else "max"
        T = self.num_iteration
        masks = self._masks(n, n if T > 1 else 1, rows, H, W, dev, f64)
        zeros = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
        score = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        x = feats.contiguous()
        for it in range(T):
            n_ego = n if it < T - 1 else 1                    # (1) the last round: ego 0 only
            xs = torch.empty((n_ego, n, C, H, W), dtype=torch.float32, device=dev)
            for i in range(n_ego):
                for j in range(n):
                    ops.warp_agent(x[j], zeros, rows[i][j], f64, out=(xs[i, j], score))
            ego = x[:n_ego]
            stacked = ops.conv3x3(ego, w_x, b_x)              # (4) [E | beta_x | can_x] or E alone
            agg = ops.v2v_message(xs, masks[:n_ego], stacked, w_n, None if self.gru_flag else ego, mode)   # (2)
            if self.gru_flag:                                 # (3)
                h = ops.gru_zero_state(ops.conv3x3(agg, w_a), stacked[:, C:])
                for w_l, b_l in layers:
                    h = ops.gru_zero_state(ops.conv3x3(h, w_l, b_l))
                x = h
            else:
                x = agg
        return x[:1]

    def _mlp(self, out):
        """mlp over channels of out [B, C, H, W]: heal_conv1x1 on NCHW (heal_linear on the token-major copy when H*W % 4)."""
        B, C, H, W = (int(v) for v in out.shape)
        if (H * W) % 4 == 0:
            return ops.conv1x1(out, self.mlp.weight.view(C, C, 1, 1), self.mlp.bias)
        y = ops.linear(out.permute(0, 2, 3, 1).contiguous(), self.mlp.weight, self.mlp.bias)
        return y.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()

    def forward(self, x, record_len, affine_matrix):
        C, H, W = (int(v) for v in x.shape[1:])
        self._check(H, W)
        lens = record_len_to_list(record_len)
        if not self.fused_ok(x, lens):
            return self.forward_torch(x, record_len, affine_matrix)
        aff, f64 = _host_affine(affine_matrix)
        nodes = []
        for b, feats in enumerate(regroup(x, lens)):
            n = feats.shape[0]
            rows = [aff[b][i, :n] for i in range(n)]
            nodes.append(self.fuse_scene(feats, rows, f64))
        return self._mlp(torch.cat(nodes))


# ---- multiscale fusion of HeterModelBaselineMs (CoAlign) ------------------------------------------------------------------------
MS_MAX_AGENTS = ops.WARP_ATT_MAX_AGENTS


def _ms_mode(fusion_net):
    kinds = {type(m) for m in fusion_net}
    if kinds == {AttFusion}:
        return "att"
    if kinds == {MaxFusion}:
        return "max"
    raise NotImplementedError(f"multiscale fusion takes AttFusion or MaxFusion at every level, got {sorted(k.__name__ for k in kinds)}")


def ms_fused_ok(fusion_net, feature_list, lens):
    """True when `fuse_levels` runs heal_warp_att_fuse_levels: inference on the device in fp32, at most 8 agents per scene and 4
    levels.  HEAL_MSATT_FUSED=0 keeps the torch arithmetic on the device too (the A/B switch of scripts/coalign_bench.py)."""
    return (all(f.is_cuda and f.dtype == torch.float32 for f in feature_list)
            and not (torch.is_grad_enabled() and any(f.requires_grad for f in feature_list))
            and max(lens) <= MS_MAX_AGENTS and 1 <= len(feature_list) <= ops.WARP_ATT_MAX_LEVELS
            and switches.on("HEAL_MSATT_FUSED"))


def fuse_level_torch(module, x, lens, aff):
    """One level as the reference computes it (fusion_in_one.py:87-151): warp_affine_simple with row t[0, :n] of every scene, then
    the maximum over agents, or row 0 of softmax(X X^T / sqrt_dim) X per pixel.  The CPU and gradient path."""
    C, H, W = x.shape[1:]
    out = []
    for b, feats in enumerate(regroup(x, lens)):
        n = feats.shape[0]
        ego = _warp_affine_simple(feats, aff[b][0, :n], (H, W))
        if isinstance(module, MaxFusion):
            out.append(torch.max(ego, dim=0)[0])
            continue
        t = ego.view(n, C, -1).permute(2, 0, 1)                                  # [HW, n, C]
        attn = torch.softmax(torch.bmm(t, t.transpose(1, 2)) / module.sqrt_dim, -1)
        out.append(torch.bmm(attn, t).permute(1, 2, 0).view(n, C, H, W)[0])
    return torch.stack(out)


def fuse_levels(fusion_net, feature_list, record_len, affine_matrix):
    """HeterModelBaselineMs' fusion loop (heter_model_baseline_ms.py:204-206): fusion_net[i](feature_list[i], record_len,
    affine_matrix) for every level, all levels with the same normalised affine matrix -> list of [B, C_i, H_i, W_i].
    Inference on the device: ONE heal_warp_att_fuse_levels launch per scene (`ms_fused_ok`); otherwise the reference's torch
    arithmetic.  A scene with more than 8 agents is refused on every path (the reference's configurations stop at max_cav 5)."""
    if len(fusion_net) != len(feature_list):
        raise ValueError(f"{len(fusion_net)} fusion modules for {len(feature_list)} feature levels")
    mode = _ms_mode(fusion_net)
    lens = record_len_to_list(record_len)
    if max(lens) > MS_MAX_AGENTS:
        raise ValueError(f"multiscale fusion: a scene has {max(lens)} agents, more than the {MS_MAX_AGENTS} it is built for")
    if not ms_fused_ok(fusion_net, feature_list, lens):
        aff = _torch_affine(affine_matrix, feature_list[0])
        return [fuse_level_torch(m, x, lens, aff) for m, x in zip(fusion_net, feature_list)]
    aff, f64 = _host_affine(affine_matrix)
    sqrt_dims = [m.sqrt_dim for m in fusion_net] if mode == "att" else None
    scenes, start = [], 0
    for b, n in enumerate(lens):
        scenes.append(ops.warp_att_fuse_levels([f[start:start + n] for f in feature_list], aff[b][0, :n], f64, mode, sqrt_dims))
        start += n
    if len(scenes) == 1:
        return [y.unsqueeze(0) for y in scenes[0]]
    return [torch.stack([s[i] for s in scenes]) for i in range(len(feature_list))]


def build_fusion(args):
    """The single-scale fusion operator a model YAML names (`fusion_method`: max | att | v2xvit | cobevt | v2vnet | disconet | where2comm
    | who2com -- the eight of heter_model_baseline.py:96-111).  A method named without its argument entry (args[method]) is answered
    like an unknown one, with the NotImplementedError that lists the built methods (the reference raises KeyError there)."""
    method = args["fusion_method"]
    if method == "max":
        return MaxFusion()
    if method == "att":
        return AttFusion(args["att"]["feat_dim"])
    if method == "v2xvit":
        return V2XViTFusion(args["v2xvit"])
    if method == "cobevt":
        return CoBEVT(args["cobevt"])
    if method == "v2vnet":
        return V2VNetFusion(args["v2vnet"])
    if method == "disconet":
        return DiscoFusion(args["disconet"]["feat_dim"])
    if method == "where2comm" and "where2comm" in args:
        return Where2commFusion(args["where2comm"])
    if method == "who2com" and "who2com" in args:
        return Who2comFusion(args["who2com"])
    raise NotImplementedError(f"fusion_method '{method}' is not built, or its argument entry args['{method}'] is missing (SURVEY 2, row 2): "
                              "max, att, v2xvit, cobevt, v2vnet, disconet, where2comm and who2com are built")
