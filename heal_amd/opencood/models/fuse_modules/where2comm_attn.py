"""EncodeLayer and Where2comm of the reference's where2comm_attn.py.

EncodeLayer (reference: opencood/models/fuse_modules/where2comm_attn.py:64-103): multi-head attention of a query
over a short sequence, a residual LayerNorm, a two-layer feed-forward net and a second residual LayerNorm.  Plain torch layers with
the reference's attribute names, so a reference checkpoint's keys load strictly: this is the CPU, gradient and unsupported-shape
arithmetic of Where2commFusion (fusion_in_one.py); inference on the device reads the parameters and runs heal_conv1x1,
heal_warp_mha_fuse and heal_layernorm_nchw instead.

Where2comm (:174-341): the class docstring below."""
import torch
import torch.nn as nn

from heal_amd import ops
from heal_amd.opencood.models._heter_common import record_len_to_list
from heal_amd.opencood.models.comm_modules.where2comm import Communication
from heal_amd.opencood.models.fuse_modules import fusion_in_one as F1
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm


class EncodeLayer(nn.Module):
    def __init__(self, channels, n_head=8, dropout=0):
        super().__init__()
        self.attn = nn.MultiheadAttention(channels, n_head, dropout)
        self.linear1 = nn.Linear(channels, channels)
        self.linear2 = nn.Linear(channels, channels)
        self.norm1 = nn.LayerNorm(channels)
        self.norm2 = nn.LayerNorm(channels)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.relu = nn.ReLU()

    def forward(self, q, k, v):
        """(seq, batch, feature) order: q [1, HW, C], k and v [n, HW, C] -> [1, HW, C]."""
        context, _ = self.attn(q, k, v)
        output1 = self.norm1(q + self.dropout1(context))
        context = self.linear2(self.relu(self.linear1(output1)))
        return self.norm2(output1 + self.dropout2(context))


class Where2comm(nn.Module):
    """Where2comm.forward (reference: where2comm_attn.py:174-341): the communication masks from the agents' confidence maps
    (comm_modules/where2comm.py), every agent's map times its mask, warp into the ego frame and per-pixel attention (`ATTEN`, :44-54)
    or maximum (`MAX`, :56-61) over the agents -- single-scale (:311-339), or per level of a backbone whose later levels are
    computed inside the fusion (:254-310): `backbone.resnet(x)` gives every level from the unmasked input, `backbone.blocks[i]` is
    fed the MASKED level before it.  `backbone.deblocks` per level and the trailing one follow (:298-310).

        forward(x, rm, record_len, pairwise_t_matrix, backbone=None) -> (x_fuse, communication_rates, {})

    x [sum n, C, H, W], rm the confidence logits [sum n, A, H, W], pairwise_t_matrix the RAW [B, L, L, 4, 4] matrix, normalised here
    with the H and W of x (:248-252: transformation_utils.normalize_pairwise_tfm with discrete_ratio = voxel_size[0] and
    downsample_rate).  The only parameters are `naive_communication.gaussian_filter.{weight, bias}`, as in the reference.

    Inference on the device: one heal_comm_mask pass (ops.comm_mask) and ONE heal_warp_att_fuse_levels_masked launch per scene; the
    masked maps are read by the fusion alone and never written -- except in the `backbone.blocks` form, where the masked level is
    the next block's input and the product is a broadcast multiply (the kernel then reads x m with m once more: m m = m).  Under
    autograd the mask still comes from the kernel (it carries no gradient) and the features go through x * mask, the
    differentiable warp and fusion_in_one.fuse_level_torch.  On CPU tensors, and on the device under HEAL_COMM_FUSED=0, the
    reference's torch composition runs.  A scene with more than 8 agents is refused on every path, as fusion_in_one.fuse_levels does.

    Kept as the reference writes it: the single-scale path indexes the concatenated masks by SCENE (:334 `communication_masks[b]`),
    so every agent of scene b is multiplied by the mask of global agent b; without a `communication` entry the rate is an integer
    zero tensor on the device (:271, :322).
    `agg_operator.mode: Transformer` is refused: it cannot run in the reference (single-scale the module is stored as
    `fuse_network` but called as `fuse_modules`, :213 against :338; multi-scale TransformerFusion.forward is called with one argument
    instead of four, :295 against :113; its `with_scm` path passes `quality_map=` to a stock nn.MultiheadAttention, :91)."""

    def __init__(self, args):
        super().__init__()
        self.communication = False
        self.round = 1
        if "communication" in args:
            self.communication = True
            self.naive_communication = Communication(args["communication"])
            if "round" in args["communication"]:
                self.round = args["communication"]["round"]
        self.discrete_ratio = args["voxel_size"][0]
        self.downsample_rate = args["downsample_rate"]
        self.agg_mode = args["agg_operator"]["mode"]
        self.multi_scale = args["multi_scale"]
        if self.agg_mode == "Transformer":
            raise NotImplementedError(
                "Where2comm: agg_operator.mode 'Transformer' is not built because it cannot run in the reference: single-scale the "
                "module is stored as fuse_network but called as fuse_modules (where2comm_attn.py:213, :338), multi-scale "
                "TransformerFusion.forward gets one argument instead of four (:295, :113), and with_scm passes quality_map= to a "
                "stock nn.MultiheadAttention (:91).  ATTEN and MAX are built")
        if self.agg_mode not in ("ATTEN", "MAX"):
            raise NotImplementedError(f"Where2comm: agg_operator.mode {self.agg_mode!r}: ATTEN and MAX are built")
        make = (lambda dim: F1.AttFusion(dim)) if self.agg_mode == "ATTEN" else (lambda dim: F1.MaxFusion())
        if self.multi_scale:
            self.num_levels = len(args["layer_nums"])
            self.fuse_modules = nn.ModuleList([make(args["num_filters"][idx]) for idx in range(self.num_levels)])
        else:
            self.fuse_modules = make(args["agg_operator"]["feature_dim"] if self.agg_mode == "ATTEN" else None)

    # ---- pieces -------------------------------------------------------------------------------------------------------------
    def _masks(self, rm, lens, n_levels, device):
        """([mask per level] | None, rate)."""
        if not self.communication:
            return None, torch.zeros((), dtype=torch.int64, device=device)           # :271, :322  torch.tensor(0).to(x.device)
        return self.naive_communication.level_masks(rm, lens, n_levels)

    def _fused_ok(self, feats):
        return (all(f.is_cuda and f.dtype == torch.float32 for f in feats)
                and not (torch.is_grad_enabled() and any(f.requires_grad for f in feats))
                and 1 <= len(feats) <= ops.WARP_ATT_MAX_LEVELS and ops.comm_fused_enabled())

    def _fuse(self, modules, feats, masks, premultiplied, lens, aff):
        """feats[l] [sum n, C_l, H_l, W_l], masks[l] [sum n, 1, H_l, W_l] | masks None, premultiplied[l]: feats[l] already holds
        x m -> [fused level l [B, C_l, H_l, W_l]]."""
        if not self._fused_ok(feats):
            a = aff if isinstance(aff, torch.Tensor) else torch.from_numpy(aff)
            a = a.to(feats[0].device)
            out = []
            for l, (m, x) in enumerate(zip(modules, feats)):
                if masks is not None and not premultiplied[l]:
                    x = x * masks[l]
                out.append(F1.fuse_level_torch(m, x, lens, a))
            return out
        aff, f64 = F1._host_affine(aff)
        mode = "att" if self.agg_mode == "ATTEN" else "max"
        sqrt_dims = [m.sqrt_dim for m in modules] if mode == "att" else None
        feats = [f.contiguous() for f in feats]
        scenes, start = [], 0
        for b, n in enumerate(lens):
            ms = None if masks is None else [m[start:start + n] for m in masks]
            scenes.append(ops.warp_att_fuse_levels([f[start:start + n] for f in feats], aff[b][0, :n], f64, mode, sqrt_dims, masks=ms))
            start += n
        if len(scenes) == 1:
            return [y.unsqueeze(0) for y in scenes[0]]
        return [torch.stack([s[i] for s in scenes]) for i in range(len(feats))]

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, x, rm, record_len, pairwise_t_matrix, backbone=None):
        H, W = int(x.shape[2]), int(x.shape[3])
        lens = record_len_to_list(record_len)
        if max(lens) > F1.MS_MAX_AGENTS:
            raise ValueError(f"Where2comm: a scene has {max(lens)} agents, more than the {F1.MS_MAX_AGENTS} it is built for")
        aff = normalize_pairwise_tfm(pairwise_t_matrix, H, W, self.discrete_ratio, self.downsample_rate)       # :248-252

        if not self.multi_scale:                                                                                # :311-339
            masks, rate = self._masks(rm, lens, 1, x.device)
            if masks is not None:
                # :334 `node_features * communication_masks[b]`: the mask of GLOBAL agent b for every agent of scene b
                masks = [torch.cat([masks[0][b:b + 1].expand(n, -1, -1, -1) for b, n in enumerate(lens)])]
            return self._fuse([self.fuse_modules], [x], masks, [False], lens, aff)[0], rate, {}

        L = self.num_levels
        masks, rate = self._masks(rm, lens, L, x.device)
        if hasattr(backbone, "resnet"):                                                                         # :257-262
            feats = list(backbone.resnet(x))[:L]
            premultiplied = [False] * L
        else:
            feats, premultiplied = [], []
            for i in range(L):
                x = backbone.blocks[i](x)
                feats.append(x)
                premultiplied.append(False)
                if masks is not None and i + 1 < L:
                    x = x * masks[i]                   # :269, :275: the masked level is the next block's input
                    feats[-1], premultiplied[-1] = x, True
        fused = self._fuse(self.fuse_modules, feats, masks, premultiplied, lens, aff)
        return backbone.decode_multiscale_feature(fused), rate, {}                                              # :298-310
