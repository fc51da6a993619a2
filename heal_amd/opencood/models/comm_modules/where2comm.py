"""Communication of Where2comm (reference: opencood/models/comm_modules/where2comm.py:9-78): every agent's confidence map becomes
a spatial mask that says which cells of its feature map are sent.

Same constructor arguments (`thre`, optional `gaussian_smooth: {k_size, c_sigma}`), the same `gaussian_filter` parameters with the
reference's initial values (:24-32 -- 1 / (2 pi sigma) exp(-(x^2 + y^2) / (2 sigma^2)): sigma, not sigma squared, in the prefactor,
as the reference writes it) and the same three return values.  `forward` is the reference's torch composition (the CPU path, and
the device path under HEAL_COMM_FUSED=0); `level_masks` is what Where2comm calls: on the device one heal_comm_mask pass
(ops.comm_mask) over all scenes and pyramid levels, otherwise the composition followed by max_pool2d per level.

Two properties of the reference are kept as written:
  * :69-71 `communication_mask_nodiag[::2] = ones_mask[::2]` forces the masks of agents 0, 2, 4, ... of a scene to ones, not only
    the ego's;
  * :63 the rate counts the first agent's ones BEFORE that override.
The filter's parameters stay in the state_dict (a checkpoint may carry other values) and are read, never recomputed.  The mask
carries no gradient, in the reference either (torch.where on a comparison)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from heal_amd import ops


class Communication(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.smooth = False
        self.thre = args["thre"]
        if "gaussian_smooth" in args:
            self.smooth = True
            kernel_size = args["gaussian_smooth"]["k_size"]
            c_sigma = args["gaussian_smooth"]["c_sigma"]
            self.gaussian_filter = nn.Conv2d(1, 1, kernel_size=kernel_size, stride=1, padding=(kernel_size - 1) // 2)
            self.init_gaussian_filter(kernel_size, c_sigma)
            self.gaussian_filter.requires_grad = False         # :22 sets an attribute of the module; the parameters stay trainable

    def init_gaussian_filter(self, k_size=5, sigma=1):
        center = k_size // 2
        x, y = np.mgrid[0 - center:k_size - center, 0 - center:k_size - center]
        g = 1 / (2 * np.pi * sigma) * np.exp(-(np.square(x) + np.square(y)) / (2 * np.square(sigma)))
        self.gaussian_filter.weight.data = torch.Tensor(g).to(self.gaussian_filter.weight.device).unsqueeze(0).unsqueeze(0)
        self.gaussian_filter.bias.data.zero_()

    def forward(self, batch_confidence_maps, record_len, pairwise_t_matrix=None):
        """:34-78.  batch_confidence_maps: one [n_b, A, H, W] map of logits per scene -> (the confidence maps times the masks per
        scene, the masks [sum n_b, 1, H, W], the mean over scenes of the first agent's share of ones)."""
        B = len(batch_confidence_maps)
        H, W = batch_confidence_maps[0].shape[2:]
        masks, rates, maps = [], [], []
        for b in range(B):
            ori = batch_confidence_maps[b].sigmoid().max(dim=1)[0].unsqueeze(1)
            smoothed = self.gaussian_filter(ori) if self.smooth else ori
            mask = torch.where(smoothed > self.thre, torch.ones_like(smoothed), torch.zeros_like(smoothed))
            rates.append(mask[0].sum() / (H * W))
            nodiag = mask.clone()
            nodiag[::2] = 1.0                                  # :69-71: every even agent of the scene, see the module docstring
            masks.append(nodiag)
            maps.append(ori * nodiag)
        return maps, torch.cat(masks, dim=0), sum(rates) / B

    def fused_ok(self, rm):
        k = self.gaussian_filter.kernel_size[0] if self.smooth else 1
        return (rm.is_cuda and rm.dtype == torch.float32 and ops.comm_fused_enabled()
                and (not self.smooth or (self.gaussian_filter.kernel_size == (k, k) and k % 2 == 1 and k <= ops.COMM_MAX_K)))

    def level_masks(self, rm, lens, n_levels):
        """rm [sum n_b, A, H, W] confidence logits of all scenes, lens the agents per scene -> ([masks of level 0 .. n_levels - 1],
        rate).  Level l is max_pool2d(., 2) of level l - 1 (where2comm_attn.py:264-275)."""
        rm = rm.detach()
        if self.fused_ok(rm):
            w = self.gaussian_filter.weight if self.smooth else None
            b = self.gaussian_filter.bias if self.smooth else None
            masks, _, rate = ops.comm_mask(rm, lens, w, b, self.thre, n_levels)
            return masks, rate
        with torch.no_grad():
            _, mask, rate = self.forward(torch.split(rm, lens), lens)
            masks = [mask]
            for _ in range(1, n_levels):
                masks.append(F.max_pool2d(masks[-1], kernel_size=2))
        return masks, rate
