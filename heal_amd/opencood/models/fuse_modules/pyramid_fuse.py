"""PyramidFusion (reference: opencood/models/fuse_modules/pyramid_fuse.py:65-168) on top of the
fused warp + occupancy-softmax kernel K5 (heal_warp_fuse)."""
import functools

import torch
import torch.nn as nn

from heal_amd import derived, ops, switches
from heal_amd.opencood.models.sub_modules.bev_blocks import (Bottleneck, ResNetBEVBackbone, ResNetModified)


def crop_window(H, W, ratio_h, ratio_w):
    """pyramid_fuse.py:151-158: centre window of a camera agent's map whose score is kept."""
    crop_H = H / ratio_h - 4
    crop_W = W / ratio_w - 4
    return (int(H // 2 - crop_H // 2), int(H // 2 + crop_H // 2),
            int(W // 2 - crop_W // 2), int(W // 2 + crop_W // 2))


def weighted_fuse_autograd(x, occ, record_len, affine_matrix, crops=None):
    """Gradient path of pyramid_fuse.py:17-63,139-160 with torch operators: score = sigmoid(occ) + 1e-4 (times the camera
    crop mask when one is given), features and scores of every agent sampled bilinearly in the ego frame (zeros outside),
    softmax over the agents with never-observed positions (score exactly 0) left out, weighted sum."""
    import torch.nn.functional as F
    score = torch.sigmoid(occ) + 1e-4
    if crops is not None:
        keep = torch.ones_like(score)
        for a, c in enumerate(crops):
            if c is not None:
                keep[a] = 0
                keep[a, :, c[0]:c[1], c[2]:c[3]] = 1
        score = score * keep
    out, start = [], 0
    for b, n in enumerate(record_len):
        M = torch.as_tensor(affine_matrix[b][0, :n], dtype=x.dtype, device=x.device)
        xs, ss = x[start:start + n], score[start:start + n]
        grid = F.affine_grid(M, list(xs.shape), align_corners=False)
        feat = F.grid_sample(xs, grid, align_corners=False)
        sc = F.grid_sample(ss, F.affine_grid(M, list(ss.shape), align_corners=False), align_corners=False)
        sc = sc.masked_fill(sc == 0, float("-inf")).softmax(dim=0)
        sc = torch.where(torch.isnan(sc), torch.zeros_like(sc), sc)
        out.append((feat * sc).sum(0))
        start += n
    return torch.stack(out)


class _WarpFuse(torch.autograd.Function):
    """K5 with a hand-written backward: forward = heal_warp_fuse, backward = heal_warp_fuse_backward (one thread per ego pixel
    re-samples every agent, scatters the map gradient through the bilinear taps and pushes the softmax gradient back to the
    occupancy logits).  The warped [n,C,H,W] stack of the reference's autograd is never stored."""

    @staticmethod
    def forward(ctx, x, occ, rows, grid_f64, crop):
        x, occ = x.contiguous(), occ.contiguous()
        ctx.save_for_backward(x, occ)
        ctx.args = (rows, grid_f64, crop)
        return ops.warp_fuse(x, occ, rows, grid_f64, crop)

    @staticmethod
    def backward(ctx, grad_out):
        x, occ = ctx.saved_tensors
        rows, grid_f64, crop = ctx.args
        g_x, g_occ = ops.warp_fuse_backward(x, occ, rows, grad_out.contiguous(), grid_f64, crop)
        return g_x, g_occ, None, None, None


def weighted_fuse(x, occ, record_len, affine_matrix, grid_f64=True, crops=None):
    """pyramid_fuse.py:17-63 with the score construction folded in.

    x [sum(n),C,H,W]; occ [sum(n),1,H,W] occupancy LOGITS; record_len: list of ints;
    affine_matrix: host numpy [B,L,L,2,3]; crops: per-agent (h0,h1,w0,w1) or None."""
    grad = torch.is_grad_enabled() and (x.requires_grad or occ.requires_grad)
    if grad and not (x.is_cuda and switches.on("HEAL_K5_BACKWARD")):
        return weighted_fuse_autograd(x, occ, record_len, affine_matrix, crops)   # any device: torch operators
    out = []
    start = 0
    for b, n in enumerate(record_len):
        rows = affine_matrix[b][0, :n]
        crop = None
        if crops is not None:
            crop = [crops[start + a] if crops[start + a] is not None else (0, 0, 0, 0) for a in range(n)]
        if grad:   # training on the device: the HIP kernels in both directions
            out.append(_WarpFuse.apply(x[start:start + n], occ[start:start + n], rows, grid_f64, crop))
        else:
            out.append(ops.warp_fuse(x[start:start + n], occ[start:start + n], rows, grid_f64, crop))
        start += n
    return out[0].unsqueeze(0) if len(out) == 1 else torch.stack(out)   # (one scene: no copy)


def _stage_influence(lo, hi, layer, size_in):
    """[lo, hi) of the stage INPUT that differs from the all-zero input -> ([lo', hi') of the stage output that can differ from the
    zero-input output, output size).  Every Bottleneck is 1x1 -> 3x3 (stride s, padding 1) -> 1x1 (+ a 1x1 stride-s downsample):
    output o reads inputs s o - 1 .. s o + 1."""
    size = size_in
    for blk in layer:
        s_ = blk.stride
        size = (size - 1) // s_ + 1
        lo = max(0, -((1 - lo) // s_))         # ceil((lo - 1) / s)
        hi = min(size, hi // s_ + 1)           # floor((hi - 1 + 1) / s) + 1, exclusive
    return lo, hi, size


def _stage_needs(olo, ohi, layer, size_in):
    """[olo, ohi) of the stage OUTPUT -> the [ilo, ihi) of its INPUT those outputs read (the receptive field, clipped to the map)."""
    for blk in reversed(list(layer)):
        s_ = blk.stride
        olo, ohi = s_ * olo - 1, s_ * (ohi - 1) + 2
    return max(0, olo), min(size_in, ohi)


def k5_read_box(H, W, window):
    """The box (y0, y1, x0, x1) of a camera agent's H x W map that K5 reads when the agent's score is kept on `window` (crop_window):
    the window's bilinear ring, clipped to the map, the columns rounded out to 16 bytes (heal_warp_fuse_levels_src's box rule)."""
    wy0, wy1, wx0, wx1 = window
    return max(0, wy0 - 1), min(H, wy1 + 1), max(0, wx0 - 1) // 4 * 4, min(W, -(-(wx1 + 1) // 4) * 4)


@functools.lru_cache(maxsize=None)
def stage_roi_plan(box, strides, H, W):
    """Region-of-interest plan of ONE image through one stage of Bottlenecks (1x1 -> 3x3 stride s, padding 1 -> 1x1, + identity; the
    first block's identity may be a 1x1 stride-s downsample): box = (y0, y1, x0, x1) of the stage OUTPUT that somebody reads,
    strides = the blocks' strides, H x W the stage input ->
        (per block {"conv1", "conv2", "conv3", "downsample"} -> the box of that convolution's OUTPUT that is needed,
         the box of the stage INPUT that is read).
    Backwards, the interval arithmetic of _stage_needs one block at a time: conv3, conv2 and the downsample are needed on the block's
    output need O (conv3 is pointwise and adds the identity at the same pixel); conv1 (pointwise, at the block's input resolution)
    on what the 3x3 reads for O: rows s lo - 1 .. s (hi - 1) + 1, clipped to the map; the block's input is read there too (the
    identity's pixels, s O, lie inside), and that is the previous block's output need.  Pure function of shapes and configuration:
    cached.  An empty box gives empty needs."""
    y0, y1, x0, x1 = (int(v) for v in box)
    sizes = [(int(H), int(W))]
    for s_ in strides:
        sizes.append(((sizes[-1][0] - 1) // s_ + 1, (sizes[-1][1] - 1) // s_ + 1))
    if not (0 <= y0 <= y1 <= sizes[-1][0] and 0 <= x0 <= x1 <= sizes[-1][1]):
        raise ValueError(f"stage_roi_plan: box {box} outside the {sizes[-1][0]} x {sizes[-1][1]} stage output")
    blocks = []
    for j in reversed(range(len(strides))):
        s_, (hi_, wi_) = strides[j], sizes[j]
        out = (y0, y1, x0, x1)
        if y1 > y0 and x1 > x0:
            y0, y1, x0, x1 = max(0, s_ * y0 - 1), min(hi_, s_ * (y1 - 1) + 2), max(0, s_ * x0 - 1), min(wi_, s_ * (x1 - 1) + 2)
        else:
            y0 = y1 = x0 = x1 = 0
        blocks.append({"conv1": (y0, y1, x0, x1), "conv2": out, "conv3": out, "downsample": out})
    return tuple(reversed(blocks)), (y0, y1, x0, x1)


def box_union(a, b):
    """Bounding box of two (y0, y1, x0, x1) boxes; None stands for "nothing"."""
    if a is None or b is None:
        return a if b is None else b
    return min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3])


class PyramidFusion(ResNetBEVBackbone):
    def __init__(self, model_cfg, input_channels=64):
        super().__init__(model_cfg, input_channels)
        if model_cfg["resnext"]:
            # ResNeXt stages: 32 groups, width 4 per group, Bottleneck with expansion 1
            self.resnet = ResNetModified(Bottleneck, model_cfg["layer_nums"], model_cfg["layer_strides"],
                                         model_cfg["num_filters"], inplanes=model_cfg.get("inplanes", 64),
                                         groups=32, width_per_group=4, expansion=1)
        self.align_corners = model_cfg.get("align_corners", False)
        if self.align_corners:
            raise NotImplementedError("align_corners=True fusion is not used by any HEAL config")
        for i in range(self.num_levels):
            setattr(self, f"single_head_{i}", nn.Conv2d(model_cfg["num_filters"][i], 1, kernel_size=1))

    def occupancy_head(self, i, feature):
        """single_head_i (pyramid_fuse.py:89-91): a one-output 1x1 convolution = a channel dot product (heal_channel_dot)."""
        head = getattr(self, f"single_head_{i}")
        if not torch.is_grad_enabled() and ops.channel_dot_supported(feature):
            return ops.channel_dot(feature, head.weight, head.bias)
        return head(feature)

    def forward_single(self, spatial_features):
        feature_list = self.get_multiscale_feature(spatial_features)
        occ_map_list = [self.occupancy_head(i, feature_list[i]) for i in range(self.num_levels)]
        return self.decode_multiscale_feature(feature_list), occ_map_list

    # ---- camera agents: their padded maps are ZERO outside the centre box (round 6) ------------------------------------------------
    # The camera modalities' BEV maps cover the camera grid (+-51.2 m) and are zero-padded to the LiDAR range before the fusion
    # pyramid (heter_pyramid_collab.py:153-167, torchvision CenterCrop: 128^2 -> 256^2), so 75 % of a camera agent's pyramid input is
    # exactly zero -- and the reference still pushes it through every ResNeXt block (pyramid_fuse.py:71-79,139).  A convolution stack
    # is local: an output pixel whose receptive field holds only zero input equals the stack's output for an ALL-ZERO map at that
    # position.  So for the camera agents each stage runs on a CROP (the box its content can influence + the receptive-field halo,
    # aligned to 8 pixels) and the rest of the stage output is the zero-input response `BG`, computed once per weight version
    # (a frame-independent constant).  Exact: the pasted box is computed by the same kernels from the same values; only work whose
    # result is known in advance is skipped.  Level 0: 144^2 of 256^2 pixels, level 1: 88^2 of 128^2; the last level's content box
    # already reaches the borders and runs in full.  HEAL_PYRAMID_CAMCROP=0 switches it off.
    def _zero_response_slot(self, like):
        """(tag, sources, extra) of the zero response in heal_amd.derived: every parameter and buffer of the pyramid, the map size."""
        return "pyramid_zero_response", [*self.resnet.parameters(), *self.resnet.buffers()], (tuple(like.shape[1:]), str(like.device))

    def _zero_response(self, like):
        """Stage outputs of the pyramid for an all-zero [1, C, H, W] input."""
        def build():
            z = torch.zeros((1,) + tuple(like.shape[1:]), dtype=like.dtype, device=like.device)
            return [f.clone() for f in self.resnet(z)]
        tag, sources, extra = self._zero_response_slot(like)
        return derived.derived(tag, sources, build, extra)

    def _camcrop_plan(self, x, cam_slice, box):
        """Per stage: None (run the stage in full) or (crop of the stage input (y0, y1, x0, x1), output box to paste (global), the same
        box in the crop's output coordinates).  box = (y0, y1, x0, x1) of the non-zero region of the camera agents' input."""
        H, W = int(x.shape[2]), int(x.shape[3])
        ly, hy, lx, hx = box
        plan = []
        for i in range(self.layernum_):
            layer = getattr(self.resnet, f"layer{i}")
            s_tot = 1
            for blk in layer:
                s_tot *= blk.stride
            oly, ohy, Ho = _stage_influence(ly, hy, layer, H)
            olx, ohx, Wo = _stage_influence(lx, hx, layer, W)
            iy0, iy1 = _stage_needs(oly, ohy, layer, H)
            ix0, ix1 = _stage_needs(olx, ohx, layer, W)
            a = 8 * s_tot                      # crop origin / size: multiples of 8 output pixels (kernel tile and 16-B row constraints)
            cy0, cy1, cx0, cx1 = iy0 // a * a, min(H, -(-iy1 // a) * a), ix0 // a * a, min(W, -(-ix1 // a) * a)
            if (cy1 - cy0) * (cx1 - cx0) > 0.7 * H * W:
                plan.append(None)              # the content reaches (nearly) everywhere: no saving in cropping this stage
            else:
                plan.append(((cy0, cy1, cx0, cx1), (oly, ohy, olx, ohx),
                             (oly - cy0 // s_tot, ohy - cy0 // s_tot, olx - cx0 // s_tot, ohx - cx0 // s_tot)))
            ly, hy, lx, hx, H, W = oly, ohy, olx, ohx, Ho, Wo
        return plan

    def get_multiscale_feature_camcrop(self, x, cam_slice, box):
        """get_multiscale_feature for a scene whose agents [cam_slice] are camera agents with non-zero input inside `box` only (and
        whose other agents form ONE contiguous range)."""
        n = int(x.shape[0])
        c0, c1 = cam_slice
        other = (0, c0) if c0 > 0 else (c1, n)
        bg = self._zero_response(x)
        plan = self._camcrop_plan(x, cam_slice, box)
        feats = []
        for i in range(self.layernum_):
            layer = getattr(self.resnet, f"layer{i}")
            if plan[i] is None:
                x = self.resnet.run_stage(layer, x)
                feats.append(x)
                continue
            (cy0, cy1, cx0, cx1), (gy0, gy1, gx0, gx1), (py0, py1, px0, px1) = plan[i]
            full = torch.empty((n,) + tuple(bg[i].shape[1:]), dtype=x.dtype, device=x.device)
            if other[1] > other[0]:            # the LiDAR agents: the whole map, written straight into their slice
                xa = x[other[0]:other[1]]
                for j, blk in enumerate(layer):
                    xa = blk(xa, out=full[other[0]:other[1]]) if j == len(layer) - 1 else blk(xa)
            yc = layer(x[c0:c1, :, cy0:cy1, cx0:cx1].contiguous())
            full[c0:c1] = bg[i]                # (broadcast copy) the zero-input response everywhere ...
            full[c0:c1, :, gy0:gy1, gx0:gx1] = yc[:, :, py0:py1, px0:px1]   # ... and the box the content reaches
            x = full
            feats.append(x)
        return feats

    @property
    def layernum_(self):
        return self.resnet.layernum

    def _camcrop_args(self, spatial_features, agent_modality_list, cam_boxes):
        """(cam_slice, box) when the camera-crop walk applies: inference on a HIP device, ResNeXt stages, the camera agents form one
        contiguous range at an end of the scene and share one valid box."""
        if (not cam_boxes or agent_modality_list is None or torch.is_grad_enabled() or not spatial_features.is_cuda
                or not switches.on("HEAL_PYRAMID_CAMCROP")):
            return None
        cams = [k for k, m in enumerate(agent_modality_list) if m in cam_boxes]
        n = len(agent_modality_list)
        if not cams or cams != list(range(cams[0], cams[-1] + 1)) or (cams[0] != 0 and cams[-1] != n - 1):
            return None
        from heal_amd.opencood.models.sub_modules.bev_blocks import Bottleneck
        if not all(isinstance(b, Bottleneck) and b.conv2.kernel_size == (3, 3) and b.conv2.padding == (1, 1)
                   for i in range(self.layernum_) for b in getattr(self.resnet, f"layer{i}")):
            return None
        boxes = [cam_boxes[agent_modality_list[k]] for k in cams]
        box = (min(b[0] for b in boxes), max(b[1] for b in boxes), min(b[2] for b in boxes), max(b[3] for b in boxes))
        H, W = int(spatial_features.shape[2]), int(spatial_features.shape[3])
        if H % 32 or W % 32 or not (0 <= box[0] < box[1] <= H and 0 <= box[2] < box[3] <= W):
            return None
        if derived.capturing() and not derived.ready(*self._zero_response_slot(spatial_features)):
            return None     # the zero response would be computed INSIDE the capture (valid only after a replay): plain walk for this graph
        return (cams[0], cams[-1] + 1), box

    def multiscale(self, spatial_features, agent_modality_list=None, cam_boxes=None):
        """get_multiscale_feature, by the camera-crop walk where it applies (cam_boxes: see forward_collab)."""
        cc = self._camcrop_args(spatial_features, agent_modality_list, cam_boxes)
        if cc is not None:
            return self.get_multiscale_feature_camcrop(spatial_features, *cc)
        return self.get_multiscale_feature(spatial_features)

    # ---- lean inference walk: every agent's map is fused from where its stage left it -------------------------------------------------
    # The camera-crop walk above still receives a STACK of the agents' maps, with the camera maps zero-padded to the LiDAR range, and
    # rebuilds a full-size stack after stage 0 (crop copy, zero-response broadcast, paste) -- although K5 multiplies everything outside a
    # camera agent's crop window by a score of exactly zero.  Here the caller hands over the LiDAR agents' tensor and the camera agents'
    # UNPADDED maps; stage 0 runs on the LiDAR tensor as it is and on the camera crop (content + halo), and K5 reads both results in place
    # (ops.warp_fuse_levels_src: per agent a pointer, strides and the box its map is defined on).  Stage 1's camera input is the cached
    # zero response PRE-CROPPED to that stage's input crop with the valid stage-0 box pasted in.  From stage 1 on the assembly is the
    # camera-crop walk's (the last stage runs on all agents in one launch).  Same kernels on the same values as the camera-crop walk.
    def _zero_response_crop(self, like, level, crop):
        """The zero-input response of stage `level` on crop = (y0, y1, x0, x1), contiguous [1, C, h, w]."""
        tag, sources, extra = self._zero_response_slot(like)
        return "pyramid_zero_response_crop", sources, extra + (int(level), tuple(int(v) for v in crop))

    @staticmethod
    def _cam_window(H, W, mod, cam_crop_info):
        return crop_window(H, W, cam_crop_info[mod][f"crop_ratio_H_{mod}"], cam_crop_info[mod][f"crop_ratio_W_{mod}"])

    # ---- regions of interest: stages that run "in full" skip the tiles of the camera agents' maps that nobody reads -------------------
    # A stage the crop plan leaves alone (plan[i] is None: the last level, whose content box reaches the border) runs on the full maps
    # of all agents in one launch per convolution.  K5 reads a camera agent's map of that level only on the crop window's bilinear
    # ring (k5_read_box) and multiplies everything else by a score of exactly zero, so going backwards through the blocks each
    # convolution's output is needed on a known box (stage_roi_plan) -- and the kernels skip the 64-pixel / 8 x 32 tiles outside it
    # (ops.conv1x1 / ops.grouped_conv3x3 with `roi`: same buffers, same single launch over all agents, blocks that leave early).  LiDAR
    # agents get the full image.  Outside the boxes the stage output is UNINITIALISED memory: no needed pixel reads it (the plan is
    # exactly the receptive field), the occupancy head may (its result is sliced to the K5 box afterwards).
    # HEAL_PYRAMID_ROI=0 (ops.pyramid_roi_enabled) restores the walk without ROIs.
    def lean_roi_plan(self, shape, plan, c0, c1, agent_modality_list, cam_crop_info):
        """{stage index: ResNetModified.run_stage's `roi`} for the stages forward_collab_lean runs in full (plan[i] is None, i >= 1),
        {} when ROIs are off.  shape: (H, W) of the pyramid input.  Last stage first: a stage's output need is the box K5 reads at
        its level, united with what the NEXT stage reads of it (its input need when that stage runs by ROI too, its input crop when
        it is cropped)."""
        if not ops.pyramid_roi_enabled():
            return {}
        n = len(agent_modality_list)
        sizes = [tuple(int(v) for v in shape)]
        for i in range(self.layernum_):
            h, w = sizes[-1]
            for blk in getattr(self.resnet, f"layer{i}"):
                h, w = (h - 1) // blk.stride + 1, (w - 1) // blk.stride + 1
            sizes.append((h, w))
        rois, next_need = {}, [None] * n        # next_need[k]: box of THIS stage's output the following stage reads for agent k
        for i in reversed(range(1, self.layernum_)):
            (hi_, wi_), (ho, wo) = sizes[i], sizes[i + 1]
            if plan[i] is not None:
                next_need = [tuple(plan[i][0]) if c0 <= k < c1 else (0, hi_, 0, wi_) for k in range(n)]
                continue
            strides = tuple(int(blk.stride) for blk in getattr(self.resnet, f"layer{i}"))
            per_agent, needs_in = [], []
            for k in range(n):
                if c0 <= k < c1:
                    box = box_union(k5_read_box(ho, wo, self._cam_window(ho, wo, agent_modality_list[k], cam_crop_info)), next_need[k])
                else:
                    box = (0, ho, 0, wo)
                blocks, need_in = stage_roi_plan(box, strides, hi_, wi_)
                per_agent.append(blocks)
                needs_in.append(need_in)
            rois[i] = [{name: [per_agent[k][j][name] for k in range(n)] for name in ("conv1", "conv2", "conv3", "downsample")}
                       for j in range(len(strides))]
            next_need = needs_in
        return rois

    def lean_plan(self, like, record_len, agent_modality_list, cam_boxes, cam_crop_info):
        """What forward_collab_lean needs, or None when the lean walk does not apply: one scene of at most 8 agents at inference, the
        conditions of the camera-crop walk (_camcrop_args), a crop window for every camera agent, a cropped stage 0, the other agents
        of ONE modality (their encoder's output is then the LiDAR tensor in scene order), cached responses ready under capture.
        like: a [k, C, H, W] tensor of the full map size on the model's device (k may be 0)."""
        if (len(record_len) != 1 or not 1 <= self.num_levels <= ops.WARP_MAX_LEVELS or int(record_len[0]) > ops.WARP_MAX_AGENTS
                or self.training or not switches.on("HEAL_K5_LEVELS") or not switches.on("HEAL_PYRAMID_LEAN")):
            return None
        cc = self._camcrop_args(like, agent_modality_list, cam_boxes)
        if cc is None:
            return None
        (c0, c1), box = cc
        n = len(agent_modality_list)
        other = (0, c0) if c0 > 0 else (c1, n)
        if not cam_crop_info or any(agent_modality_list[k] not in cam_crop_info for k in range(c0, c1)):
            return None
        if len({agent_modality_list[k] for k in range(*other)}) > 1:
            return None
        plan = self._camcrop_plan(like, (c0, c1), box)
        if plan[0] is None:
            return None
        H, W = int(like.shape[2]), int(like.shape[3])
        gbox = plan[0][1]
        for k in range(c0, c1):     # K5 reads a camera agent's stage-0 crop on its valid box: the window's bilinear ring must lie inside
            wy0, wy1, wx0, wx1 = self._cam_window(H, W, agent_modality_list[k], cam_crop_info)
            if not (gbox[0] <= max(0, wy0 - 1) and min(H, wy1 + 1) <= gbox[1] and gbox[2] <= max(0, wx0 - 1) and min(W, wx1 + 1) <= gbox[3]):
                return None
        if self.layernum_ > 1 and plan[1] is not None:
            slot = self._zero_response_crop(like, 0, plan[1][0])
            if derived.capturing() and not derived.ready(slot[0], slot[1], slot[2]):
                return None
        return (c0, c1), other, plan

    def forward_collab_lean(self, lidar, cam_maps, like, lean, affine_matrix, agent_modality_list, cam_crop_info, cam_boxes,
                            grid_f64=True):
        """forward_collab of one scene by the lean walk.  lidar: [n_l, C, H, W] (the non-camera agents in scene order) or None;
        cam_maps: the camera agents' unpadded [C, h, w] maps in scene order; lean: lean_plan's result -> fused feature (no occupancy
        list: the full-size occupancy maps of the camera agents are never formed)."""
        (c0, c1), other, plan = lean
        n, nc, nl = len(agent_modality_list), c1 - c0, other[1] - other[0]
        bg = self._zero_response(like)
        dt, dev = like.dtype, like.device
        # stage 0: the camera agents enter as the stage's input crop (their content inside a zero halo)
        (cy0, cy1, cx0, cx1), gbox, pbox = plan[0]
        layer = self.resnet.layer0
        xc = torch.zeros((nc, int(like.shape[1]), cy1 - cy0, cx1 - cx0), dtype=dt, device=dev)
        for j, m in enumerate(cam_maps):
            b = cam_boxes[agent_modality_list[c0 + j]]
            xc[j, :, b[0] - cy0:b[1] - cy0, b[2] - cx0:b[3] - cx0] = m
        yc = layer(xc)
        full, xl = None, None
        if self.layernum_ > 1 and plan[1] is None:      # the next stage runs on the full maps of all agents: assemble them
            full = torch.empty((n,) + tuple(bg[0].shape[1:]), dtype=dt, device=dev)
            full[c0:c1] = bg[0]
            full[c0:c1, :, gbox[0]:gbox[1], gbox[2]:gbox[3]] = yc[:, :, pbox[0]:pbox[1], pbox[2]:pbox[3]]
        if nl:
            xl = lidar
            for j, blk in enumerate(layer):
                xl = blk(xl, out=full[other[0]:other[1]]) if (full is not None and j == len(layer) - 1) else blk(xl)
        sources, shapes = [], []
        occ_c = self.occupancy_head(0, yc)
        occ_l = self.occupancy_head(0, xl) if nl else None
        level = [None] * n
        for j in range(nl):
            level[other[0] + j] = (xl[j], occ_l[j, 0], (0, 0))
        for j in range(nc):
            level[c0 + j] = (yc[j, :, pbox[0]:pbox[1], pbox[2]:pbox[3]], occ_c[j, 0, pbox[0]:pbox[1], pbox[2]:pbox[3]],
                             (gbox[0], gbox[2]))
        sources.append(level)
        shapes.append(tuple(int(v) for v in bg[0].shape[2:]))
        rois = self.lean_roi_plan(like.shape[2:], plan, c0, c1, agent_modality_list, cam_crop_info)
        for i in range(1, self.layernum_):
            layer = getattr(self.resnet, f"layer{i}")
            if plan[i] is None:
                full = self.resnet.run_stage(layer, full, roi=rois.get(i))
            else:
                (cy0, cy1, cx0, cx1), g2, p2 = plan[i]
                nxt = torch.empty((n,) + tuple(bg[i].shape[1:]), dtype=dt, device=dev)
                if nl:
                    xa = full[other[0]:other[1]] if full is not None else xl
                    for j, blk in enumerate(layer):
                        xa = blk(xa, out=nxt[other[0]:other[1]]) if j == len(layer) - 1 else blk(xa)
                if full is not None:
                    xin = full[c0:c1, :, cy0:cy1, cx0:cx1].contiguous()
                else:       # the cached zero response on this stage's input crop + the valid box of the previous stage's crop
                    crop = (cy0, cy1, cx0, cx1)
                    tag, src, extra = self._zero_response_crop(like, i - 1, crop)
                    bgc = derived.derived(tag, src, lambda: bg[i - 1][:, :, cy0:cy1, cx0:cx1].contiguous(), extra)
                    xin = bgc.repeat(nc, 1, 1, 1)
                    iy0, iy1, ix0, ix1 = max(gbox[0], cy0), min(gbox[1], cy1), max(gbox[2], cx0), min(gbox[3], cx1)
                    xin[:, :, iy0 - cy0:iy1 - cy0, ix0 - cx0:ix1 - cx0] = yc[:, :, pbox[0] + iy0 - gbox[0]:pbox[0] + iy1 - gbox[0],
                                                                             pbox[2] + ix0 - gbox[2]:pbox[2] + ix1 - gbox[2]]
                yc = layer(xin)
                nxt[c0:c1] = bg[i]
                nxt[c0:c1, :, g2[0]:g2[1], g2[2]:g2[3]] = yc[:, :, p2[0]:p2[1], p2[2]:p2[3]]
                gbox, pbox, full = g2, p2, nxt
            occ = self.occupancy_head(i, full)
            H, W = int(full.shape[2]), int(full.shape[3])
            level = []
            for k in range(n):
                y0, y1, x0, x1 = 0, H, 0, W
                if c0 <= k < c1:
                    # the stack holds the camera agents' whole map; K5 needs it on the crop window's bilinear ring only (columns
                    # rounded out to 16 bytes): its staging is clipped to that box
                    y0, y1, x0, x1 = k5_read_box(H, W, self._cam_window(H, W, agent_modality_list[k], cam_crop_info))
                level.append((full[k, :, y0:y1, x0:x1], occ[k, 0, y0:y1, x0:x1], (y0, x0)))
            sources.append(level)
            shapes.append((H, W))
        crops_all = []
        for (H, W) in shapes:
            crops_all.append([self._cam_window(H, W, mod, cam_crop_info) if mod in cam_crop_info else None for mod in agent_modality_list])
        fused = ops.warp_fuse_levels_src(sources, shapes, affine_matrix[0][0, :n], grid_f64, crops_all)
        return self.decode_multiscale_feature([f.unsqueeze(0) for f in fused])

    def forward_collab(self, spatial_features, record_len, affine_matrix, agent_modality_list=None,
                       cam_crop_info=None, grid_f64=True, cam_boxes=None):
        """affine_matrix: host numpy [B,L,L,2,3] (normalize_pairwise_tfm of the host pairwise matrix);
        record_len: list of ints.  cam_boxes: {modality: (y0, y1, x0, x1)} -- the caller's promise that the maps of those (camera)
        modalities are exactly zero outside the box (it zero-padded them itself): enables the camera-crop stage walk."""
        feature_list = self.multiscale(spatial_features, agent_modality_list, cam_boxes if len(record_len) == 1 else None)
        use_crop = bool(cam_crop_info) and not self.training
        fused_feature_list, occ_map_list = [], []
        if (len(record_len) == 1 and not torch.is_grad_enabled() and feature_list[0].is_cuda
                and 1 <= self.num_levels <= ops.WARP_MAX_LEVELS and int(record_len[0]) <= ops.WARP_MAX_AGENTS and switches.on("HEAL_K5_LEVELS")):
            # inference, one scene: the three levels are independent once the stages ran -> ONE K5 launch for all of them
            # (heal_warp_fuse_levels; HEAL_K5_LEVELS=0 keeps one heal_warp_fuse launch per level for A/B)
            n = int(record_len[0])
            crops_all = []
            for i in range(self.num_levels):
                occ_map_list.append(self.occupancy_head(i, feature_list[i]))
                crops = None
                if use_crop:
                    _, _, H, W = occ_map_list[i].shape
                    crops = [crop_window(H, W, cam_crop_info[mod][f"crop_ratio_H_{mod}"], cam_crop_info[mod][f"crop_ratio_W_{mod}"])
                             if mod in cam_crop_info else None for mod in agent_modality_list]
                crops_all.append(crops)
            fused = ops.warp_fuse_levels([f[:n] for f in feature_list], [o[:n] for o in occ_map_list], affine_matrix[0][0, :n],
                                         grid_f64, crops_all if use_crop else None)
            return self.decode_multiscale_feature([f.unsqueeze(0) for f in fused]), occ_map_list
        for i in range(self.num_levels):
            occ_map = self.occupancy_head(i, feature_list[i])
            occ_map_list.append(occ_map)
            crops = None
            if use_crop:
                _, _, H, W = occ_map.shape
                crops = []
                for mod in agent_modality_list:
                    if mod in cam_crop_info:
                        crops.append(crop_window(H, W, cam_crop_info[mod][f"crop_ratio_H_{mod}"],
                                                 cam_crop_info[mod][f"crop_ratio_W_{mod}"]))
                    else:
                        crops.append(None)
            fused_feature_list.append(weighted_fuse(feature_list[i], occ_map, record_len, affine_matrix,
                                                    grid_f64, crops))
        return self.decode_multiscale_feature(fused_feature_list), occ_map_list
