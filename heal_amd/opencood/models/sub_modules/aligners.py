"""The aligners of AlignNet beyond ConvNeXt: resnet1x1, resnet3x3, scaligner, cbam, fanet and sdta.

Parameter names, shapes and registration order follow the reference, so that its checkpoints load unchanged and `state_dict()`
lists its keys in its order: opencood/models/sub_modules/feature_alignnet_modules.py:33-293, 368-505 and cbam.py:31-98.

Every module follows ConvNeXtBlock.forward's rule.  On a device tensor outside the gradient path (`grad_path` false) and with
HEAL_ALIGN_FUSED on it runs on this library's operators: Conv + BatchNorm folded (heal_amd.derived), pointwise convolutions and
Linear layers on heal_conv1x1 with their bias / activation / residual fused, channel LayerNorm in one NCHW pass, and for SDTA the
cross-covariance attention folded into one pointwise weight per image (ops.xca_weights, include/heal_amd_align.h).  On CPU tensors,
under autograd, with BatchNorm in training mode, for a shape an operator's `_supported` predicate refuses, or with
HEAL_ALIGN_FUSED=0, it runs the reference's composition line by line on the same parameters.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from heal_amd.derived import derived
from heal_amd.opencood.models.sub_modules.bev_blocks import ConvBN, ConvNeXtBlock, LayerNorm, grad_path


def _fused(x, *modules):
    """True where the module may run on the library's operators (see the module docstring)."""
    from heal_amd import ops
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not grad_path(x, *modules) and ops.align_fused_enabled()


def _pointwise(x, conv, act=0, residual=None):
    """A 1x1 nn.Conv2d (+ ReLU for act 1) outside the gradient path: heal_conv1x1 where it takes the shape, torch otherwise."""
    from heal_amd import ops
    if ops.conv1x1_supported(conv.in_channels, conv.out_channels, int(x.shape[2] * x.shape[3])):
        return ops.conv1x1(x, conv.weight, conv.bias, residual, act)
    y = conv(x)
    if residual is not None:
        y = y + residual
    return F.relu(y) if act == 1 else y


# ---- resnet1x1 / resnet3x3 -------------------------------------------------------------------------------------------------------------
class ResidualBlock(nn.Module):
    """feature_alignnet_modules.py:368-401 (deform=False, use_1x1conv=False)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, deform=False):
        super().__init__()
        if kernel_size not in (1, 3):
            raise ValueError("ResidualBlock: kernel_size must be 1 or 3")
        if deform:
            raise NotImplementedError("deformable residual aligner is out of scope (needs mmcv)")
        padding = kernel_size // 2
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=1)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=kernel_size, padding=padding)
        self.conv3 = None
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.bn2 = nn.BatchNorm2d(out_channels)

    def forward(self, X):
        from heal_amd import ops
        if (_fused(X, self) and (self.conv1.kernel_size == (3, 3) or ops.conv1x1_supported(
                self.conv1.in_channels, self.conv1.out_channels, int(X.shape[2] * X.shape[3])))):
            # BatchNorm folded into both convolutions; residual and ReLU in the epilogue of the second
            Y = ConvBN.run(X, self.conv1, self.bn1, relu=True)
            return ConvBN.run(Y, self.conv2, self.bn2, relu=True, residual=X)
        Y = F.relu(self.bn1(self.conv1(X)))
        Y = self.bn2(self.conv2(Y))
        return F.relu(Y + X)


class _ResAligner(nn.Module):
    kernel_size = None

    def __init__(self, args):
        super().__init__()
        dim, deform = args["dim"], args.get("deform", False)
        self.model = nn.Sequential(*[ResidualBlock(dim, dim, kernel_size=self.kernel_size, deform=deform)
                                     for _ in range(args["num_of_blocks"])])

    def forward(self, x):
        return self.model(x)


class Res1x1Aligner(_ResAligner):
    """feature_alignnet_modules.py:404-417."""
    kernel_size = 1


class Res3x3Aligner(_ResAligner):
    """feature_alignnet_modules.py:419-432."""
    kernel_size = 3


# ---- scaligner ---------------------------------------------------------------------------------------------------------------------------
class ResMLP(nn.Module):
    """feature_alignnet_modules.py:453-463: x + (LayerNorm -> (Linear -> GELU) x n)(x) on channels-last tokens."""

    def __init__(self, num_of_layers=2, dim=64):
        super().__init__()
        model_list = [nn.LayerNorm(dim)]
        for _ in range(num_of_layers):
            model_list.append(nn.Linear(dim, dim))
            model_list.append(nn.GELU())
        self.model = nn.Sequential(*model_list)

    def forward(self, x):
        return x + self.model(x)

    def forward_nchw(self, x):
        """The same on an NCHW map with the library's operators: one LayerNorm pass, each Linear + GELU one pointwise convolution.
        heal_conv1x1 adds its residual BEFORE the activation, so the skip (which the block adds after the last GELU) is one
        in-place addition on the last layer's result, not that layer's residual argument."""
        from heal_amd import ops
        ln = self.model[0]
        h = ops.layernorm_nchw(x, ln.weight, ln.bias, ln.eps)
        for m in self.model[1:]:
            if isinstance(m, nn.Linear):
                h = ops.conv1x1(h, m.weight[:, :, None, None], m.bias, None, 3)
        return h.add_(x)


class SCAligner(nn.Module):
    """feature_alignnet_modules.py:465-505."""

    def __init__(self, args):
        super().__init__()
        self.backbone = nn.Sequential(*[ResMLP(args["num_of_layers"], args["dim"]) for _ in range(args["num_of_blocks"])])

    def forward(self, x):
        from heal_amd import ops
        if (_fused(x, self)
                and ops.conv1x1_supported(x.shape[1], x.shape[1], int(x.shape[2] * x.shape[3]))):
            for block in self.backbone:          # NCHW throughout: the two permutes of the reference disappear
                x = block.forward_nchw(x)
            return x
        x = x.permute(0, 2, 3, 1)
        x = self.backbone(x)
        return x.permute(0, 3, 1, 2)


# ---- cbam --------------------------------------------------------------------------------------------------------------------------------
class ChannelAttention(nn.Module):
    """cbam.py:31-46 (the reduction is fixed at 16 whatever `ratio` says)."""

    def __init__(self, in_planes, ratio=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.fc = nn.Sequential(nn.Conv2d(in_planes, in_planes // 16, 1, bias=False), nn.ReLU(),
                                nn.Conv2d(in_planes // 16, in_planes, 1, bias=False))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return self.sigmoid(self.fc(self.avg_pool(x)) + self.fc(self.max_pool(x)))


class SpatialAttention(nn.Module):
    """cbam.py:48-60."""

    def __init__(self, kernel_size=7):
        super().__init__()
        self.conv1 = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        avg_out = torch.mean(x, dim=1, keepdim=True)
        max_out, _ = torch.max(x, dim=1, keepdim=True)
        return self.sigmoid(self.conv1(torch.cat([avg_out, max_out], dim=1)))


class CBAMBlock(nn.Module):
    """cbam.py:62-98, BasicBlock with 1x1 convolutions (stride 1, no downsample)."""
    expansion = 1

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.ca = ChannelAttention(planes)
        self.sa = SpatialAttention()
        self.downsample = None
        self.stride = 1

    def forward(self, x):
        from heal_amd import ops
        residual = x
        if _fused(x, self) and ops.conv1x1_supported(x.shape[1], self.conv1.out_channels, int(x.shape[2] * x.shape[3])):
            out = ConvBN.run(x, self.conv1, self.bn1, relu=True)       # the two pointwise convolutions with BatchNorm folded
            out = ConvBN.run(out, self.conv2, self.bn2, relu=False)
        else:
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.bn2(self.conv2(out))
        out = self.ca(out) * out          # channel gate, spatial attention and the tail stay torch operators
        out = self.sa(out) * out
        out = out + residual
        return self.relu(out)


class CBAM(nn.Module):
    """feature_alignnet_modules.py:281-293."""

    def __init__(self, args):
        super().__init__()
        dim = args["dim"]
        self.model = nn.Sequential(*[CBAMBlock(dim, dim) for _ in range(args["num_of_blocks"])])

    def forward(self, x):
        return self.model(x)


# ---- fanet -------------------------------------------------------------------------------------------------------------------------------
class ARNetBlock(nn.Module):
    """feature_alignnet_modules.py:213-225."""

    def __init__(self, indim, outdim):
        super().__init__()
        self.model = nn.Sequential(nn.Conv2d(indim, indim, kernel_size=1), nn.ReLU(),
                                   nn.Conv2d(indim, indim, kernel_size=3, padding=1, groups=8), nn.ReLU(),
                                   nn.Conv2d(indim, outdim, kernel_size=1))

    def forward(self, x):
        from heal_amd import ops
        if not _fused(x, self):
            return self.model(x)
        c0, c1, c2 = self.model[0], self.model[2], self.model[4]
        x = _pointwise(x, c0, act=1)
        C, W = c1.in_channels, int(x.shape[3])
        if C % 16 == 0 and C // 8 in (4, 8, 16) and W % 4 == 0 and int(x.shape[0]) * (C // 16) <= 65535:
            x = ops.grouped_conv3x3(x, c1.weight, c1.bias, 8, 1, True)     # heal_grouped_small_conv3x3's shapes
        else:
            x = F.relu(c1(x))
        return _pointwise(x, c2)


class FALayer(nn.Module):
    """feature_alignnet_modules.py:227-242."""

    def __init__(self, indim, outdim, imgdim):
        super().__init__()
        self.conv1 = nn.Conv2d(imgdim, imgdim, 1)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(imgdim, outdim, 1)
        self.conv3 = nn.Conv2d(imgdim, outdim, 1)
        self.arblock = ARNetBlock(indim, outdim)

    def forward(self, feature, img):
        feature = self.arblock(feature)
        if _fused(img, self):
            inter = _pointwise(img, self.conv1, act=1)
            gamma, beta = _pointwise(inter, self.conv2), _pointwise(inter, self.conv3)
        else:
            inter = self.relu(self.conv1(img))
            gamma, beta = self.conv2(inter), self.conv3(inter)
        return feature * gamma + beta


class FANet(nn.Module):
    """feature_alignnet_modules.py:244-274."""

    def __init__(self, args):
        super().__init__()
        dim = args["dim"]
        self.falayer1 = FALayer(dim, dim, dim)
        self.falayer2 = FALayer(dim, dim * 2, dim)
        self.falayer3 = FALayer(dim * 2, dim * 4, dim)
        self.falayer4 = FALayer(dim * 4, dim * 2, dim)
        self.falayer5 = FALayer(dim * 2, dim, dim)
        self.maxpool = nn.MaxPool2d(2)
        self.upsample2d = nn.Upsample(scale_factor=2, mode="bilinear")
        self.skip_conv1 = nn.Conv2d(dim * 2, dim * 2, 1)
        self.skip_conv2 = nn.Conv2d(dim, dim, 1)

    def _skip(self, conv, x):
        return _pointwise(x, conv) if _fused(x, self) else conv(x)

    def forward(self, x):
        img0 = x.detach()                                    # the "image" branch carries no gradient (the reference's x.detach())
        img1 = self.maxpool(img0)
        img2 = self.maxpool(img1)
        feature0 = self.falayer1(x, img0)
        feature1 = self.falayer2(self.maxpool(feature0), img1)
        feature2 = self.falayer3(self.maxpool(feature1), img2)
        feature3 = self.falayer4(self.upsample2d(feature2), img1) + self._skip(self.skip_conv1, feature1)
        return self.falayer5(self.upsample2d(feature3), img0) + self._skip(self.skip_conv2, feature0)


# ---- sdta --------------------------------------------------------------------------------------------------------------------------------
def _scale_bias(x, conv):
    """A depthwise 1x1 convolution is a per-channel scale and bias."""
    C = conv.out_channels
    return torch.addcmul(conv.bias.view(1, C, 1, 1), x, conv.weight.view(1, C, 1, 1))


class XCA(nn.Module):
    """feature_alignnet_modules.py:33-67 on [B, N, C] tokens (the gradient path; the inference path is SDTAEncoder._fused_forward)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0].transpose(-2, -1), qkv[1].transpose(-2, -1), qkv[2].transpose(-2, -1)
        q = F.normalize(q, dim=-1)
        k = F.normalize(k, dim=-1)
        attn = (q @ k.transpose(-2, -1)) * self.temperature
        attn = self.attn_drop(attn.softmax(dim=-1))
        x = (attn @ v).permute(0, 3, 1, 2).reshape(B, N, C)
        return self.proj_drop(self.proj(x))


class ConvEncoder(ConvNeXtBlock):
    """feature_alignnet_modules.py:74-103 (kernel_size 1, deformable=False): ConvNeXtBlock's attributes with a 1x1 depthwise stem."""

    def __init__(self, dim, layer_scale_init_value=1e-6, expan_ratio=4, kernel_size=1):
        if expan_ratio != 4:
            raise NotImplementedError("ConvEncoder: expan_ratio must be 4")
        super().__init__(dim, layer_scale_init_value=layer_scale_init_value, kernel_size=kernel_size)
        self.drop_path = nn.Identity()

    def forward(self, x):
        from heal_amd import ops
        if (_fused(x, self) and self.dwconv.kernel_size == (1, 1)
                and ops.conv1x1_supported(x.shape[1], 4 * x.shape[1], int(x.shape[2] * x.shape[3]))):
            xn = ops.layernorm_nchw(_scale_bias(x, self.dwconv), self.norm.weight, self.norm.bias, self.norm.eps)
            h = ops.conv1x1(xn, self.pwconv1.weight[:, :, None, None], self.pwconv1.bias, None, 3)
            w2, b2 = self._folded_pw2()
            return ops.conv1x1(h, w2, b2, x, 0)
        inp = x
        x = self.dwconv(x).permute(0, 2, 3, 1)
        x = self.pwconv2(self.act(self.pwconv1(self.norm(x))))
        if self.gamma is not None:
            x = self.gamma * x
        return inp + self.drop_path(x.permute(0, 3, 1, 2))


class SDTAEncoder(nn.Module):
    """feature_alignnet_modules.py:105-160 (deformable=False, no positional embedding, drop rates 0)."""

    def __init__(self, dim, layer_scale_init_value=1e-6, expan_ratio=4, num_heads=4, qkv_bias=True, num_conv=2):
        super().__init__()
        convs = []
        for _ in range(num_conv):
            convs.append(nn.Conv2d(dim, dim, kernel_size=1, padding=0, groups=dim))
            convs.append(nn.ReLU())
        self.convs = nn.Sequential(*convs)
        self.norm_xca = LayerNorm(dim, eps=1e-6)
        self.gamma_xca = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) \
            if layer_scale_init_value > 0 else None
        self.xca = XCA(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, expan_ratio * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(expan_ratio * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True) \
            if layer_scale_init_value > 0 else None
        self.drop_path = nn.Identity()

    def _folded_proj(self):
        """XCA's projection with gamma_xca folded in: (gamma_xca (.) W_proj [C, C], gamma_xca (.) b_proj)."""
        def build():
            w, b = self.xca.proj.weight, self.xca.proj.bias
            if self.gamma_xca is not None:
                w, b = w * self.gamma_xca[:, None], b * self.gamma_xca
            return w.contiguous(), b.contiguous()
        return derived("sdta_xca_proj", (self.xca.proj.weight, self.xca.proj.bias, self.gamma_xca), build)

    _folded_pw2 = ConvNeXtBlock._folded_pw2      # pwconv2 with gamma folded: the same attributes, the same fold

    def _fusable(self, x):
        from heal_amd import ops
        B, C, H, W = (int(v) for v in x.shape)
        return (_fused(x, self) and C % 64 == 0 and B <= 65535 and self.xca.qkv.bias is not None
                and ops.conv1x1_supported(C, 4 * C, H * W) and ops.xca_supported(C, self.xca.num_heads, H * W))

    def _fused_forward(self, x):
        """NCHW throughout.  The qkv map of the pointwise convolution IS the transposed operand layout XCA works on (channel
        s C + h d + i = row i of head h, contiguous over the pixels); attention and projection fold into one [C, C] weight per
        image (ops.xca_weights), applied to the image's v rows by heal_conv1x1 with the bias and the residual fused."""
        from heal_amd import ops
        B, C = int(x.shape[0]), int(x.shape[1])
        t = x
        for m in self.convs:
            t = _scale_bias(t, m) if isinstance(m, nn.Conv2d) else t.relu_()
        xn = ops.layernorm_nchw(t, self.norm_xca.weight, self.norm_xca.bias, self.norm_xca.eps)
        qkv = ops.conv1x1(xn, self.xca.qkv.weight[:, :, None, None], self.xca.qkv.bias, None, 0)
        pw, pb = self._folded_proj()
        Wb, _, _ = ops.xca_weights(qkv, self.xca.temperature, pw, self.xca.num_heads)
        frags = ops.xca_fragments(Wb)
        y = torch.empty_like(t)
        for b in range(B):        # B = the agents of the scene; the v rows of one image are contiguous NCHW memory
            ops.conv1x1(qkv[b:b + 1, 2 * C:3 * C], Wb[b][:, :, None, None], pb, t[b:b + 1], 0, out=y[b:b + 1], fragments=frags[b])
        yn = ops.layernorm_nchw(y, self.norm.weight, self.norm.bias, self.norm.eps)
        h = ops.conv1x1(yn, self.pwconv1.weight[:, :, None, None], self.pwconv1.bias, None, 3)
        w2, b2 = self._folded_pw2()
        return ops.conv1x1(h, w2, b2, x, 0)

    def forward(self, x):
        if self._fusable(x):
            return self._fused_forward(x)
        inp = x
        x = self.convs(x)
        B, C, H, W = x.shape
        x = x.reshape(B, C, H * W).permute(0, 2, 1)
        a = self.xca(self.norm_xca(x))
        if self.gamma_xca is not None:
            a = self.gamma_xca * a
        x = x + self.drop_path(a)
        x = x.reshape(B, H, W, C)
        x = self.pwconv2(self.act(self.pwconv1(self.norm(x))))
        if self.gamma is not None:
            x = self.gamma * x
        return inp + self.drop_path(x.permute(0, 3, 1, 2))


class SDTAAgliner(nn.Module):
    """feature_alignnet_modules.py:435-448 (the reference's spelling)."""

    def __init__(self, args):
        super().__init__()
        dim = args["dim"]
        self.model = nn.ModuleList()
        for _ in range(args["num_of_blocks"]):
            self.model.append(ConvEncoder(dim=dim))
            self.model.append(SDTAEncoder(dim=dim))

    def forward(self, x):
        for m in self.model:
            x = m(x)
        return x


ALIGNERS = {"scaligner": SCAligner, "resnet1x1": Res1x1Aligner, "resnet3x3": Res3x3Aligner, "sdta": SDTAAgliner, "cbam": CBAM,
            "fanet": FANet}
