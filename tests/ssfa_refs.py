"""fp64 numpy restatements of the two SSFA kernels (include/heal_amd_ssfa.h), written in another formulation than the kernels use.

deconv3x3_s2   a SCATTER over input pixels: every x[iy, ix] adds its Cout x 3 x 3 patch into the output at rows 2 iy - 1 + ky and
               columns 2 ix - 1 + kx (the kernel gathers by output parity).  Rows / columns -1 of the padded canvas are cut off
               (padding 1); row / column 2H - 1 / 2W - 1 exists because of output_padding 1.
ssfa_blend     the two-way softmax through log-sum-exp: pa = exp(sa - lse(sa, sb)) (the kernel evaluates 1 / (1 + exp(sb - sa))).
"""
import numpy as np


def deconv3x3_s2_linear(x, w):
    """The transposed convolution alone (no bias, no activation): x [n,Cin,H,W], w [Cin,Cout,3,3] -> [n,Cout,2H,2W] float64."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, H, W = x.shape
    cout = w.shape[1]
    canvas = np.zeros((n, cout, 2 * H + 1, 2 * W + 1))          # canvas row r = output row r - 1
    xm = x.reshape(n, cin, H * W)
    for ky in range(3):
        for kx in range(3):
            # every input pixel at once: its contribution through tap (ky, kx) lands at canvas (2 iy + ky, 2 ix + kx)
            canvas[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.matmul(w[:, :, ky, kx].T[None], xm).reshape(n, cout, H, W)
    return canvas[:, :, 1:, 1:].copy()


def deconv3x3_s2(x, w, bias=None, relu=True, residual=None, linear=None):
    """x [n,Cin,H,W], w [Cin,Cout,3,3] (ConvTranspose2d layout), bias [Cout], residual [n,R,2H,2W] added after the ReLU to the first
    R channels -> [n,Cout,2H,2W] float64.  linear: deconv3x3_s2_linear(x, w) if the caller has it already."""
    y = deconv3x3_s2_linear(x, w) if linear is None else np.array(linear, np.float64)
    if bias is not None:
        y += np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if relu:
        y = np.maximum(y, 0.0)
    if residual is not None:
        r = np.asarray(residual, np.float64)
        y[:, :r.shape[1]] += r
    return y


def ssfa_blend(a, b, wa, ba, wb, bb):
    """a, b [n,C,H,W]; wa, wb [C]; ba, bb scalars -> (out [n,C,H,W], pa [n,1,H,W]) float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sa = np.einsum("nchw,c->nhw", a, np.asarray(wa, np.float64).reshape(-1))[:, None] + float(ba)
    sb = np.einsum("nchw,c->nhw", b, np.asarray(wb, np.float64).reshape(-1))[:, None] + float(bb)
    m = np.maximum(sa, sb)
    lse = m + np.log(np.exp(sa - m) + np.exp(sb - m))
    pa, pb = np.exp(sa - lse), np.exp(sb - lse)
    return a * pa + b * pb, pa
