/* heal_amd_ssfa.h -- the dense neck of the SECOND + SSFA detectors (CIA-SSD's spatial-semantic feature aggregation;
 * opencood/models/sub_modules/cia_ssd_utils.py:6-55): an overlapping 3x3 stride-2 transposed convolution and the attention blend.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them).  Same conventions as include/heal_amd.h: fp32 NCHW device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no atomics, no workspace, bit-equal across launches; *_supported are host arithmetic and return 0 for a
 * shape out of range.  The library is built with -ffp-contract=off.
 *
 * heal_deconv3x3_s2 -- ConvTranspose2d(k = 3, stride = 2, padding = 1, output_padding = 1) with bias, ReLU and a residual fused:
 *     y[n,co,oy,ox] = act(bias[co] + sum_{ci,ky,kx} x[n,ci,iy,ix] w[ci,co,ky,kx]) (+ residual[n,co,oy,ox] for co < res_channels)
 *     oy = 2 iy - 1 + ky,  ox = 2 ix - 1 + kx,  output 2H x 2W.
 *   The residual is added AFTER the activation (SSFA: deconv_block_0(x_trans_1) + x_trans_0) and covers the first res_channels
 *   output channels only, so two deblocks that read one input run as one launch with their weights concatenated along Cout.
 *   The four output parities of a base pixel (by, bx) are four GEMMs over ci that share their operands (X.. = 0 outside the map):
 *     y[2by  ,2bx  ] = W11 X00                                   X00 = x[by  ,bx  ]   X01 = x[by  ,bx+1]
 *     y[2by  ,2bx+1] = W12 X00 + W10 X01                         X10 = x[by+1,bx  ]   X11 = x[by+1,bx+1]
 *     y[2by+1,2bx  ] = W21 X00 + W01 X10                         Wkykx = w[:, :, ky, kx] transposed to [co, ci]
 *     y[2by+1,2bx+1] = W22 X00 + W20 X01 + W02 X10 + W00 X11
 *   9 taps per 4 outputs and no product with an inserted zero.  The last odd row / column (by = H - 1 / bx = W - 1) keeps only its
 *   ky = 2 / kx = 2 taps: X1. / X.1 lie outside the map there.
 *   Grid (Cout / 32, ceil(H / 8) ceil(W / 16), n), 256 threads.  A wave owns 32 output channels x 2 base rows x 16 base columns
 *   (all four parities: 64 accumulator registers) on v_mfma_f32_16x16x4_f32, the weights as the A operand, 16 consecutive pixels of
 *   a row as the B operand, both read straight into registers (no LDS, no barrier) one 8-channel chunk ahead of the MFMAs.  The three
 *   input rows of a wave serve both of its base rows.  The products of 32 input channels are summed in the MFMA accumulator and the
 *   segments added in channel order in a second register set, which keeps the summation error of the longest chain (4 taps x Cin)
 *   at that of a 128-term chain.  The even and the odd column of a base pixel leave as one 8-byte store.
 *   wfrag: the weight [Cin, Cout, 3, 3] in fragment order [Cout / 16][Cin / 8][9][64][2], element [mt][kc][3 ky + kx][lane][j] =
 *   w[8 kc + 4 j + (lane >> 4)][16 mt + (lane & 15)][ky][kx].
 *
 * heal_ssfa_blend -- the two-way attention at the end of SSFA, w_0 / w_1 with their BatchNorm folded to a weight and a scalar:
 *     sa = wa . a + ba,  sb = wb . b + bb   (per pixel, over the C channels)
 *     pa = 1 / (1 + exp(sb - sa))           (softmax([sa, sb])[0])
 *     out = a pa + b (1 - pa)
 *   One pass: grid (ceil(HW / 64), n), 256 threads = 16 channel groups x 16 pixel quads; a thread keeps its C / 16 channels of four
 *   pixels of both maps in registers between the dot products (partials combined through LDS in group order) and the blend, so the
 *   memory traffic is two reads and one write.
 */
#ifndef HEAL_AMD_SSFA_H
#define HEAL_AMD_SSFA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* heal_ssfa_fused_enabled (host only): HEAL_SSFA_FUSED as the library reads it, at every call -- 1 when the variable is unset, empty
 *   or "1" (SSFA runs on this library's operators), 0 for "0" (the reference's torch composition on the device), -1 for any other
 *   text.                                                                                                                       */
int heal_ssfa_fused_enabled(void);

/* heal_deconv3x3_s2_supported (host only): 1 if heal_deconv3x3_s2 takes the shape -- cin and cout multiples of 32 in 32 .. 2048,
 *   H, W >= 1, at most 65535 tiles of 8 x 16 base pixels and 4 H W < 2^31 -- else 0.                                            */
int heal_deconv3x3_s2_supported(int cin, int cout, int H, int W);

/* heal_deconv3x3_s2: x [n, cin, H, W]; wfrag (above); bias [cout] or NULL; residual [n, res_channels, 2H, 2W] or NULL with
 *   res_channels 0 (0 <= res_channels <= cout); relu 0 | 1; y [n, cout, 2H, 2W].  x, wfrag, residual and y 16-byte aligned;
 *   1 <= n <= 65535.                                                                                                            */
int heal_deconv3x3_s2(const float* x, const float* wfrag, const float* bias, const float* residual, int res_channels, int n,
                      int cin, int cout, int H, int W, int relu, float* y, void* stream);

/* heal_ssfa_blend_supported (host only): 1 for C in {64, 128}, HW % 4 == 0 (16-byte pixel rows), 4 <= HW < 2^24, else 0.       */
int heal_ssfa_blend_supported(int C, int HW);

/* heal_ssfa_blend: a, b [n, C, HW]; wa, wb [C]; ba, bb one float each ON THE DEVICE (a folded BatchNorm shift: no host read);
 *   out [n, C, HW]; pa_out [n, HW] or NULL.  a, b, out and pa_out 16-byte aligned; 1 <= n <= 65535.                             */
int heal_ssfa_blend(const float* a, const float* b, const float* wa, const float* wb, const float* ba, const float* bb, int n,
                    int C, int HW, float* out, float* pa_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
