"""tests/align_refs.py, the float64 yardstick of the XCA kernel tests, pinned to the reference's own recording.

The golden (tests/golden/gen_golden_aligners.py) holds the fp32 outputs of the `sdta` aligner's blocks, taken by forward hooks.
The generator also ran the reference in float64 on the same parameters and printed, for this golden:
    ConvEncoder  (block 0): reference fp32 against its float64 run 3.563e-07 of the largest magnitude (4.581)
    SDTAEncoder  (block 1): reference fp32 against its float64 run 5.085e-07 of the largest magnitude (5.448)
    align_refs.sdta_encoder against the reference's float64 SDTAEncoder: 8.636e-16 (asserted <= 1e-12 there, where the reference is)
So the float64 restatement, fed the recorded fp32 input of block 1, must meet the recorded fp32 output of block 1 within the
reference's own fp32 error.  BOUND is four times the printed 5.085e-07: the printed figure is one draw of a rounding error, and the
margin is for the same arithmetic in another summation order, not for another algorithm (an indexing or folding error is O(1))."""
import os

import numpy as np
import pytest

from tests import align_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND = 4 * 5.085e-07
HEADS = 4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "aligners_small.npz"))


def _sd(gold, name):
    return {k[len(name) + 4:]: gold[k] for k in gold.files if k.startswith(name + "/sd/")}


def test_sdta_encoder_restatement_meets_the_reference_recording(gold):
    sd = _sd(gold, "sdta")
    got = R.sdta_encoder(gold["sdta/hook/0"], sd, "channel_align.model.1.", HEADS)
    want = gold["sdta/hook/1"].astype(np.float64)
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    print(f"sdta_encoder (float64) against the recorded fp32 block output: {err:.3e} (bound {BOUND:.3e})")
    assert err <= BOUND


def test_folded_form_is_the_token_form():
    """The folded weight against XCA as the reference writes it (tokens, F.normalize, two matmuls, permute, projection) in float64."""
    rng = np.random.default_rng(3)
    B, C, N = 3, 32 * HEADS, 63
    d = C // HEADS
    qkv = rng.standard_normal((B, 3 * C, N))
    t = rng.standard_normal((B, C, N))
    temp = np.array([1.0, 2.5, 4.0, 8.0])
    pw, pb, g = rng.standard_normal((C, C)), rng.standard_normal(C), rng.uniform(0.5, 1.5, C)
    # reference order: [B, N, 3, heads, d] -> [3, B, heads, N, d] -> transpose -> [B, heads, d, N]
    r = qkv.transpose(0, 2, 1).reshape(B, N, 3, HEADS, d).transpose(2, 0, 3, 1, 4)
    q, k, v = (np.swapaxes(r[i], -2, -1) for i in range(3))
    q = q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-12)
    k = k / np.maximum(np.linalg.norm(k, axis=-1, keepdims=True), 1e-12)
    attn = np.matmul(q, np.swapaxes(k, -2, -1)) * temp.reshape(1, HEADS, 1, 1)
    attn = np.exp(attn - attn.max(-1, keepdims=True))
    attn = attn / attn.sum(-1, keepdims=True)
    x = np.matmul(attn, v).transpose(0, 3, 1, 2).reshape(B, N, C)
    want = t + (g * (x @ pw.T + pb)).transpose(0, 2, 1)
    W = R.xca_weights(qkv, temp, g[:, None] * pw, HEADS)
    got = t + np.matmul(W, qkv[:, 2 * C:]) + (g * pb)[None, :, None]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(R.xca_attention(qkv, temp, HEADS) - attn).max() <= 1e-14


def test_zero_rows_give_zero_logits_and_fp32_mode_stays_fp32():
    rng = np.random.default_rng(4)
    qkv = rng.standard_normal((1, 3 * 64, 64)).astype(np.float32)
    qkv[0, 5] = 0          # a q row of head 0
    qkv[0, 64 + 18] = 0    # a k row of head 1
    A = R.xca_attention(qkv, np.ones(4), HEADS)
    assert np.array_equal(A[0, 0, 5], np.full(16, 1 / 16))           # logits exactly 0 -> a uniform row
    assert np.ptp(A[0, 1, :, 2]) > 0 and np.all(np.isfinite(A))
    A32 = R.xca_attention(qkv, np.ones(4), HEADS, dtype=np.float32)
    W32 = R.xca_weights(qkv, np.ones(4), np.eye(64), HEADS, dtype=np.float32)
    assert A32.dtype == np.float32 and W32.dtype == np.float32 and np.abs(A32 - A).max() < 1e-6
