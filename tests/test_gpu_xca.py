"""heal_xca_weights through ops.xca_weights against the float64 restatement tests/align_refs.py (itself pinned to the reference's
recording by tests/test_align_refs_cpu.py).

Shapes: the smallest at which each mechanism of the Gram pass can go wrong.  The block step is 256 pixels; heal_xca_parts gives
    N = 64          one part, a partly filled step (three of the four waves see only zeros)
    N = 260         two parts of range 256, the second holding a single float4
    N = 1620        (45 x 36) seven parts, the last one 84 pixels: no range boundary falls on the map's end
    N = 12000       with B = 3 the grid is full, so a part is two steps: the loop runs twice and its last step is partial
for d = 16 (C = 64) and d = 32 (C = 128), B = 1 and B = 3 with different images, four distinct temperatures.

Bounds.  Gram matrix and squared norms (want_stats), per element: 2 (L + P) 2^-24 sum_n |q k| with L the pixels of one part and P the
parts -- the recursive-summation bound for a chain of L products followed by P partials, doubled for the roundings inside the matrix
instruction.  A and W: four times the error of the SAME expressions evaluated in fp32 on the CPU (align_refs with dtype=float32)
against float64, with a floor of 1e-6 of the largest magnitude; the margin is for another summation order, not another algorithm.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import align_refs as R

pytestmark = pytest.mark.gpu

HEADS = 4
TEMPS = (1.0, 2.5, 4.0, 8.0)
CASES = [(1, 64, 64), (1, 64, 260), (1, 64, 1620), (3, 64, 1620), (1, 128, 64), (1, 128, 260), (3, 128, 1620), (3, 64, 12000),
         (3, 128, 12000)]


def make(B, C, N, seed, temps=TEMPS):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.25, 2.0, (B, 3 * C, 1))                  # rows of different size: the normalisation has work to do
    qkv = (rng.standard_normal((B, 3 * C, N)) * scale).astype(np.float32)
    pw = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    return qkv, np.asarray(temps, np.float32), pw


def run(qkv, temp, pw, **kw):
    dev = torch.device("cuda:0")
    return ops.xca_weights(torch.from_numpy(qkv).to(dev), torch.from_numpy(temp).to(dev).reshape(HEADS, 1, 1),
                           torch.from_numpy(pw).to(dev), HEADS, **kw)


def check(qkv, temp, pw, tag):
    B, C3, N = qkv.shape
    C, d = C3 // 3, C3 // 3 // HEADS
    W, A, stats = run(qkv, temp, pw, want_attn=True, want_stats=True)
    W, A, stats = W.cpu().numpy(), A.cpu().numpy(), stats.cpu().numpy().astype(np.float64)
    assert W.shape == (B, C, C) and A.shape == (B, HEADS, d, d) and stats.shape == (B, HEADS, d * d + 2 * d)
    # Gram matrix and squared norms, per element
    P, L = ops.xca_parts(B, HEADS, N)
    assert P >= 1 and L % 256 == 0 and (P - 1) * L < N <= P * L
    G64, q64, k64 = R.xca_stats(qkv, HEADS)
    unit = 2.0 * (L + P) * 2.0 ** -24
    gerr = np.abs(stats[..., :d * d].reshape(B, HEADS, d, d) - G64)
    gbound = unit * R.abs_gram(qkv, HEADS)
    nerr = np.abs(np.concatenate([stats[..., d * d:d * d + d] - q64, stats[..., d * d + d:] - k64], -1))
    nbound = unit * np.concatenate([q64, k64], -1)
    print(f"{tag}: parts {P} x {L} px; Gram error / bound {float((gerr / np.maximum(gbound, 1e-300)).max()):.3e}, "
          f"norm error / bound {float((nerr / np.maximum(nbound, 1e-300)).max()):.3e}")
    assert (gerr <= gbound).all() and (nerr <= nbound).all()
    # attention and folded weight against float64, measured against what plain fp32 arithmetic gives
    out = {}
    for name, got, fn in (("A", A, lambda dt: R.xca_attention(qkv, temp, HEADS, dt)),
                          ("W", W, lambda dt: R.xca_weights(qkv, temp, pw, HEADS, dt))):
        want = fn(np.float64)
        ref32 = float(np.abs(fn(np.float32).astype(np.float64) - want).max())
        tol = max(4.0 * ref32, 1e-6 * float(np.abs(want).max()))
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag}: {name} error {err:.3e}, fp32 restatement {ref32:.3e}, tolerance {tol:.3e}, largest |{name}| "
              f"{float(np.abs(want).max()):.3e}")
        out[name] = (err, tol)
    assert np.isfinite(A).all() and np.isfinite(W).all()
    for name, (err, tol) in out.items():
        assert err <= tol, (name, err, tol)
    np.testing.assert_allclose(A.sum(-1), 1.0, atol=1e-5)
    return A


@pytest.mark.parametrize("B,C,N", CASES)
def test_weights_against_float64(B, C, N):
    check(*make(B, C, N, seed=B * 1000 + C + N), tag=f"B{B} C{C} N{N}")


def test_zero_rows_take_the_clamp():
    qkv, temp, pw = make(1, 64, 1620, seed=7)
    qkv[0, 5] = 0                    # a q row of head 0
    qkv[0, 64 + 16 + 2] = 0          # a k row of head 1
    A = check(qkv, temp, pw, tag="zero rows")
    assert np.array_equal(A[0, 0, 5], np.full(16, np.float32(1 / 16)))      # logits exactly 0: a uniform row


def test_large_temperature_needs_the_max_subtraction():
    qkv, _, pw = make(1, 64, 260, seed=8)
    qkv[0, 64 + 3] = 2.0 * qkv[0, 3]          # k row 3 parallel to q row 3: a logit of 60, exp(60) overflows fp32
    A = check(qkv, np.asarray((60.0, 2.5, 4.0, 8.0), np.float32), pw, tag="temperature 60")
    assert A[0, 0, 3, 3] > 0.99


def test_repeated_calls_are_bit_equal():
    qkv, temp, pw = make(3, 128, 1620, seed=9)
    a = run(qkv, temp, pw, want_attn=True, want_stats=True)
    b = run(qkv, temp, pw, want_attn=True, want_stats=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    w_only = run(qkv, temp, pw)
    assert w_only[1] is None and w_only[2] is None and torch.equal(w_only[0], a[0])


def test_unsupported_shape_is_refused():
    assert not ops.xca_supported(64, HEADS, 63)
    assert not ops.xca_supported(64, HEADS, 60) and not ops.xca_supported(96, HEADS, 256) and ops.xca_supported(64, HEADS, 64)
    qkv, temp, pw = make(1, 64, 63, seed=1)
    with pytest.raises(_capi.HealAmdError):
        run(qkv, temp, pw)


def test_fragments_are_the_pointwise_kernels_layout():
    """ops.xca_fragments against ops.conv1x1_fragments, and the per-image apply against float64."""
    dev = torch.device("cuda:0")
    qkv, temp, pw = make(2, 64, 260, seed=11)
    W, _, _ = run(qkv, temp, pw)
    frags = ops.xca_fragments(W)
    for b in range(2):
        assert torch.equal(frags[b].reshape(-1), ops.conv1x1_fragments(W[b].clone()).reshape(-1))
    rng = np.random.default_rng(12)
    t = rng.standard_normal((2, 64, 13, 20)).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    q4 = torch.from_numpy(qkv).to(dev).reshape(2, 192, 13, 20)
    td, y = torch.from_numpy(t).to(dev), torch.empty((2, 64, 13, 20), device=dev)
    for b in range(2):
        ops.conv1x1(q4[b:b + 1, 128:], W[b][:, :, None, None], torch.from_numpy(bias).to(dev), td[b:b + 1], 0, out=y[b:b + 1],
                    fragments=frags[b])
    want = t.reshape(2, 64, 260) + np.matmul(R.xca_weights(qkv, temp, pw, HEADS), qkv[:, 128:].astype(np.float64)) \
        + bias[None, :, None]
    err = float(np.abs(y.cpu().numpy().reshape(2, 64, 260) - want).max()) / float(np.abs(want).max())
    print(f"apply: {err:.3e} of the largest magnitude")
    assert err <= 1e-5
