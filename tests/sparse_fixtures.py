"""Integer fixtures of the sparse 3-D convolution conformance suite (tests/test_gpu_sparse_conformance.py) -- numpy only, so that
the CPU test (tests/test_sparse_fixtures_cpu.py) can check on a machine without a GPU that every geometry still reaches the edge
its case id names.

Values follow tests/test_gpu_conformance.py: features are integers in [-3, 3] scaled by 1 or 2 (alternating every 4 rows),
weights integers in [-2, 2] scaled per output channel by 0 / 1 / 2 counted from the last channel, BatchNorm scales powers of two
and shifts nonzero quarter-integers.  Every product and partial sum is then a quarter-integer far below 2^24: fp32 computes it
exactly in any summation order, and a kernel result must equal the fp64 reference bit for bit."""
import numpy as np

from oracle import oracle_np as O

EXACT = 2.0 ** 22          # every output's sum |w||x| * scale + |shift| stays below this
SLOT = 64                  # output sites per pair-tile slot (k_sp_nbr_tiles) and per k_sp_conv2 block at M = 64

# name -> (ksize, stride, padding, submanifold)
LAYERS = {
    "subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    "s2": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
    "s2p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), False),
    "k311": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),      # conv_out of VoxelBackBone8x
}

COUNTS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)

# the filled box of `dense`: batch b's sites are rows b * 4128 .. ; interior row (z, y) = (1, 1) of the box holds the sorted rows
# 1291 .. 1546, which contain the aligned runs 1344 .. 1407 (64) and 1408 .. 1535 (64 and 128) of sites with all 27 taps live
DENSE_SHAPE, DENSE_BOX0, DENSE_BOX = (6, 6, 262), (1, 1, 2), (4, 4, 258)


def keys(idx, shape):
    idx = np.asarray(idx, np.int64)
    D, H, W = shape
    return ((idx[:, 0] * D + idx[:, 1]) * H + idx[:, 2]) * W + idx[:, 3]


def sort_sites(idx, shape):
    idx = np.asarray(idx, np.int32)
    return np.ascontiguousarray(idx[np.argsort(keys(idx, shape), kind="stable")])


class Geometry:
    """Sorted input sites; `rules(layer)` -> (out_idx, out_shape, nbr [n_out, K] int64) from oracle_np.sparse_conv_rules."""

    def __init__(self, name, idx, shape, batch):
        self.name, self.shape, self.batch = name, list(shape), int(batch)
        self.idx = sort_sites(idx, shape)
        k = keys(self.idx, shape)
        assert len(k) >= 1 and np.all(np.diff(k) > 0), f"{name}: sites must be unique"
        self._rules = {}

    @property
    def n(self):
        return int(self.idx.shape[0])

    def rules(self, layer):
        if layer not in self._rules:
            ks, st, pd, subm = LAYERS[layer]
            out_idx, out_shape, nbr = O.sparse_conv_rules(self.idx, self.shape, ks, st, pd, subm)
            self._rules[layer] = (np.ascontiguousarray(out_idx, np.int32), list(out_shape), nbr)
        return self._rules[layer]


def full_slots(nbr, sites=SLOT):
    """Slots (`sites` consecutive output rows starting at a multiple of `sites`) whose every row has all taps live."""
    n = nbr.shape[0] // sites * sites
    full = (nbr[:n] >= 0).all(1).reshape(-1, sites).all(1)
    return np.nonzero(full)[0]


def dense():
    """A filled 4 x 4 x 258 box per batch inside a 6 x 6 x 262 grid: whole 64- and 128-site slots of the submanifold layer have
    27 live taps at every site -- the worst case that sizes the pair tiles (108 tiles) and k_sp_conv2's MAXT."""
    z, y, x = np.meshgrid(*(np.arange(o, o + s) for o, s in zip(DENSE_BOX0, DENSE_BOX)), indexing="ij")
    one = np.stack([z.ravel(), y.ravel(), x.ravel()], 1)
    idx = np.concatenate([np.concatenate([np.full((len(one), 1), b), one], 1) for b in range(2)])
    return Geometry("dense", idx, DENSE_SHAPE, 2)


def isolated():
    """Sites 3 cells apart in every direction: each submanifold output has the centre tap only."""
    z, y, x = np.meshgrid(np.arange(1, 10, 3), np.arange(0, 13, 3), np.arange(2, 16, 3), indexing="ij")
    one = np.stack([z.ravel(), y.ravel(), x.ravel()], 1)
    idx = np.concatenate([np.concatenate([np.full((len(one), 1), b), one], 1) for b in range(2)])
    return Geometry("isolated", idx, (10, 13, 16), 2)


def faces():
    """Every face, edge and corner cell of an odd 7 x 9 x 11 grid (2 batches): taps that fall outside the grid on every side,
    under stride 2 with padding (1, 1, 1) and (0, 1, 1)."""
    shape = (7, 9, 11)
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    on = (z == 0) | (z == shape[0] - 1) | (y == 0) | (y == shape[1] - 1) | (x == 0) | (x == shape[2] - 1)
    one = np.stack([z[on], y[on], x[on]], 1)
    idx = np.concatenate([np.concatenate([np.full((len(one), 1), b), one], 1) for b in range(2)])
    return Geometry("faces", idx, shape, 2)


def seam(seed=5):
    """3 batches of 5 x 6 x 7 at 30 % occupancy, plus the last cell of batches 0, 1 and the first cell of batches 1, 2: adjacent
    linear keys across each batch boundary, which no neighbour pair may cross."""
    shape, batch = (5, 6, 7), 3
    rng = np.random.default_rng(seed)
    cells = batch * shape[0] * shape[1] * shape[2]
    flat = np.unique(np.concatenate([np.nonzero(rng.random(cells) < 0.3)[0], seam_keys(shape, batch)]))
    idx = np.stack(np.unravel_index(flat, (batch,) + shape), 1)
    return Geometry("seam", idx, shape, batch)


def seam_keys(shape, batch):
    per = shape[0] * shape[1] * shape[2]
    return np.array([k for b in range(batch - 1) for k in ((b + 1) * per - 1, (b + 1) * per)], np.int64)


def counts(n, seed=None):
    """n random sites of one 5 x 6 x 8 grid: the tail blocks of M = 64 | 128, the tail tiles, slots of 64 | 128 sites."""
    shape = (5, 6, 8)
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    flat = np.sort(rng.choice(shape[0] * shape[1] * shape[2], size=n, replace=False))
    idx = np.stack(np.unravel_index(flat, (1,) + shape), 1)
    return Geometry(f"counts{n}", idx, shape, 1)


# ---- values -------------------------------------------------------------------------------------------------------------------
def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def chan_mag(c):
    """2, 1, 0, 2, 1, 0, ... counted backwards from the last channel."""
    return np.array([(2.0, 1.0, 0.0)[(c - 1 - i) % 3] for i in range(c)])


def features(rng, n, c):
    """Integers in [-3, 3] times 1 or 2, alternating every 4 rows."""
    return (ints(rng, (n, c), -3, 3) * (1.0 + (np.arange(n) // 4) % 2)[:, None]).astype(np.float32)


def weights(rng, K, cin, cout):
    """[K, Cin, Cout]: integers in [-2, 2] times the output channel's magnitude."""
    return (ints(rng, (K, cin, cout), -2, 2) * chan_mag(cout)[None, None, :]).astype(np.float32)


def batchnorm(rng, c):
    """(scale, shift): powers of two in [1/4, 2]; nonzero quarter-integers in +-[1/4, 8]."""
    scale = 2.0 ** rng.integers(-2, 2, size=c)
    shift = rng.integers(1, 33, size=c) / 4.0 * (2 * rng.integers(0, 2, size=c) - 1)
    return scale.astype(np.float32), shift.astype(np.float32)


def conv_ref(x, nbr, w):
    """fp64 gather-matmul y[o] = sum_t W[t]^T x[nbr[o, t]] and its bound sum_t |W[t]|^T |x[nbr[o, t]]|."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    y = np.zeros((nbr.shape[0], w.shape[2]))
    bound = np.zeros_like(y)
    for t in range(nbr.shape[1]):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        if rows.size:
            xs = x[nbr[rows, t]]
            y[rows] += xs @ w[t]
            bound[rows] += np.abs(xs) @ np.abs(w[t])
    return y, bound


def bn_bound(bound, scale, shift):
    return bound * np.abs(np.asarray(scale, np.float64)) + np.abs(np.asarray(shift, np.float64))


def wgrad_table(rng, n_out, n_in, K, density=0.3, tap_pairs=(31, 32, 33)):
    """A synthetic [n_out, K] rulebook for the weight gradient (rows need not form a valid convolution there): live entries at
    `density`, the last output row with every tap live (the last row of the last chunk), and in chunk 0 tap t < len(tap_pairs) has
    exactly tap_pairs[t] pairs (the seams of the 32-pair MFMA stages), one of them on the chunk's last row."""
    nbr = np.where(rng.random((n_out, K)) < density, rng.integers(0, n_in, size=(n_out, K)), -1)
    nbr[-1] = rng.integers(0, n_in, size=K)
    for t, p in enumerate(tap_pairs[:K]):
        rows = min(n_out, 2048)
        if p > rows:
            continue
        col = np.full(rows, -1)
        col[np.append(np.sort(rng.choice(rows - 1, size=p - 1, replace=False)), rows - 1)] = rng.integers(0, n_in, size=p)
        nbr[:rows, t] = col
    return nbr.astype(np.int64)


def wgrad_ref(x, g, nbr, chunk=2048):
    """Per-chunk fp64 partials [chunks, K, Cin, Cout] of dW[t] = sum over pairs x[i]^T g[o], and the bound of their sum."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    n_out, K = nbr.shape
    chunks = (n_out + chunk - 1) // chunk
    part = np.zeros((chunks, K, x.shape[1], g.shape[1]))
    bound = np.zeros((K, x.shape[1], g.shape[1]))
    for c in range(chunks):
        for t in range(K):
            o = c * chunk + np.nonzero(nbr[c * chunk:(c + 1) * chunk, t] >= 0)[0]
            if o.size:
                part[c, t] = x[nbr[o, t]].T @ g[o]
                bound[t] += np.abs(x[nbr[o, t]]).T @ np.abs(g[o])
    return part, bound
