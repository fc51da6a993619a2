"""Float64 restatement of warp_affine_simple's backward (torch_transformation_utils.py:323-332), shared by the CPU and GPU tests of
heal_warp_affine_forward / heal_warp_affine_backward (include/heal_amd_train_warp.h).

The restatement takes its fp32 SAMPLE POSITIONS the way the composition does: F.affine_grid in the rows' dtype, cast to fp32
(`.to(src)`), then grid_sample's own un-normalisation ((g + 1) * size - 1) / 2 in fp32.  From these fp32 pixel positions on,
everything is float64: floor, the four corner weights (the fp32 differences x1 - ix, ix - x0 are exact, so the float64 weights are
the exact products the fp32 code rounds), the adjoint  grad_src[a, c, s] = sum_d w(d, s) G[a, c, d],  the per-element scale
sum_d |w(d, s)| |G[a, c, d]|  and each source pixel's contributor set, by brute force over every destination pixel.  What is left
between the kernel and this restatement is the rounding of about ten fp32 products and sums per element: below 1e-6 of the scale.
`check_against_autograd` ties the restatement to float64 autograd of F.grid_sample on the same positions.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

BOUND = 1e-5      # |got - want| <= BOUND * scale + TINY per element: the project's backward tolerance, ten times the derived error
TINY = 1e-30


def rigid(theta_deg, tx, ty, H, W, scale=1.0):
    """The normalised (2,3) row whose pixel-space map is p(d) = scale * R(theta) d + b with the map centre moved by (tx, ty) pixels:
    A = [[m00, m01 W/H], [m10 H/W, m11]] (what normalize_pairwise_tfm gives for a pose, at scale 1)."""
    c, s = math.cos(math.radians(theta_deg)) * scale, math.sin(math.radians(theta_deg)) * scale
    if theta_deg % 90 == 0:      # exact quarter turns
        c, s = round(c / scale) * scale, round(s / scale) * scale
    return np.array([c, -s * H / W, 2.0 * tx / W, s * W / H, c, 2.0 * ty / H], dtype=np.float64)


def random_rigid(count, H, W, seed, max_shift=0.15):
    """`count` seeded rigid rows: any angle, the centre shifted by at most max_shift of the map's smaller side."""
    rng = np.random.default_rng(seed)
    m = max_shift * min(H, W)
    return np.stack([rigid(rng.uniform(0.0, 360.0), rng.uniform(-m, m), rng.uniform(-m, m), H, W) for _ in range(count)])


def named_rows(H, W):
    """The fixed rows of the suite on an H x W map."""
    return {"identity": rigid(0, 0, 0, H, W), "rot90": rigid(90, 0, 0, H, W), "rot180": rigid(180, 0, 0, H, W),
            "rot37": rigid(37, 0.3, -0.6, H, W), "shift": rigid(0, 0.4, -0.3, H, W),
            "scale075": rigid(20, 0.2, 0.1, H, W, 0.75), "scale150": rigid(-33, -0.4, 0.3, H, W, 1.5),
            "outside": rigid(0, 3.0 * W, 0, H, W)}


def positions(rows, H, W, f64, device="cpu"):
    """fp32 pixel positions (ix, iy), each [n, H, W], of the n rows ([n, 6] or [n, 2, 3]): affine_grid in the rows' dtype (float64
    when f64, else float32), cast to fp32, un-normalised in fp32 as grid_sample does."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2, 3)
    M = torch.from_numpy(rows).to(torch.float64 if f64 else torch.float32).to(device)
    g = F.affine_grid(M, [rows.shape[0], 1, H, W], align_corners=False).to(torch.float32)
    ix = ((g[..., 0] + 1.0) * float(W) - 1.0) / 2.0
    iy = ((g[..., 1] + 1.0) * float(H) - 1.0) / 2.0
    assert ix.dtype == torch.float32
    return ix.cpu(), iy.cpu()


class Restated:
    """Taps and float64 weights of every destination pixel: idx [n, H*W, 4] (linear source index, -1 outside the map; order nw, ne,
    sw, se) and w [n, H*W, 4]."""

    def __init__(self, rows, H, W, f64=True, device="cpu"):
        self.rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        self.n, self.H, self.W, self.f64 = self.rows.shape[0], H, W, f64
        ix, iy = (t.double().reshape(self.n, H * W) for t in positions(self.rows, H, W, f64, device))
        self.ix, self.iy = ix, iy
        x0, y0 = torch.floor(ix), torch.floor(iy)
        x1, y1 = x0 + 1, y0 + 1
        w = torch.stack([(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)], dim=-1)
        xs = torch.stack([x0, x1, x0, x1], dim=-1)
        ys = torch.stack([y0, y0, y1, y1], dim=-1)
        ok = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        self.idx = torch.where(ok, (ys * W + xs), torch.full_like(xs, -1.0)).long()
        self.w = torch.where(ok, w, torch.zeros_like(w))

    def _scatter(self, G, absolute):
        """sum_d w(d, s) G[a, c, d] (or with absolute values) -> [n, C, H, W] float64."""
        n, C = G.shape[:2]
        G = G.double().reshape(n, C, self.H * self.W)
        out = torch.zeros(n, C, self.H * self.W + 1, dtype=torch.float64)      # slot HW collects the taps outside (dropped)
        for k in range(4):
            idx = torch.where(self.idx[..., k] < 0, torch.full_like(self.idx[..., k], self.H * self.W), self.idx[..., k])
            w = self.w[..., k]
            term = (w.abs()[:, None] * G.abs()) if absolute else (w[:, None] * G)
            out.scatter_add_(2, idx[:, None].expand(n, C, -1), term)
        return out[..., :-1].reshape(n, C, self.H, self.W)

    def adjoint(self, G):
        return self._scatter(G, False)

    def scale(self, G):
        return self._scatter(G, True)

    def forward(self, x):
        """The warp itself in float64 (x [n, C, H, W])."""
        n, C = x.shape[:2]
        x = torch.cat([x.double().reshape(n, C, -1), torch.zeros(n, C, 1, dtype=torch.float64)], dim=2)
        out = 0
        for k in range(4):
            idx = torch.where(self.idx[..., k] < 0, torch.full_like(self.idx[..., k], self.H * self.W), self.idx[..., k])
            out = out + torch.gather(x, 2, idx[:, None].expand(n, C, -1)) * self.w[..., k][:, None]
        return out.reshape(n, C, self.H, self.W)

    def pairs(self, a):
        """Brute force: every (source pixel s, destination pixel d) of agent a such that s is one of d's four taps inside the map
        -> (s [P], d [P]) linear indices."""
        d = torch.arange(self.H * self.W)[:, None].expand(-1, 4)
        ok = self.idx[a] >= 0
        return self.idx[a][ok], d[ok]

    def coverage(self, a):
        """Fraction of agent a's source pixels that have at least one contributor."""
        s, _ = self.pairs(a)
        return float(torch.unique(s).numel()) / (self.H * self.W)

    def max_contributors(self, a):
        s, _ = self.pairs(a)
        return int(torch.bincount(s, minlength=1).max()) if s.numel() else 0


def check_against_autograd(R, G):
    """Largest |restated adjoint - float64 autograd of grid_sample| over the elements, relative to max|G|.  grid_sample gets the
    float64 grid that un-normalises to R's positions ((2 ix + 1) / W - 1), so both work on the same sample positions."""
    n, C = G.shape[:2]
    grid = torch.stack([(2.0 * R.ix + 1.0) / R.W - 1.0, (2.0 * R.iy + 1.0) / R.H - 1.0], dim=-1).reshape(n, R.H, R.W, 2)
    x = torch.zeros(n, C, R.H, R.W, dtype=torch.float64, requires_grad=True)
    F.grid_sample(x, grid, align_corners=False).backward(G.double())
    return float((x.grad - R.adjoint(G)).abs().max() / G.abs().max())


def window_violations(R, a, win):
    """Number of brute-force (s, d) pairs of agent a that lie OUTSIDE the candidate box of heal_warp_affine_window (win: its 8
    doubles): d = (w, h) must satisfy |w - cx| <= win[6] and |h - cy| <= win[7] with (cx, cy) = Ainv (s - b)."""
    s, d = R.pairs(a)
    sx, sy = (s % R.W).double(), (s // R.W).double()
    dw, dh = (d % R.W).double(), (d // R.W).double()
    ex, ey = sx - win[4], sy - win[5]
    cx, cy = win[0] * ex + win[1] * ey, win[2] * ex + win[3] * ey
    return int((((dw - cx).abs() > win[6]) | ((dh - cy).abs() > win[7])).sum())


# ---- the GPU fixtures: name -> (H, W, C, rows [n, 6]).  The smallest shapes that still hit the edges: maps of one pixel and one row,
# a map that is no multiple of the 16 x 4 tile, one of several tiles; C = 1, one more than the backward's channel chunk (32), 70;
# n = 1, 3 and HEAL_WARP_MAX_AGENTS (8).  test_warp_refs_cpu.py checks that every agent but "outside" reaches at least half of its
# source pixels (the shifts are chosen accordingly): a backward that writes zeros cannot pass.
def gpu_fixtures():
    a, b, c = named_rows(13, 21), named_rows(32, 48), named_rows(1, 7)
    r13, r32 = random_rigid(2, 13, 21, 5, 0.1), random_rigid(2, 32, 48, 6)
    return {
        "1x1": (1, 1, 1, np.stack([rigid(0, 0, 0, 1, 1)])),
        "1x7_n3_c33": (1, 7, 33, np.stack([c["identity"], rigid(0, 0.4, 0, 1, 7), c["rot180"]])),
        "13x21_n3_c70": (13, 21, 70, np.stack([a["rot37"], a["rot90"], a["shift"]])),
        "13x21_n8_c1": (13, 21, 1, np.stack([a["identity"], a["rot180"], a["rot37"], a["shift"], a["scale075"], a["scale150"],
                                             r13[0], r13[1]])),
        "32x48_n3_c33_outside": (32, 48, 33, np.stack([r32[0], b["outside"], b["rot37"]])),
        "32x48_n1_c70": (32, 48, 70, np.stack([r32[1]])),
    }


def is_outside(row, H, W):
    return bool(np.array_equal(row, named_rows(H, W)["outside"]))


def fixture_grad(name, n, C, H, W):
    """The seeded upstream gradient of a fixture (fp32 values)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.randn(n, C, H, W, generator=g, dtype=torch.float32)
