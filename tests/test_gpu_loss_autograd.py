"""The one autograd front-end of the fused criteria (ops._FusedLoss) on the MI355X: for kd, det, occ, depth, center and unc, and for
every way of requiring gradients -- every map, strict subsets, none -- the `.grad` of each leaf is bit-equal to `scale x` the
gradient the raw operator returns for that map, and None where no gradient was asked for.

(N, H, W) = (2, 9, 15): 135 pixels, a partial 64-pixel tile per image and 6 tiles, no multiple of the 4 waves of a block.  The
scales are powers of two and 3, exact in fp32: the comparison is torch.equal."""
import numpy as np
import pytest
import torch

from heal_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = "cuda:0"
N, H, W = 2, 9, 15
SCALES = (2.0, 3.0, 0.5, 4.0)            # per term (det, center); the scalar criteria use SCALES[1]
DET = dict(pos_cls_weight=2.0, alpha=0.25, sigma=3.0, dir_offset=0.7853)
UNC = dict(xy_loss_type="l2", angle_loss_type="von-mise", angle_weight=0.5, lambda_V=0.001, s0=1.0, limit_period=True)


def _heads(A, with_dir, dim=None, label_dtype=torch.float32):
    """(maps: cls, reg, (unc,) dir | None; labels: pos, neg, targets) on the device, seeded."""
    g = torch.Generator().manual_seed(40 + A + (dim or 0))
    maps = [torch.randn((N, A, H, W), generator=g), torch.randn((N, 7 * A, H, W), generator=g) * 0.3]
    if dim is not None:
        maps.append((torch.rand((N, dim * A, H, W), generator=g) * 2 - 1) * 2.0)
    maps.append(torch.randn((N, 2 * A, H, W), generator=g) if with_dir else None)
    pos = (torch.rand((N, H, W, A), generator=g) > 0.9).to(label_dtype)
    neg = (torch.rand((N, H, W, A), generator=g) > 0.3).to(label_dtype) * (1 - pos)
    tgt = (torch.randn((N, H, W, 7 * A), generator=g) * 0.4).to(label_dtype)
    assert float(pos.sum()) > 0
    return [m if m is None else m.to(DEV) for m in maps], [t.to(DEV) for t in (pos, neg, tgt)]


def _det(A, with_dir, label_dtype):
    maps, labels = _heads(A, with_dir, label_dtype=label_dtype)
    cfg = dict(DET, weights=(1.0, 2.0, 0.2), anchor_yaw=np.deg2rad([0.0, 90.0])[:A] if with_dir else None)
    return (maps, True, lambda m: ops.det_loss_terms(*m, *labels, **cfg), lambda: ops.det_loss(*maps, *labels, **cfg))


def _unc(A, with_dir, dim):
    maps, labels = _heads(A, with_dir, dim=dim, label_dtype=torch.float64)
    cfg = dict(DET, **UNC, weights=(1.0, 2.0, 0.5, 0.2), dim=dim, anchor_yaw=np.deg2rad([0.0, 90.0])[:A] if with_dir else None)
    return (maps, False, lambda m: ops.unc_loss_terms(*m, *labels, **cfg), lambda: ops.unc_loss(*maps, *labels, **cfg))


def _occ():
    _, (pos, neg, _) = _heads(2, False)
    g = torch.Generator().manual_seed(7)
    occ = [torch.randn((N, 1, H // k, W // k), generator=g).to(DEV) for k in (1, 2, 4)]
    cfg = dict(relative_downsample=[1, 2, 4], level_weight=[0.4, 0.2, 0.1], pos_cls_weight=2.0, alpha=0.25)
    return (occ, False, lambda m: ops.occ_loss_term(m, pos, neg, **cfg), lambda: ops.occ_loss(occ, pos, neg, **cfg))


def _depth(D):
    g = torch.Generator().manual_seed(D)
    logit = (torch.randn((N, D, H, W), generator=g) * 2.0).to(DEV)
    idx = torch.randint(0, D, (N, H, W), generator=g).to(DEV)
    mask = (torch.rand((N, H, W), generator=g) > 0.6).float().to(DEV)
    return ([logit], False, lambda m: ops.depth_focal_loss_term(m[0], idx, mask, alpha=0.25, weight=1.5),
            lambda: ops.depth_focal_loss(logit, idx, mask, alpha=0.25, weight=1.5))


def _kd(C):
    g = torch.Generator().manual_seed(C)
    student, teacher = (torch.randn((N, C, H, W), generator=g).to(DEV) for _ in range(2))
    return ([student], False, lambda m: ops.KdKlLoss.apply(m[0], teacher), lambda: ops.kd_kl_loss(student, teacher))


def _center():
    g = torch.Generator().manual_seed(3)
    maps = [torch.randn((N, 1, H, W), generator=g).to(DEV), (torch.randn((N, 8, H, W), generator=g) * 0.5).to(DEV)]
    lo, hi = torch.tensor([1.0, 1.0, -1.5, 1.2, 1.5, 2.0, -3.0]), torch.tensor([W - 1.0, H - 1.0, -0.5, 2.2, 3.5, 5.0, 3.0])
    boxes = (lo + (hi - lo) * torch.rand((N, 6, 7), generator=g)).to(DEV)
    mask = torch.tensor([[1, 1, 1, 0, 1, 0], [1, 0, 1, 1, 1, 1]]).to(DEV)
    cfg = dict(cav_lidar_range=[0.0, 0.0, -3.0, float(W), float(H), 1.0], voxel_size=[1.0, 1.0, 4.0], out_size_factor=1, max_objs=8,
               min_radius=2, gaussian_overlap=0.1, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5], cls_weight=1.0, loc_weight=2.0)
    assert ops.center_loss_supported(*maps, boxes, mask, cfg["cav_lidar_range"], cfg["voxel_size"], 1, 8)
    return (maps, True, lambda m: ops.center_loss_terms(*m, boxes, mask, **cfg), lambda: ops.center_loss(*maps, boxes, mask, **cfg))


CASES = {"kd_c64": lambda: _kd(64), "kd_c5": lambda: _kd(5),
         "det_a2_dir": lambda: _det(2, True, torch.float64), "det_a1": lambda: _det(1, False, torch.float32),
         "unc_a2_dir_d3": lambda: _unc(2, True, 3), "unc_a1_d7": lambda: _unc(1, False, 7),
         "occ": _occ, "depth_d12": lambda: _depth(12), "depth_d5": lambda: _depth(5), "center": _center}


@pytest.fixture(scope="module")
def cases():
    """name -> (maps, per_term, differentiable front-end, the raw operator's (out, list of gradients)), computed once; read-only."""
    built = {}

    def get(name):
        if name not in built:
            maps, per_term, front, raw = CASES[name]()
            out, grads = raw()
            built[name] = (maps, per_term, front, out, list(grads) if isinstance(grads, (tuple, list)) else [grads])
        return built[name]
    return get


def _subsets(n):
    """Every map, the first one only, all but the first, none (what differs among them for n maps)."""
    masks = [(True,) * n, (True,) + (False,) * (n - 1), (False,) + (True,) * (n - 1), (False,) * n]
    return sorted(set(masks), reverse=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_leaf_gradients_are_the_scaled_raw_gradients_for_every_subset(cases, name):
    maps, per_term, front, raw_out, raw_grads = cases(name)
    assert len(raw_grads) == len(maps) and all((g is None) == (m is None) for g, m in zip(raw_grads, maps))
    assert all(float(g.abs().max()) > 0 for g in raw_grads if g is not None)
    for mask in _subsets(len(maps)):
        need = [want and m is not None for want, m in zip(mask, maps)]
        leaves = [None if m is None else m.clone().requires_grad_(want) for m, want in zip(maps, need)]
        out = front(leaves)
        if isinstance(out, tuple):                             # unc: (total, the four terms without a gradient)
            out, terms = out
            assert torch.equal(terms, raw_out) and not terms.requires_grad
            total = (raw_out[1] + raw_out[0]) + raw_out[2]
            assert torch.equal(out.detach(), raw_out[3] + total if maps[-1] is not None else total)
        else:
            assert torch.equal(out.detach().reshape(-1), raw_out)
        assert out.requires_grad == any(need), (name, mask)
        if any(need):
            scale = torch.tensor(SCALES[:out.numel()], device=DEV) if per_term else SCALES[1]
            (scale * out).sum().backward()
        for i, (leaf, want) in enumerate(zip(leaves, need)):
            if leaf is None:
                continue
            if not want:
                assert leaf.grad is None, (name, mask, i)
            else:
                s = SCALES[i] if per_term else SCALES[1]
                assert torch.equal(leaf.grad, s * raw_grads[i]), (name, mask, i)
