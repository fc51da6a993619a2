"""heal_warp_att_fuse_levels_masked (ops.warp_att_fuse_levels(..., masks=)) on the device: equal, element for element, to the
unmasked entry on maps premultiplied by their masks; bit-equal to it on the raw maps under all-ones masks; and within the
per-element bound of tests/coalign_refs.py (the tolerance of tests/test_gpu_coalign_conformance.py) of the float64 restatement
"premultiply, then fuse" (tests/comm_refs.py)."""
import functools

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import coalign_refs as R
from tests import comm_refs as CR
from tests.test_gpu_attention_conformance import Operands, Worst

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE = [(None, 9, 13)]                               # one level, odd sizes (C filled in per case)
THREE = [(None, 13, 21), (None, 7, 11), (None, 3, 5)]


def shifted_rows(n, seed):
    """The ego's identity, then rotations by arbitrary angles with shifts: taps leave the map over every border."""
    return R.rotation_rows(n, seed)


def outside_rows(n):
    """Identity rows, agent 1 translated by three maps: no ego pixel reaches it."""
    rows = np.tile(R.IDENTITY, (n, 1, 1))
    if n > 1:
        rows[1, 0, 2] = 6.0
    return rows


POSES = {"identity": lambda n, seed: np.tile(R.IDENTITY, (n, 1, 1)), "rotated": shifted_rows, "outside": lambda n, seed: outside_rows(n)}


@functools.lru_cache(maxsize=None)
def fixture(n, C, levels, pose, seed):
    """Random features and random zero / one masks (about 60 % ones; agent 0's of level 0 has a zero row, the last agent's are all
    ones) for one launch -> dict(feats, masks, rows, sqrt_dims).  Computed once, never modified."""
    shapes = [(C, H, W) for _, H, W in (ONE if levels == 1 else THREE)]
    g = np.random.default_rng(1000 * n + seed)
    feats = [R.random_feats(n, c, H, W, seed + 17 * i) for i, (c, H, W) in enumerate(shapes)]
    masks = [(g.random((n, 1, H, W)) < 0.6).astype(np.float32) for _, H, W in shapes]
    masks[0][0, 0, 2] = 0
    for m in masks:
        m[n - 1] = 1
    sd = [float(np.float32(1.25 * np.sqrt(c))) for c, _, _ in shapes]
    return dict(feats=feats, masks=masks, rows=POSES[pose](n, seed), sqrt_dims=sd)


def launch(fx, mode, masks, feats=None, what="masked", rows=None, grid_f64=True):
    """One launch into poisoned destinations, operands behind poisoned guards -> list of float32 numpy [C, H, W]."""
    op = Operands()
    xs = [op.put(f) for f in (fx["feats"] if feats is None else feats)]
    ms = None if masks is None else [op.put(m) for m in masks]
    outs = [op.out(f.shape[1:]) for f in fx["feats"]]
    res = ops.warp_att_fuse_levels(xs, fx["rows"] if rows is None else rows, grid_f64, mode, fx["sqrt_dims"], outs=outs, masks=ms)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, outs))
    op.check(what)
    return [o.cpu().numpy() for o in outs]


def same(a, b):
    """Equal as fp32 values (-0 == +0: a masked tap has the sign of the word it was multiplied with)."""
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


# every agent count: k_warp_att_fuse_masked<NA> is instantiated apart from the unmasked kernel.  1, 3 and 8 on every axis; the counts
# between them on the smallest case that still crosses a level boundary under a rotation.
MASKED_CASES = ([(n, C, levels, pose) for n in (1, 3, 8) for C in (6, 64) for levels in (1, 3) for pose in sorted(POSES)]
                + [(n, 6, 3, "rotated") for n in (2, 4, 5, 6, 7)])


@pytest.mark.parametrize("n,C,levels,pose", MASKED_CASES)
def test_masked_entry_equals_the_unmasked_entry_on_premultiplied_maps(n, C, levels, pose):
    fx = fixture(n, C, levels, pose, 7)
    pre = [CR.premultiply(f, m) for f, m in zip(fx["feats"], fx["masks"])]
    ones = [np.ones_like(m) for m in fx["masks"]]
    worst = Worst("comm_fuse_att", n=n, C=C, levels=levels, pose=pose)
    for mode in ("att", "max"):
        got = launch(fx, mode, fx["masks"], what=f"masked {mode}")
        want = launch(fx, mode, None, feats=pre, what=f"premultiplied {mode}")
        raw = launch(fx, mode, None, what=f"raw {mode}")
        all_ones = launch(fx, mode, ones, what=f"ones {mode}")
        for l in range(len(got)):
            assert same(got[l], want[l]), (mode, l, "masked != unmasked on premultiplied maps")
            assert np.array_equal(all_ones[l].view(np.int32), raw[l].view(np.int32)), (mode, l, "all-ones masks change the bits")
            if n > 1:                                   # (one agent: its masks are all ones, see fixture)
                assert not same(got[l], raw[l]), (mode, l, "the mask had no effect")
            f, m = fx["feats"][l], fx["masks"][l]
            if mode == "max":
                assert same(got[l], CR.masked_max(f, m, fx["rows"])), (mode, l)
            else:
                ref = CR.masked_att(f, m, fx["rows"], fx["sqrt_dims"][l])
                worst.add(f"pix{ref['layout'][0]}", R.max_ratio(got[l], ref["out"], ref["B"]), f"level {l} {f.shape}")
    worst.done()


@pytest.mark.parametrize("grid_f64", [True, False])
def test_masked_entry_device_rows_equal_host_rows(grid_f64):
    """The rows as a float64 CUDA tensor (read by the kernel at run time) give the bits of the rows passed by value: the file's
    smallest rotated fixture with more than one agent, three levels in one launch."""
    fx = fixture(3, 6, 3, "rotated", 7)
    dev_rows = torch.from_numpy(fx["rows"]).to(DEV)
    for mode in ("att", "max"):
        host = launch(fx, mode, fx["masks"], what=f"host rows {mode}", grid_f64=grid_f64)
        got = launch(fx, mode, fx["masks"], what=f"device rows {mode}", rows=dev_rows, grid_f64=grid_f64)
        for l in range(len(host)):
            assert float(np.abs(host[l]).max()) > 0
            assert torch.equal(torch.from_numpy(got[l]), torch.from_numpy(host[l])), (mode, l)


def test_masks_are_checked_like_the_feature_maps_before_the_launch(monkeypatch):
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    z = lambda *s: torch.zeros(s, device=DEV)      # noqa: E731
    feats = [z(2, 4, 8, 16), z(2, 8, 4, 8)]
    good = [z(2, 1, 8, 16), z(2, 1, 4, 8)]
    rows = np.tile(R.IDENTITY, (2, 1, 1))
    for bad in ([good[0]], [good[0], z(2, 1, 4, 4)], [good[0], z(2, 2, 4, 8)], [good[0], z(1, 1, 4, 8)], [good[0].double(), good[1]],
                [good[0], good[1].cpu()], [good[0], good[1].tolist()], [good[0], z(2, 4, 8)]):
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels(feats, rows, masks=bad)
        assert launched == []
    out = ops.warp_att_fuse_levels(feats, rows, masks=[z(2, 1, 8, 32)[..., ::2], good[1]])     # a strided view is made contiguous
    assert launched == ["heal_warp_att_fuse_levels_masked"] and tuple(out[0].shape) == (4, 8, 16)
    ops.warp_att_fuse_levels(feats, rows)
    assert launched[-1] == "heal_warp_att_fuse_levels"                                        # masks=None: the unmasked entry
