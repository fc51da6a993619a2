"""CoAlign's fused warp + agent-attention kernel element by element: k_warp_att_fuse<n> (heal_amd/csrc/warp_fuse.hip) for n = 1..8 in
both modes and both block layouts (16 pixels x 16 channel slices, 64 pixels x 4 slices), each layout alone and mixed in one launch.

`max` mode is compared bit for bit with the kernel's own sampling arithmetic repeated in fp32 numpy (tests/coalign_refs.py:
sample_f32), random float features included.  `att` mode is compared bit for bit on the exact fixtures (equal agents, selector) and
held to the per-element bound |got - ref| <= SAFETY * EPS * (k * T + E) + TINY on random floats, with k, T and E derived in
tests/coalign_refs.py from the kernel's operation sequence (coalign_k; proven to have teeth on the CPU in
tests/test_coalign_refs_cpu.py).  Nothing is normalised by a tensor-wide maximum.  The features lie inside NaN-poisoned buffers and
every output is NaN-prefilled inside one: a tap of weight 0 must still read a valid address (NaN * 0 would show), every output word
must have been written, and no word outside may change."""
import functools

import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import coalign_refs as R
from tests.test_gpu_attention_conformance import Operands, Worst

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def launch(fx, mode, what, grid_f64=True, device_rows=False):
    """One launch of every level of the fixture into poisoned destinations -> list of float32 numpy [C, H, W]."""
    op = Operands()
    xs = [op.put(f) for f in fx["feats"]]
    outs = [op.out(f.shape[1:]) for f in fx["feats"]]
    rows = torch.from_numpy(fx["rows"]).to(DEV) if device_rows else fx["rows"]
    with torch.no_grad():
        res = ops.warp_att_fuse_levels(xs, rows, grid_f64, mode, fx.get("sqrt_dims"), outs=outs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, outs))
    op.check(what)
    return [o.cpu().numpy() for o in outs]


def same_bits(a, b):
    """Equal as fp32 values (-0 == +0: a tap of weight 0 has the sign of whichever finite word it was multiplied with)."""
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def check(fx, mode, worst, tag, grid_f64=True, got=None):
    """max: bit for bit; att: the per-element bound, recorded per layout.  n = 1 in att mode is 1 * x + 0: the sample itself."""
    got = launch(fx, mode, tag, grid_f64) if got is None else got
    n = fx["feats"][0].shape[0]
    for l, f in enumerate(fx["feats"]):
        if mode == "max":
            assert same_bits(got[l], R.max_reference(f, fx["rows"], grid_f64)), (tag, "max", l, f.shape)
            continue
        ref = att_ref(fx, l, grid_f64)
        worst.add(f"pix{ref['layout'][0]}", R.max_ratio(got[l], ref["out"], ref["B"]), f"{tag} level {l} {tuple(f.shape)}")
        if n == 1:
            assert same_bits(got[l], R.sample_f32(f, fx["rows"], grid_f64)[0]), (tag, "one agent", l)
    return got


_REFS = {}


def att_ref(fx, l, grid_f64=True):
    """The float64 reference of level l of a fixture, computed once per fixture object and never modified."""
    key = (id(fx), l, grid_f64)
    if key not in _REFS:
        sd = None if fx.get("sqrt_dims") is None else fx["sqrt_dims"][l]
        r = R.att_reference(fx["feats"][l], fx["rows"], sd, grid_f64)
        _REFS[key] = (fx, {k: r[k] for k in ("out", "B", "layout")})          # the fixture is kept alive: id() stays unique
    return _REFS[key][1]


@functools.lru_cache(maxsize=None)
def fixture(n, name, pose, seed, own_sqrt_dims=True):
    levels = {"mixed": R.MIXED, "small": R.SMALL, "threshold": R.THRESHOLD, "pix64": [R.PIX64]}
    levels.update({f"mixed{i}": [lv] for i, lv in enumerate(R.MIXED)})
    return R.bound_fixture(n, levels[name], pose, seed, own_sqrt_dims)


# ================================================================================================ every instantiation, both layouts
@pytest.mark.parametrize("n", range(1, 9))
def test_every_agent_count_in_both_layouts_and_modes(n):
    """k_warp_att_fuse<n> on four levels in one launch -- 16-pixel, 64-pixel (253 x 260, ragged on both axes), W < 16 and 1 x 1 --
    so that block0 is crossed from each layout into the other; rotations with taps off every border (n = 1: the ego under a rotation
    of its own).  Two launches give the same bits."""
    worst = Worst("coalign_att", n=n, levels="mixed")
    fx = fixture(n, "mixed", "rot" if n > 1 else "ego", n)
    got = check(fx, "att", worst, "mixed att")
    again = launch(fx, "att", "mixed att again")
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again)), "two launches differ"
    check(fx, "max", worst, "mixed max")
    worst.done()


@pytest.mark.parametrize("name", ["mixed0", "mixed1", "mixed2", "mixed3", "small", "threshold"])
def test_each_layout_alone_channel_counts_and_the_threshold(name):
    """Every level of the mixed launch alone (block0 = 0 only); C = 1 (15 empty slices), C = 64 and a map with W < 16; and a pair of
    levels on either side of the 1024-tile threshold between the layouts (252 and 256 rows of 256 pixels)."""
    n = 2 if name == "threshold" else 3
    worst = Worst("coalign_att", n=n, levels=name)
    fx = fixture(n, name, "rot", 11)
    for mode in ("att", "max"):
        check(fx, mode, worst, f"{name} {mode}")
    worst.done()


# ======================================================================================================================= poses
@pytest.mark.parametrize("pose,name,n", [("identity", "small", 5), ("offmap", "small", 5), ("offmap", "pix64", 3), ("ego", "small", 4),
                                         ("ego", "pix64", 2)])
def test_poses(pose, name, n):
    """Identity; a neighbour no ego pixel reaches (every wave skips its loads, its logit 0 keeps its share, in `max` it is a zero map)
    and one reached by the first tenth of every row (waves reached in part); an ego row of its own that puts part of the ego's
    sample off the map."""
    worst = Worst("coalign_att", n=n, levels=name, pose=pose)
    fx = fixture(n, name, pose, 5)
    C, H, W = fx["feats"][0].shape[1:]
    rc = R.reached(fx["rows"], H, W)
    if pose == "offmap":
        assert not rc[1].any() and rc[2].any() and not rc[2].all() and rc[0].all()
    if pose == "ego":
        assert not rc[0].all() and rc[0].any()
    for mode in ("att", "max"):
        check(fx, mode, worst, f"{pose} {mode}")
    worst.done()


def test_library_sqrt_dim_device_rows_and_fp32_grid():
    """sqrt_dims left to the library (sqrt(C) in fp32); affine rows read from the device give the bits of the host rows; the sampling
    grid built in fp32 (grid_f64 = False) against the reference on grid_f32."""
    worst = Worst("coalign_att", n=4, levels="small", pose="rot, library sqrt_dim / fp32 grid")
    fx = fixture(4, "small", "rot", 9, False)
    for mode in ("att", "max"):
        host = check(fx, mode, worst, f"host rows {mode}")
        dev = launch(fx, mode, f"device rows {mode}", device_rows=True)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(host, dev)), mode
        check(fx, mode, worst, f"fp32 grid {mode}", grid_f64=False)
    worst.done()


# ======================================================================================================================= exact
@pytest.mark.parametrize("n,C,H,W", R.EQUAL_CASES)
def test_exact_equal_agents(n, C, H, W):
    """Every agent the same integer map under the identity, sqrt_dim = 1/2: p = 1 / n exactly and the output is the map, bit for bit,
    in both modes and both layouts."""
    fx = R.equal_agents(n, C, H, W, seed=n)
    assert fx["units"] < R.EXACT_LIMIT
    one = dict(feats=[fx["feats"]], rows=fx["rows"], sqrt_dims=[fx["sqrt_dim"]])
    for mode in ("att", "max"):
        got, = launch(one, mode, f"equal agents {mode}")
        assert same_bits(got, fx["want"]), mode


@pytest.mark.parametrize("n,C,H,W", R.SELECTOR_CASES)
def test_exact_selector(n, C, H, W):
    """One neighbour is 512 times the ego under the ego's own half-pixel translation, sqrt_dim = 1/4: where the ego's sample is
    non-zero its logit leads by more than 104, expf underflows to 0 and the output is that neighbour's sample bit for bit; where the
    ego's sample is zero every logit is 0 and the output is the mean of the samples (bit for bit when n is a power of two, within
    the bound otherwise)."""
    fx = R.selector(n, C, H, W, seed=n)
    nz, zero, gap = R.selector_masks(fx)
    assert fx["units"] < R.EXACT_LIMIT and gap > R.UNDERFLOW_GAP and nz.any() and zero.any()
    one = dict(feats=[fx["feats"]], rows=fx["rows"], sqrt_dims=[fx["sqrt_dim"]])
    got, = launch(one, "att", "selector")
    s = R.sample_f32(fx["feats"], fx["rows"])
    assert same_bits(got[:, nz], s[fx["chosen"]][:, nz]), "selected pixels"
    ref = R.att_reference(fx["feats"], fx["rows"], fx["sqrt_dim"])
    if n & (n - 1) == 0:
        assert same_bits(got[:, zero], ref["out"][:, zero].astype(np.float32)), "uniform pixels"
    assert R.max_ratio(got[:, zero], ref["out"][:, zero], ref["B"][:, zero]) <= 1.0
    got, = launch(one, "max", "selector max")
    assert same_bits(got, R.max_reference(fx["feats"], fx["rows"]))


# ==================================================================================================================== refusals
def test_outs_are_checked_before_the_launch(monkeypatch):
    z = lambda *s, **k: torch.zeros(s, device=DEV, **k)      # noqa: E731
    feats = [z(2, 4, 8, 8), z(2, 3, 4, 4)]
    rows = np.tile(R.IDENTITY, (2, 1, 1))
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    good = [z(4, 8, 8), z(3, 4, 4)]
    for outs in ([good[0]], good + [z(3, 4, 4)], [good[0], z(3, 4, 5)], [good[0], z(4, 4, 3)], [z(4, 64), good[1]],
                 [good[0].double(), good[1]], [good[0], good[1].cpu()], [z(4, 8, 16)[..., ::2], good[1]], [good[0], good[1].tolist()]):
        with pytest.raises(_capi.HealAmdError):
            ops.warp_att_fuse_levels(feats, rows, outs=outs)
    assert launched == []
    res = ops.warp_att_fuse_levels(feats, rows, outs=good)
    assert res[0] is good[0] and res[1] is good[1] and launched == ["heal_warp_att_fuse_levels"]
