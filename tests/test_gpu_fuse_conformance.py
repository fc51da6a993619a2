"""The two single-level warp + fuse kernels element by element: k_disco_fuse<n> (heal_amd/csrc/disco_fuse.hip, DiscoNet) and
k_warp_mha_fuse<n> (heal_amd/csrc/warp_mha.hip, Where2comm) for n = 1..8 under rotations, at the kernels' own channel, head and
map boundaries, with agents out of reach of every wave and of part of the waves, an ego row of its own, and logits more than 104
apart.

Every assertion is one of: the per-element bound |got - ref| <= SAFETY * EPS * (k * T + E) + TINY against the float64 reference of
tests/fuse_refs.py (k, T and E derived there from the kernels' statements, disco_k / mha_k; proven against the modules' float64
torch arithmetic, and proven to have teeth, in tests/test_fuse_refs_cpu.py); equality of fp32 values with the kernels' own sampling
arithmetic repeated in numpy (ego_warped; every output of one agent; the pixels of the large-logit fixtures that one agent
dominates); or equality of bits between two launches.  Nothing is normalised by a tensor-wide maximum.  Every operand lies inside a
NaN-poisoned buffer and every output is NaN-prefilled inside one: a tap of weight 0 and a clamped channel must still read inside the
operand (NaN * 0 would show), every output word must have been written, and no word outside may change.  DiscoNet's logits
(`scores`) are formed from phase 1's taps and its output from phase 2's: both are held to the same reference.

A behaviour that differs from the reference on purpose: a tap outside the map is multiplied by 0 instead of skipped, so a
non-finite value at element 0 of a feature plane reaches pixels whose taps all lie outside the map.  Inputs here are finite."""
import numpy as np
import pytest
import torch

from heal_amd import _capi, ops
from tests import fuse_refs as R
from tests.test_gpu_attention_conformance import Operands, Worst

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def same(a, b):
    """Equal as fp32 values (-0 == +0: a tap of weight 0 has the sign of whichever finite word it was multiplied with)."""
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a, np.float32)), torch.from_numpy(np.ascontiguousarray(b, np.float32)))


def bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def _rows(fx, device_rows):
    return torch.from_numpy(fx["rows"]).to(DEV) if device_rows else fx["rows"]


_FRAGS = {}


def w1n_fragments(name):
    """ops.mfma_a_fragments of the case's W1n as a host array (the launch puts it behind guards like every other operand)."""
    if name not in _FRAGS:
        _FRAGS[name] = ops.mfma_a_fragments(torch.from_numpy(R.disco_fixture(name)["w1n"]).to(DEV)).cpu().numpy()
    return _FRAGS[name]


def launch_disco(name, what, grid_f64=True, device_rows=False, bare=False, hook=True):
    """One launch into poisoned destinations -> (out [C, H, W], scores [n, H, W] or None) float32 numpy.  bare: one agent without the
    PixelWeightLayer operands; hook False: without return_scores."""
    fx = R.disco_fixture(name)
    op = Operands()
    feats = op.put(fx["feats"])
    out = op.out((fx["C"], fx["H"], fx["W"]))
    with torch.no_grad():
        if bare:
            res = ops.disco_fuse(feats, _rows(fx, device_rows), grid_f64, *([None] * 8), out=out)
            scores = None
        else:
            args = [op.put(fx["e0"]), op.put(w1n_fragments(name))] + [op.put(fx[o]) for o in R.DISCO_OPERANDS[3:]]
            scores = op.out((fx["n"], fx["H"], fx["W"])) if hook else None
            res = ops.disco_fuse(feats, _rows(fx, device_rows), grid_f64, *args, return_scores=hook, out=out, scores=scores)
            if hook:
                assert res[1].data_ptr() == scores.data_ptr()
                res = res[0]
    assert res.data_ptr() == out.data_ptr()
    op.check(what)
    return out.cpu().numpy(), None if scores is None else scores.cpu().numpy()


def launch_mha(name, what, grid_f64=True, device_rows=False, logits=True):
    """One launch into poisoned destinations -> (ctx, ego_warped [C, H, W], logits [n, heads, H, W] or None) float32 numpy."""
    fx = R.mha_fixture(name)
    op = Operands()
    args = [op.put(fx[o]) for o in R.MHA_OPERANDS]
    shape = (fx["C"], fx["H"], fx["W"])
    outs = (op.out(shape), op.out(shape))
    lg = op.out((fx["n"], fx["heads"], fx["H"], fx["W"])) if logits else None
    with torch.no_grad():
        res = ops.warp_mha_fuse(*args, fx["heads"], _rows(fx, device_rows), grid_f64, fx["scale"], return_logits=logits, outs=outs,
                                logits=lg)
    assert len(res) == 2 + logits and all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs + ((lg,) if logits else ())))
    op.check(what)
    return outs[0].cpu().numpy(), outs[1].cpu().numpy(), lg.cpu().numpy() if logits else None


def check_disco(name, worst, tag, grid_f64=True, got=None):
    """out and scores within the bound of the full reference, and out within the much narrower bound of the softmax-and-sum of the
    kernel's own scores (recorded); one agent: the sample itself."""
    out, scores = launch_disco(name, tag, grid_f64) if got is None else got
    fx, ref = R.disco_fixture(name), R.disco_ref(name, grid_f64)
    worst.add("out", R.max_ratio(out, ref["out"], ref["B"]), f"{tag} {name}")
    worst.add("scores", R.max_ratio(scores, ref["logit"], ref["B_logit"]), f"{tag} {name}")
    own, B_own = R.disco_out_given_scores(fx["feats"], scores, fx["rows"], grid_f64)
    worst.add("out_given_scores", R.max_ratio(out, own, B_own), f"{tag} {name}")      # phase 2 alone, on the kernel's own logits
    if fx["n"] == 1:
        assert same(out, R.sample_f32(fx["feats"], fx["rows"], grid_f64)[0]), (tag, name, "one agent")
    return out, scores


def check_mha(name, worst, tag, grid_f64=True, got=None):
    """ctx and logits within the bound (recorded), ego_warped the sample itself; one agent: ctx = S_0(v_map) + bv bit for bit."""
    ctx, ego, logits = launch_mha(name, tag, grid_f64) if got is None else got
    fx, ref = R.mha_fixture(name), R.mha_ref(name, grid_f64)
    worst.add("ctx", R.max_ratio(ctx, ref["ctx"], ref["B_ctx"]), f"{tag} {name}")
    worst.add("logits", R.max_ratio(logits, ref["logits"], ref["B_logits"]), f"{tag} {name}")
    assert same(ego, ref["ego_warped"]), (tag, name, "ego_warped")
    if fx["n"] == 1:
        v = R.sample_f32(fx["kv_map"][:, fx["C"]:], fx["rows"], grid_f64)[0]
        assert same(ctx, (v + fx["bv"][:, None, None]).astype(np.float32)), (tag, name, "one agent")
    return ctx, ego, logits


# ========================================================================================================== every instantiation
@pytest.mark.parametrize("n", range(1, 9))
def test_disco_fuse_every_agent_count(n):
    """k_disco_fuse<n> on a 13 x 21 map under rotations with taps off every border (n = 1: the ego under a rotation of its own): the
    sampling grid in float64 and in fp32, rows from the host and from the device (the same bits), two launches (the same bits), with
    and without the `scores` hook (the same output bits); one agent with and without the PixelWeightLayer operands."""
    name = f"n{n}"
    worst = Worst("disco_fuse", n=n, case=name)
    for grid_f64 in (True, False):
        got = check_disco(name, worst, f"grid_f64={grid_f64}", grid_f64)
        again = launch_disco(name, "again", grid_f64)
        dev = launch_disco(name, "device rows", grid_f64, device_rows=True)
        assert all(bits(a, b) for a, b in zip(got, again)), "two launches differ"
        assert all(bits(a, b) for a, b in zip(got, dev)), "device rows differ from host rows"
        assert bits(got[0], launch_disco(name, "no scores", grid_f64, hook=False)[0]), "the scores hook changes the output"
        if n == 1:
            bare, _ = launch_disco(name, "bare", grid_f64, bare=True)
            assert bits(bare, got[0]), "one agent: the PixelWeightLayer operands change the output"
    worst.done()


@pytest.mark.parametrize("n", range(1, 9))
def test_warp_mha_fuse_every_agent_count(n):
    """k_warp_mha_fuse<n> likewise; without the `logits` hook the outputs keep their bits."""
    name = f"n{n}"
    worst = Worst("warp_mha_fuse", n=n, case=name)
    for grid_f64 in (True, False):
        got = check_mha(name, worst, f"grid_f64={grid_f64}", grid_f64)
        again = launch_mha(name, "again", grid_f64)
        dev = launch_mha(name, "device rows", grid_f64, device_rows=True)
        plain = launch_mha(name, "no logits", grid_f64, logits=False)
        assert all(bits(a, b) for a, b in zip(got, again)), "two launches differ"
        assert all(bits(a, b) for a, b in zip(got, dev)), "device rows differ from host rows"
        assert bits(got[0], plain[0]) and bits(got[1], plain[1]), "the logits hook changes the outputs"
    worst.done()


# ======================================================================================================================= poses
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("pose", ["identity", "offmap", "ego"])
def test_disco_fuse_poses(pose, n):
    """Identity; a neighbour no ego pixel reaches (every block skips its loads: its logit is the MLP of E0 alone and keeps its share)
    and one reached by part of the waves; an ego row of its own that puts part of the ego's own-map term off the map."""
    name = f"{pose}{n}"
    fx = R.disco_fixture(name)
    worst = Worst("disco_fuse", n=n, case=name)
    out, scores = check_disco(name, worst, pose)
    if pose == "offmap":
        rc = R.reached(fx["rows"], fx["H"], fx["W"])
        assert not rc[1].any() and rc[2].any() and not rc[2].all()
        assert float(R.disco_ref(name)["p"][1].mean()) > 0.05         # the absent agent holds its share of the softmax
    worst.done()


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("pose", ["identity", "offmap", "ego"])
def test_warp_mha_fuse_poses(pose, n):
    """As above; the absent agent's logit is scale * q . bk, and part of ego_warped and of q is sampled off the map under `ego`."""
    name = f"{pose}{n}"
    fx = R.mha_fixture(name)
    worst = Worst("warp_mha_fuse", n=n, case=name)
    ctx, ego, logits = check_mha(name, worst, pose)
    rc = R.reached(fx["rows"], fx["H"], fx["W"])
    if pose == "offmap":
        assert not rc[1].any() and float(R.mha_ref(name)["p"][1].mean()) > 0.05
    if pose == "ego":
        assert not rc[0].all() and same(ego[:, ~rc[0]], np.zeros_like(ego[:, ~rc[0]]))
    worst.done()


# ======================================================================================================= channel, head and map edges
@pytest.mark.parametrize("C", R.DISCO_CHANNELS)
def test_disco_fuse_channel_edges(C):
    """One MFMA k-step and one channel per wave in phase 2 (4); 8; a chunk tail (28); exactly one staging chunk (32); 36; two chunks
    and one k-step (68) -- 5 x 17: one pixel into a second tile on both axes."""
    worst = Worst("disco_fuse", n=3, case=f"C{C}")
    check_disco(f"C{C}", worst, "channels")
    worst.done()


@pytest.mark.parametrize("C,heads", R.MHA_HEADS)
def test_warp_mha_fuse_head_edges(C, heads):
    """d = 1 with heads = C; an odd d (the tail of the channel sweeps unrolled by 2); one head; d = 16."""
    worst = Worst("warp_mha_fuse", n=3, case=f"C{C}x{heads}")
    check_mha(f"C{C}x{heads}", worst, "heads")
    worst.done()


@pytest.mark.parametrize("H,W", R.MAPS)
def test_map_edges(H, W):
    """1 x 1; exactly one 16 x 4 tile; one pixel into a second tile on both axes; smaller than a tile; ten tiles high and narrower
    than one."""
    for kernel, check in (("disco_fuse", check_disco), ("warp_mha_fuse", check_mha)):
        worst = Worst(kernel, n=3, case=f"{H}x{W}")
        check(f"{H}x{W}", worst, "map")
        worst.done()


# ================================================================================================================ large logits
def test_disco_fuse_large_logits():
    """w4 times 256: logits up to several hundred.  Outputs finite and within the bound; where one agent leads every other by more
    than 104, expf underflows to 0 and the output is that agent's sample: within the bound with T of that agent alone, and equal to
    the fp32 sample."""
    worst = Worst("disco_fuse", n=4, case="large")
    out, scores = check_disco("large", worst, "large")
    fx, ref = R.disco_fixture("large"), R.disco_ref("large")
    dom, who = R.dominated(ref["logit"])
    assert dom.mean() > 0.1 and np.isfinite(out).all() and np.isfinite(scores).all()
    assert float((np.sort(scores, 0)[-1] - np.sort(scores, 0)[-2])[dom].min()) > R.UNDERFLOW_GAP
    x, xa = R.sample_f64(fx["feats"], fx["rows"])
    pick = lambda t: np.take_along_axis(t, who[None, None], 0)[0][:, dom]      # noqa: E731
    worst.add("out_dominated", R.max_ratio(out[:, dom], pick(x), R.SAFETY * R.EPS * ref["k"]["out"] * pick(xa)), "large")
    assert same(out[:, dom], pick(R.sample_f32(fx["feats"], fx["rows"])))
    worst.done()


def test_warp_mha_fuse_large_logits():
    """The last agent's K map times 256: per head its logit leads or trails by hundreds.  Where one agent leads by more than 104 the
    context is that agent's v = S(v_map) + bv: within the bound with T of that agent alone, and equal to the fp32 value."""
    worst = Worst("warp_mha_fuse", n=4, case="large")
    ctx, ego, logits = check_mha("large", worst, "large")
    fx, ref = R.mha_fixture("large"), R.mha_ref("large")
    C, heads, H, W = fx["C"], fx["heads"], fx["H"], fx["W"]
    d = C // heads
    dom, who = R.dominated(ref["logits"])                                              # [heads, H, W]
    assert dom.mean() > 0.1 and np.isfinite(ctx).all() and np.isfinite(logits).all()
    assert float((np.sort(logits, 0)[-1] - np.sort(logits, 0)[-2])[dom].min()) > R.UNDERFLOW_GAP
    dom_c, who_c = np.repeat(dom, d, 0), np.repeat(who, d, 0)                          # per channel: head c // d
    v64, va = R.sample_f64(fx["kv_map"][:, C:], fx["rows"])
    bv = fx["bv"].astype(np.float64)[None, :, None, None]
    pick = lambda t: np.take_along_axis(t, who_c[None], 0)[0][dom_c]      # noqa: E731
    worst.add("ctx_dominated", R.max_ratio(ctx[dom_c], pick(v64 + bv), R.SAFETY * R.EPS * ref["k"]["out"] * pick(va + np.abs(bv))), "large")
    v32 = (R.sample_f32(fx["kv_map"][:, C:], fx["rows"]) + fx["bv"][None, :, None, None]).astype(np.float32)
    assert same(ctx[dom_c], pick(v32))
    worst.done()


# ==================================================================================================================== refusals
def test_destinations_are_checked_before_the_launch(monkeypatch):
    z = lambda *s, **k: torch.zeros(s, device=DEV, **k)      # noqa: E731
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    n, C, heads, H, W = 2, 8, 2, 4, 8
    rows = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 1, 1))
    bad = lambda *shape: [z(*shape[:-1], shape[-1] + 1), z(*shape).double(), z(*shape).cpu(), z(*shape[:-1], 2 * shape[-1])[..., ::2],      # noqa: E731
                          z(*shape).tolist()]
    disco = [z(n, C, H, W), rows, True, z(128, H, W), ops.mfma_a_fragments(z(128, C)), z(32, 128), z(32), z(8, 32), z(8), z(8), z(1)]
    for out in bad(C, H, W):
        with pytest.raises(_capi.HealAmdError):
            ops.disco_fuse(*disco, out=out)
    for scores in bad(n, H, W):
        with pytest.raises(_capi.HealAmdError):
            ops.disco_fuse(*disco, return_scores=True, scores=scores)
    with pytest.raises(_capi.HealAmdError):
        ops.disco_fuse(*disco, scores=z(n, H, W))                      # `scores` without return_scores
    mha = [z(C, H, W), z(n, 2 * C, H, W), z(C, H, W), z(C), z(C), z(C), heads, rows]
    for o in bad(C, H, W):
        for outs in ((o, z(C, H, W)), (z(C, H, W), o)):
            with pytest.raises(_capi.HealAmdError):
                ops.warp_mha_fuse(*mha, outs=outs)
    for outs in ((z(C, H, W),), z(C, H, W), (z(C, H, W),) * 3):
        with pytest.raises(_capi.HealAmdError):
            ops.warp_mha_fuse(*mha, outs=outs)
    for lg in bad(n, heads, H, W):
        with pytest.raises(_capi.HealAmdError):
            ops.warp_mha_fuse(*mha, return_logits=True, logits=lg)
    with pytest.raises(_capi.HealAmdError):
        ops.warp_mha_fuse(*mha, logits=z(n, heads, H, W))
    assert launched == []
    out, scores = z(C, H, W), z(n, H, W)
    res = ops.disco_fuse(*disco, return_scores=True, out=out, scores=scores)
    outs, lg = (z(C, H, W), z(C, H, W)), z(n, heads, H, W)
    res2 = ops.warp_mha_fuse(*mha, return_logits=True, outs=outs, logits=lg)
    assert res[0] is out and res[1] is scores and res2[0] is outs[0] and res2[1] is outs[1] and res2[2] is lg
    assert launched == ["heal_disco_fuse", "heal_warp_mha_fuse"]
