"""heal_comm_mask (ops.comm_mask) on the device against the reference's recordings (tests/golden/w2c_comm_small.npz): every level's
mask, the egos' counts and the rate are compared EXACTLY -- the fixture keeps every smoothed value 1e-4 from the threshold
(tests/golden/w2c_comm_margins.py), more than ten times the worst fp32 accumulation error of the largest filter."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import _capi, ops
from tests.golden import w2c_comm_margins as WM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "w2c_comm_small.npz"))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, psm=None):
    return ops.comm_mask(dev(c["psm"]) if psm is None else psm, c["record_len"], dev(c["weight"]), dev(c["bias"]), c["thre"],
                         c["n_levels"])


@pytest.mark.parametrize("prefix", sorted(WM.MASK_CASES))
def test_masks_counts_and_rate_equal_the_reference(g, prefix):
    c = WM.mask_case(g, prefix)
    masks, count, rate = run(c)
    assert len(masks) == c["n_levels"] and count.dtype == torch.int32 and rate.dtype == torch.float32 and rate.dim() == 0
    H, W = c["psm"].shape[2:]
    for l, m in enumerate(masks):
        want = g[f"{prefix}mask{l}"]
        assert tuple(m.shape) == want.shape == (5, 1, H >> l, W >> l) and m.dtype == torch.float32
        assert np.array_equal(m.cpu().numpy(), want.astype(np.float32)), (prefix, l)
        if l:                                                    # levels >= 1 are max_pool2d of level 0, applied l times
            pooled = masks[0]
            for _ in range(l):
                pooled = F.max_pool2d(pooled, kernel_size=2)
            assert torch.equal(m, pooled), (prefix, l)
    assert count.cpu().tolist() == g[prefix + "count"].tolist()
    assert np.float32(rate.item()) == g[prefix + "rate"]
    again = run(c)                                               # two launches: the same bits
    assert all(torch.equal(a, b) for a, b in zip(masks, again[0])) and torch.equal(count, again[1])
    assert rate.view(torch.int32).item() == again[2].view(torch.int32).item()


def test_a_list_and_a_tensor_record_len_and_a_conv_shaped_weight(g):
    """The module's own parameters as they lie in the state_dict: weight [1, 1, k, k]; record_len as a CPU tensor."""
    c = WM.mask_case(g, "par_")
    masks, count, rate = ops.comm_mask(dev(c["psm"]), torch.tensor(c["record_len"]), dev(c["weight"]).view(1, 1, 5, 5), dev(c["bias"]),
                                       c["thre"], 3)
    assert np.array_equal(masks[0].cpu().numpy(), g["par_mask0"].astype(np.float32)) and count.cpu().tolist() == g["par_count"].tolist()
    # the parameters are read: the default filter gives another mask on these logits
    other, _, _ = ops.comm_mask(dev(c["psm"]), c["record_len"], dev(WM.gaussian_weight(5, 1.0)), dev(np.zeros(1, np.float32)), c["thre"], 3)
    assert not torch.equal(other[0], masks[0])


def test_replay_in_a_captured_graph_reads_the_new_logits(g):
    """Captured once, replayed after the logits AND the filter were overwritten in place: the replay equals the eager call on the
    new contents (kernel launches only, no host synchronisation, the parameters read from device memory at run time)."""
    c, d = WM.mask_case(g, "odd_"), WM.mask_case(g, "par_")
    psm, w, b = dev(c["psm"]), dev(c["weight"]), dev(c["bias"])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ops.comm_mask(psm, c["record_len"], w, b, c["thre"], 3)                   # warm-up: the workspace exists before the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            masks, count, rate = ops.comm_mask(psm, c["record_len"], w, b, c["thre"], 3)
        graph.replay()
        st.synchronize()
        assert np.array_equal(masks[0].cpu().numpy(), g["odd_mask0"].astype(np.float32))
        psm.copy_(dev(d["psm"]))
        w.copy_(dev(d["weight"]))
        b.copy_(dev(d["bias"]))
        graph.replay()
        st.synchronize()
        eager = ops.comm_mask(psm, c["record_len"], w, b, c["thre"], 3)
        st.synchronize()
    assert all(torch.equal(a, e) for a, e in zip(masks, eager[0])) and torch.equal(count, eager[1]) and torch.equal(rate, eager[2])
    assert not np.array_equal(masks[0].cpu().numpy(), g["odd_mask0"].astype(np.float32))


def test_bad_arguments_raise_before_anything_is_launched(g, monkeypatch):
    c = WM.mask_case(g, "odd_")
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    psm, w, b = dev(c["psm"]), dev(c["weight"]), dev(c["bias"])
    E = _capi.HealAmdError
    bad = [
        lambda: ops.comm_mask(psm, [3, 2], torch.zeros((4, 4), device=DEV), b, 0.5, 3),                 # even k
        lambda: ops.comm_mask(psm, [3, 2], torch.zeros((11, 11), device=DEV), b, 0.5, 3),               # k above HEAL_COMM_MAX_K
        lambda: ops.comm_mask(psm.cpu(), [3, 2], w, b, 0.5, 3),                                         # a CPU tensor
        lambda: ops.comm_mask(psm, [3, 2], w.cpu(), b, 0.5, 3),
        lambda: ops.comm_mask(psm, [3, 3], w, b, 0.5, 3),                                               # record_len sums to 6
        lambda: ops.comm_mask(psm, [5, 0], w, b, 0.5, 3),                                               # an empty scene
        lambda: ops.comm_mask(psm, [3, 2], w, None, 0.5, 3),                                            # a weight without a bias
        lambda: ops.comm_mask(psm, [3, 2], torch.zeros((3, 5), device=DEV), b, 0.5, 3),                 # not square
        lambda: ops.comm_mask(psm, [3, 2], w, b, 0.5, 0),                                               # levels out of range
        lambda: ops.comm_mask(psm, [3, 2], w, b, 0.5, ops.WARP_MAX_LEVELS + 1),
        lambda: ops.comm_mask(psm.double(), [3, 2], w, b, 0.5, 3),
        lambda: ops.comm_mask(psm[0], [1], w, b, 0.5, 1),                                               # not [n, A, H, W]
    ]
    for i, f in enumerate(bad):
        with pytest.raises(E):
            f()
        assert launched == [], i
    assert ops.COMM_MAX_K == 9
