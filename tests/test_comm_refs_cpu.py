"""tests/comm_refs.py -- the float64 restatement of Where2comm's mask chain and of "premultiply, then fuse" -- against the reference's
recordings (tests/golden/w2c_comm_small.npz) and against torch on the CPU.  The GPU suites compare the kernels with these
restatements; here the restatements themselves are pinned.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import coalign_refs as R
from tests import comm_refs as CR
from tests.golden import w2c_comm_margins as WM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "w2c_comm_small.npz"))


@pytest.mark.parametrize("prefix", sorted(WM.MASK_CASES))
def test_mask_chain_equals_the_recorded_reference(g, prefix):
    c = WM.mask_case(g, prefix)
    ch = WM.chain(c)
    for l in range(c["n_levels"]):
        assert np.array_equal(ch["masks"][l], g[f"{prefix}mask{l}"][:, 0]), (prefix, l)
    assert ch["count"].tolist() == g[prefix + "count"].tolist()
    assert ch["rate"] == g[prefix + "rate"] and ch["rate"].dtype == np.float32


@pytest.mark.parametrize("prefix", sorted(WM.MASK_CASES))
def test_fixture_keeps_its_margin_and_is_mixed(g, prefix):
    c = WM.mask_case(g, prefix)
    ch = WM.chain(c)
    print(prefix, "margin", ch["margin"], "ones", ch["raw"].mean())
    assert ch["margin"] >= WM.MARGIN
    assert WM.is_mixed(ch["raw"], prefix)
    forced = g[prefix + "mask0"][list(WM.FORCED)]
    assert forced.min() == 1                                                  # agents 0, 2 of scene 0 and agent 0 of scene 1
    if c["k"]:
        assert 0 < ch["s"].min() and (prefix == "par_" or ch["s"].max() < 1)   # smoothed values in (0, 1): what MARGIN is sized for


def test_fixture_holds_the_cases_it_names(g):
    assert [g[f"odd_mask{l}"].shape[2:] for l in range(3)] == [(13, 11), (6, 5), (3, 2)]
    assert g["tiny_mask1"].shape[2:] == (1, 1) and g["one_mask0"].shape[2:] == (1, 1) and g["big_mask3"].shape[2:] == (5, 4)
    assert np.abs(g["ext_psm"]).max() == 30 and (g["ext_psm"] == -30).any() and (g["ext_psm"] == 30).any()
    assert g["par_bias"][0] == np.float32(0.05) and not np.array_equal(g["par_weight"], WM.gaussian_weight(5, 1.0))
    for prefix, (_, _, _, k, _) in WM.MASK_CASES.items():
        if k and prefix != "par_":
            assert np.array_equal(g[prefix + "weight"], WM.gaussian_weight(k, 1.0)) and g[prefix + "bias"][0] == 0
    assert "raw_weight" not in g.files
    for prefix in ("odd_", "big_"):                                           # the coarsest level is not all ones
        top = g[f"{prefix}mask{WM.MASK_CASES[prefix][4] - 1}"][list(WM.FREE)]
        assert 0 < top.mean() < 1
    # the override restarts per scene: global agent 3 (index 0 of scene 1) is forced, global agent 4 is not
    assert g["odd_mask0"][3].min() == 1 and g["odd_mask0"][4].min() == 0 and g["odd_mask0"][1].min() == 0


@pytest.mark.parametrize("prefix", ["odd_", "big_", "tiny_", "raw_"])
def test_mask_chain_equals_torch(g, prefix):
    """The same chain from torch's own operators in fp32: sigmoid, max, conv2d, comparison, max_pool2d."""
    c = WM.mask_case(g, prefix)
    x = torch.from_numpy(c["psm"]).sigmoid().max(dim=1, keepdim=True)[0]
    if c["k"]:
        k = c["k"]
        x = F.conv2d(x, torch.from_numpy(c["weight"]).view(1, 1, k, k), torch.from_numpy(c["bias"]), padding=(k - 1) // 2)
    m = (x > c["thre"]).float()
    ch = WM.chain(c)
    assert np.array_equal(m.numpy()[:, 0].astype(np.uint8), ch["raw"])
    assert float(np.abs(x.numpy()[:, 0] - ch["s"]).max()) < 1e-5
    start = 0
    for n in c["record_len"]:
        m[start:start + n:2] = 1
        start += n
    for l in range(c["n_levels"]):
        assert np.array_equal(m.numpy()[:, 0].astype(np.uint8), ch["masks"][l])
        if l + 1 < c["n_levels"]:
            m = F.max_pool2d(m, kernel_size=2)


def test_pooling_nests():
    """Floor-mode 2 x 2 pooling repeated l times is the maximum over the 2^l x 2^l square: no level depends on another."""
    rng = np.random.default_rng(3)
    m = (rng.random((2, 45, 38)) < 0.05).astype(np.uint8)
    direct = CR.pool_levels(m, 4)
    t = torch.from_numpy(m).float().unsqueeze(1)
    for l in range(4):
        assert np.array_equal(direct[l], t.numpy()[:, 0].astype(np.uint8)), l
        t = F.max_pool2d(t, 2)


@pytest.mark.parametrize("mode", ["att", "max"])
def test_premultiply_then_fuse_equals_torch(mode):
    """masked_att / masked_max against warp_affine_simple + the per-pixel attention (or maximum) of torch on x * mask."""
    rng = np.random.default_rng(11)
    n, C, H, W = 3, 6, 9, 7
    feats = R.random_feats(n, C, H, W, 5)
    masks = (rng.random((n, 1, H, W)) < 0.6).astype(np.float32)
    rows = R.poses("rot", n, 4)
    xm = torch.from_numpy(CR.premultiply(feats, masks))
    grid = F.affine_grid(torch.from_numpy(rows), [n, C, H, W], align_corners=False).to(xm)
    ego = F.grid_sample(xm, grid, align_corners=False)
    if mode == "max":
        want, got = ego.max(0)[0].numpy(), CR.masked_max(feats, masks, rows)
    else:
        t = ego.view(n, C, -1).permute(2, 0, 1)
        sd = R.f32_sqrt_dim(C)
        want = torch.bmm(torch.softmax(torch.bmm(t, t.transpose(1, 2)) / sd, -1), t).permute(1, 2, 0).view(n, C, H, W)[0].numpy()
        got = CR.masked_att(feats, masks, rows)["out"]
    assert float(np.abs(got - want).max()) <= 1e-5 * max(1.0, float(np.abs(want).max()))
    assert float(np.abs(got - (CR.masked_max(feats, np.ones_like(masks), rows) if mode == "max"
                               else CR.masked_att(feats, np.ones_like(masks), rows)["out"])).max()) > 1e-3      # the mask matters
