"""Cases and margins of tests/golden/w2c_comm_small.npz, shared by the generator (gen_golden_w2c_comm.py, which asserts them on what
it writes) and the tests (which assert them on what they read).

A communication mask is a comparison `s > thre`; a smoothed value that sits on the threshold would make the mask depend on the
rounding of an fp32 accumulation, not on the arithmetic.  The smoothed values lie in (0, 1) and the worst fp32 accumulation error of
81 taps is a few 1e-6, so every smoothed value of a fixture -- evaluated in float64 (tests/comm_refs.py) -- keeps at least MARGIN =
1e-4 from the threshold: more than a factor of 10.  The generator nudges the logits of pixels that break this.

Mask cases (prefix -> settings); all have record_len [3, 2], so that the even-agent override restarts in the second scene (global
agents 0, 2 | 3 are forced, 1 | 4 are not):
  odd_   13 x 11, 3 levels: 13 -> 6 -> 3 and 11 -> 5 -> 2, the floor drops a row and a column; no tile multiple, H != W; A = 2; k = 5
  tiny_  3 x 2: smaller than the filter radius (k = 7); 2 levels (3 -> 1, 2 -> 1); A = 1
  one_   1 x 1; k = 3; A = 2
  k1_, k3_, k7_   13 x 11 with the other filter sizes; A = 1, 2, 1
  raw_   no smoothing (a config without `gaussian_smooth`); A = 2
  par_   a perturbed filter weight and bias 0.05: the parameters are read, not recomputed
  ext_   logits of +-30 on a tenth of the pixels
  big_   45 x 38: more than one 32 x 32 tile on both axes, the largest filter (k = 9) across the tile borders, 4 levels; A = 1
"""
import numpy as np

from tests import comm_refs as CR

MARGIN = 1e-4
RECORD_LEN = [3, 2]
FORCED, FREE = (0, 2, 3), (1, 4)           # global agents with an even / odd index within their scene
# prefix -> (H, W, A, k (0: no smoothing), n_levels)
MASK_CASES = {
    "odd_": (13, 11, 2, 5, 3),
    "tiny_": (3, 2, 1, 7, 2),
    "one_": (1, 1, 2, 3, 1),
    "k1_": (13, 11, 1, 1, 3),
    "k3_": (13, 11, 2, 3, 3),
    "k7_": (13, 11, 1, 7, 3),
    "raw_": (13, 11, 2, 0, 3),
    "par_": (13, 11, 2, 5, 3),
    "ext_": (13, 11, 2, 5, 3),
    "big_": (45, 38, 1, 9, 4),
}
# module cases: prefix -> (agg_operator.mode, multi_scale, backbone form | None)
MODULE_CASES = {
    "att_ss_": ("ATTEN", False, None), "att_plain_": ("ATTEN", True, "plain"), "att_res_": ("ATTEN", True, "resnet"),
    "max_ss_": ("MAX", False, None), "max_plain_": ("MAX", True, "plain"), "max_res_": ("MAX", True, "resnet"),
}
MODULE_HW, MODULE_C, MODULE_RANGE_M, MODULE_VOXEL = 32, 8, 25.6, 0.8       # a 32 x 32 map of 0.8 m cells: +-12.8 m
MODEL_KEYS = ("cls_preds", "reg_preds", "bbox_preds", "cls_preds_single", "reg_preds_single", "bbox_preds_single", "comm_rate")


def gaussian_weight(k, sigma):
    """comm_modules/where2comm.py:24-29 as float32 [k, k]."""
    c = k // 2
    x, y = np.mgrid[0 - c:k - c, 0 - c:k - c]
    return (1 / (2 * np.pi * sigma) * np.exp(-(np.square(x) + np.square(y)) / (2 * np.square(sigma)))).astype(np.float32)


def mask_case(g, prefix):
    """The inputs of a mask case from the fixture."""
    H, W, A, k, levels = MASK_CASES[prefix]
    c = dict(psm=g[prefix + "psm"], thre=float(g[prefix + "thre"]), n_levels=levels, record_len=list(RECORD_LEN), k=k,
             weight=g[prefix + "weight"] if k else None, bias=g[prefix + "bias"] if k else None)
    assert c["psm"].shape == (sum(RECORD_LEN), A, H, W)
    return c


def chain(c):
    return CR.mask_chain(c["psm"], c["record_len"], c["weight"], 0.0 if c["bias"] is None else c["bias"], c["thre"], c["n_levels"])


def is_mixed(raw, prefix):
    """Both zeros and ones in every agent that is not forced -- with one pixel per agent (one_): across those agents."""
    free = raw[list(FREE)]
    if free[0].size == 1:
        return bool(free.min() == 0 and free.max() == 1)
    return all(bool(m.min() == 0 and m.max() == 1) for m in free)


def pick_threshold(s):
    """The middle of the widest gap between neighbouring smoothed values of the free agents, among their upper-middle part (so
    that a minority of the cells is sent and the pooled levels keep zeros)."""
    v = np.sort(s[list(FREE)].reshape(-1))
    if v.size == 2:
        return float(0.5 * (v[0] + v[1]))
    lo = v.size * 7 // 10
    hi = max(v.size * 9 // 10, lo + 2)                                   # between the 70th and the 90th percentile
    mid = v[lo:hi]
    i = int(np.argmax(np.diff(mid)))
    return float(0.5 * (mid[i] + mid[i + 1]))


HEAD_GAIN, HEAD_BIAS = 512.0, 132.3


def model_fill(model):
    """detfill.fill_module, then the score head's weight times HEAD_GAIN and its bias HEAD_BIAS: the closed-form fill leaves the
    confidence logits of the model case within 0.01 of each other, and the masks would follow the filter's response to the map
    border instead of the features.  With the gain the logits spread by about 0.7 around -132.3, which the bias centres."""
    import torch
    from tests.golden.detfill import fill_module
    fill_module(model)
    with torch.no_grad():
        model.cls_head.weight.mul_(HEAD_GAIN)
        model.cls_head.bias.fill_(HEAD_BIAS)
    return model
