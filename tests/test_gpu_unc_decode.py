"""heal_decode_nms_agents_unc, UncertaintyVoxelPostprocessor.post_process on it, and the PointPillarUncertainty forward, on the
MI355X.  The pooled decode + NMS is heal_decode_nms_agents' (its own tests hold it to the reference): here corners, scores and
count must be ITS bits, and the new outputs -- the pooled anchor index of every kept box and the uncertainty channels gathered
at it -- are checked exactly against maps that store their own location."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heal_amd import configs, ops, synth
from heal_amd.opencood.data_utils.post_processor.uncertainty_voxel_postprocessor import UncertaintyVoxelPostprocessor
from heal_amd.opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
from heal_amd.opencood.models.point_pillar import PointPillar
from heal_amd.opencood.tools import train_utils
from oracle import cref
from tests.golden import late_margins as M
from tests.golden.detfill import fill_module

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULTS = (0.2, 0.7853, 2, 0.15)          # score threshold, dir_offset, num_bins, nms_thresh of the HEAL YAMLs
GT_RANGE = [-16.0, -16.0, -3.0, 16.0, 16.0, 1.0]
SIZES = [(12, 16), (9, 11)]
POSES = [[0, 0, 0, 0, 0, 0], [3.0, -2.0, 0.1, 0.0, 25.0, 0.0], [-4.0, 5.0, -0.2, 0.3, -70.0, 0.2], [6.0, 6.0, 0.05, -0.4, 140.0, 0.3],
         [-7.0, -3.0, 0.15, 0.2, 200.0, -0.3], [2.0, 7.0, 0.0, 0.0, 80.0, 0.0], [-6.0, 1.0, 0.1, 0.0, -150.0, 0.0],
         [5.0, -6.0, -0.1, 0.0, 310.0, 0.0]]


def anchors_for(H, W):
    r = [-W * 0.4, -H * 0.4, -3, W * 0.4, H * 0.4, 1]
    p = configs.m1_late(r)["postprocess"]
    p["anchor_args"].update({"W": 2 * W, "H": 2 * H, "cav_lidar_range": r})
    a = VoxelPostprocessor(p, train=False).generate_anchor_box()
    assert a.shape == (H, W, 2, 7)
    return a


def location_map(k, dim, A, H, W):
    """An uncertainty map whose every element is its own flat location (+ the agent), exact in float32."""
    v = torch.arange(dim * A * H * W, dtype=torch.float32).view(1, dim * A, H, W) + 100000.0 * k
    assert float(v.max()) < 2 ** 24
    return v


def scene(n, dim, seed, sizes=SIZES, clusters=6, mode="normal", lo=0.25, hi=0.95):
    rng = np.random.default_rng(seed)
    cavs = []
    for k in range(n):
        H, W = sizes[k % len(sizes)]
        c = M.make_cav(rng, anchors_for(H, W), synth.x_to_world(POSES[k]), clusters, mode)
        c["unc"] = location_map(k, dim, 2, H, W).numpy()
        cavs.append(c)
    M.deal_ladder(rng, cavs, lo=lo, hi=hi)
    return cavs


def on_device(cavs):
    return [{k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV) for k, v in c.items() if not k.startswith("_")}
            for c in cavs]


def both(cavs, top=1000, gt_range=GT_RANGE):
    """(decode_nms_agents, decode_nms_agents_unc) on the same device tensors, no host synchronisation inside."""
    d = on_device(cavs)
    lists = [[c[k] for c in d] for k in ("cls", "reg", "dir", "anchors")]
    tfms = torch.stack([c["tfm"] for c in d])
    base = ops.decode_nms_agents(*lists, tfms, *DEFAULTS, gt_range, nms_top=top, sync=False, want_agent=True)
    unc = ops.decode_nms_agents_unc(*lists, [c["unc"] for c in d], tfms, *DEFAULTS, gt_range, nms_top=top, sync=False,
                                    want_agent=True, want_index=True)
    torch.cuda.synchronize()
    return d, base, unc


def check_against_base(d, base, unc, dim, what):
    """Corners, scores, count and agent are decode_nms_agents' bits; index and uncertainty name the anchor the box came from."""
    (bc, bs, bn, ba), (uc, us, un, uu, ua, ui) = base, unc
    k = int(bn.item())
    assert int(un.item()) == k and k > 0, (what, k, int(un.item()))
    assert torch.equal(uc[:k], bc[:k]) and torch.equal(us[:k], bs[:k]) and torch.equal(ua[:k], ba[:k]), what
    assert tuple(uu.shape[1:]) == (dim,)
    offs = np.cumsum([0] + [c["cls"].numel() for c in d])
    idx, agent, score, got = ui[:k].cpu().numpy(), ua[:k].cpu().numpy(), us[:k].cpu().numpy(), uu[:k].cpu().numpy()
    assert len(set(idx.tolist())) == k
    worst = 0.0
    for i in range(k):
        a_k = int(np.searchsorted(offs, idx[i], side="right") - 1)
        assert a_k == agent[i], (what, i)
        A, H, W = d[a_k]["cls"].shape[1:]
        local = int(idx[i] - offs[a_k])
        a, hw = local % A, local // A
        logit = float(d[a_k]["cls"][0, a].reshape(-1)[hw])
        worst = max(worst, abs(1.0 / (1.0 + np.exp(-logit)) - float(score[i])))
        want = d[a_k]["unc"][0].reshape(dim * A, H * W)[a * dim:(a + 1) * dim, hw].cpu().numpy()
        assert np.array_equal(got[i], want), (what, i, got[i], want)
    print(f"{what}: {k} boxes, score at the index within {worst:.3e}")
    assert worst <= 1e-6
    return k


# ---------------------------------------------------------------------------------------------------- the entry point
@pytest.mark.parametrize("dim", [2, 3, 7])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_bits_of_decode_nms_agents_plus_index_and_uncertainty(n, dim):
    cavs = scene(n, dim, 40 + n)
    d, base, unc = both(cavs)
    k = check_against_base(d, base, unc, dim, f"{n} cavs, dim {dim}")
    assert n == 1 or len(set(unc[4][:k].cpu().tolist())) > 1


def test_outputs_are_optional_and_sync_form():
    cavs = scene(2, 3, 7)
    d, base, unc = both(cavs)
    k = int(base[2].item())
    lists = [[c[key] for c in d] for key in ("cls", "reg", "dir", "anchors")]
    tfms = torch.stack([c["tfm"] for c in d])
    c3 = ops.decode_nms_agents_unc(*lists, [c["unc"] for c in d], tfms, *DEFAULTS, GT_RANGE)
    assert len(c3) == 3 and torch.equal(c3[0], base[0][:k]) and torch.equal(c3[1], base[1][:k]) and torch.equal(c3[2], unc[3][:k])
    c4 = ops.decode_nms_agents_unc(*lists, [c["unc"] for c in d], [c["tfm"].cpu().numpy() for c in d], *DEFAULTS, GT_RANGE,
                                   want_index=True)
    assert len(c4) == 4 and torch.equal(c4[3], unc[5][:k]) and torch.equal(c4[2], unc[3][:k])
    nodir = ops.decode_nms_agents_unc(lists[0], lists[1], None, lists[3], [c["unc"] for c in d], tfms, *DEFAULTS, GT_RANGE)
    want = ops.decode_nms_agents(lists[0], lists[1], None, lists[3], tfms, *DEFAULTS, GT_RANGE)
    assert torch.equal(nodir[0], want[0]) and torch.equal(nodir[1], want[1])
    quiet = [dict(c, cls=torch.full_like(c["cls"], -8.0)) for c in d]
    none = ops.decode_nms_agents_unc([c["cls"] for c in quiet], lists[1], lists[2], lists[3], [c["unc"] for c in d], tfms,
                                     *DEFAULTS, GT_RANGE, want_agent=True, want_index=True)
    assert none == (None, None, None, None, None)


def test_more_candidates_than_nms_top():
    cavs = scene(2, 3, 11, clusters=14)
    info = M.offenders(cavs, *DEFAULTS, GT_RANGE)[1]
    assert info["passing"] >= 100, info
    d, base, unc = both(cavs, top=64)
    assert base[0].shape[0] == 64 and unc[3].shape == (64, 3)
    check_against_base(d, base, unc, 3, f"nms_top 64 of {info['passing']}")


def test_more_than_4096_candidates_take_the_select_path():
    cavs = scene(1, 3, 13, sizes=[(48, 48)], clusters=0, mode="dense", lo=0.21, hi=0.99)
    info = M.offenders(cavs, *DEFAULTS, [-40.0, -40.0, -3.0, 40.0, 40.0, 1.0])[1]
    assert info["above_threshold"] == 48 * 48 * 2 and info["passing"] > 4096, info
    d, base, unc = both(cavs, gt_range=[-40.0, -40.0, -3.0, 40.0, 40.0, 1.0])
    check_against_base(d, base, unc, 3, f"{info['passing']} candidates")


# ---------------------------------------------------------------------------------------------------- the post-processor
@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "unc_post.npz"))


def post_for(g, cls=UncertaintyVoxelPostprocessor):
    p = configs.lidar_uncertainty([float(v) for v in g["sq_range"]])["postprocess"]
    p["gt_range"] = [float(v) for v in g["gt_range"]]
    return cls(p, train=False)


def dicts(g, tag, dev=DEV):
    n = int(g[f"{tag}_n"])
    data = {f"cav{k}": {"transformation_matrix": torch.from_numpy(g[f"{tag}{k}_tfm"]),
                        "anchor_box": torch.from_numpy(g[f"{tag}{k}_anchors"])} for k in range(n)}
    out = {f"cav{k}": {name: torch.from_numpy(g[f"{tag}{k}_{short}"]).to(dev) for name, short in
                       (("cls_preds", "cls"), ("reg_preds", "reg"), ("unc_preds", "unc"), ("dir_preds", "dir"))} for k in range(n)}
    return data, out


@pytest.mark.parametrize("tag", ["p", "s"])
def test_post_process_reproduces_the_reference_on_the_kernel(g, tag):
    post = post_for(g)
    data, out = dicts(g, tag)
    calls = {}
    ops.TIMING = calls
    try:
        pred, score, unc = post.post_process(data, out, return_uncertainty=True)
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert "decode_nms_agents_unc" in calls, calls
    pred, score, unc = pred.cpu().numpy(), score.cpu().numpy(), unc.cpu().numpy()
    assert pred.shape == g[f"{tag}_pred"].shape and score.shape == g[f"{tag}_score"].shape      # count (and, below, order)
    e_c, e_s = float(np.abs(pred - g[f"{tag}_pred"]).max()), float(np.abs(score - g[f"{tag}_score"]).max())
    print(f"{tag}: {pred.shape[0]} boxes, corners within {e_c:.3e}, scores within {e_s:.3e}")
    assert e_c <= 1e-3 and e_s <= 1e-6
    assert np.array_equal(unc, g[f"{tag}_unc"])
    # the tensor path on the device gives the same boxes
    f_pred, f_score, f_unc = post._post_process_unc_tensors(list(data.values()), list(out.values()))
    assert f_pred.shape[0] == pred.shape[0] and np.array_equal(f_unc.cpu().numpy(), unc)
    assert float(np.abs(f_pred.cpu().numpy() - pred).max()) <= 1e-3


def test_post_process_without_survivors_and_without_uncertainty(g):
    post = post_for(g)
    data, out = dicts(g, "s")
    two = post.post_process(data, out)
    parent = post_for(g, VoxelPostprocessor).post_process(data, {k: {n: t for n, t in v.items() if n != "unc_preds"}
                                                                 for k, v in out.items()})
    assert len(two) == 2 and torch.equal(two[0], parent[0]) and torch.equal(two[1], parent[1])
    for o in out.values():
        o["cls_preds"] = torch.full_like(o["cls_preds"], -8.0)
    assert post.post_process(data, out, return_uncertainty=True) == (None, None, None)
    assert post.post_process(data, out) == (None, None)


# ---------------------------------------------------------------------------------------------------- the model
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]


def test_model_forward_heads():
    hypes = configs.lidar_uncertainty(M_RANGE)
    model = fill_module(train_utils.create_model(hypes)).to(DEV).eval()
    parts = []
    for b, seed in enumerate((191, 192)):
        pts = synth.lidar_frame(seed)
        near = (np.abs(pts[:, 0]) < M_RANGE[3] + 2) & (np.abs(pts[:, 1]) < M_RANGE[4] + 2)
        parts.append(cref.voxelize(pts[near][:1000], M_RANGE, (0.4, 0.4, 4), 32, 70000, batch_idx=b))
    data = {"processed_lidar": {
        "voxel_features": torch.from_numpy(np.concatenate([p[0] for p in parts])).to(DEV),
        "voxel_coords": torch.from_numpy(np.concatenate([p[1] for p in parts])).to(torch.int32).to(DEV),
        "voxel_num_points": torch.from_numpy(np.concatenate([p[2] for p in parts])).to(torch.int32).to(DEV)}}
    with torch.no_grad():
        out = model(data)
        feat = model.bev_features(data)[1]
    assert sorted(out) == ["cls_preds", "dir_preds", "reg_preds", "unc_preds"]
    assert [tuple(out[k].shape) for k in sorted(out)] == [(2, 2, 32, 32), (2, 4, 32, 32), (2, 14, 32, 32), (2, 6, 32, 32)]
    assert tuple(feat.shape) == (2, 384, 32, 32)
    # the PointPillar detector holding the same weights: where the structure coincides, the same bits
    args = {k: v for k, v in hypes["model"]["args"].items() if k not in ("anchor_num", "uncertainty_dim")}
    plain = PointPillar({**args, "anchor_number": 2}).to(DEV).eval()
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("unc_head")}, strict=True)
    with torch.no_grad():
        want = plain(data)
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        assert torch.equal(out[k], want[k]), k
    ref = F.conv2d(feat, model.unc_head.weight, model.unc_head.bias)
    err = float((out["unc_preds"] - ref).abs().max()) / float(ref.abs().max())
    print(f"unc_preds against F.conv2d: relative error {err:.3e}")
    assert err <= 1e-5 and float(ref.abs().max()) > 0
