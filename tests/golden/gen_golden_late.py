"""Generate tests/golden/late_decode.npz by running the REFERENCE's VoxelPostprocessor.post_process (build container only) on
late-fusion scenes: several cavs in output_dict, each with its own pose and anchor table
(opencood/data_utils/post_processor/voxel_postprocessor.py:277-405).

    python -m tests.golden.gen_golden_late

Case "a": 5 cavs with distinct non-trivial poses -- three on a 32 x 32 grid, one on a 24 x 40 grid with its own anchor table
(the reference's generate_anchor_box on a matching range), one with NO score above the threshold, one whose candidates ALL
fail the size / z filters.  Case "b": 3 cavs pooling more than 1000 filter-passing candidates (the top-1000 cut).

The above-threshold logits come from a ladder of distinct scores, and candidates that would put a decision on an edge are
demoted to background until every margin of tests/golden/late_margins.py holds; the margins are asserted on what is written.
The fixture stores inputs and the reference's outputs only."""
import copy
import os

import numpy as np
import torch

from heal_amd import configs, synth
from tests.golden import late_margins as M
from tests.golden import ref_import as R

OUT = os.path.dirname(os.path.abspath(__file__))
GT_RANGE = [-16.0, -16.0, -3.0, 16.0, 16.0, 1.0]


def _post(lidar_range, W, H):
    """The reference's VoxelPostprocessor on `lidar_range` (anchor grid W x H cells of 0.4 m, feature stride 2)."""
    vp = R.ref("opencood.data_utils.post_processor.voxel_postprocessor")
    p = copy.deepcopy(configs.m1_late(lidar_range)["postprocess"])
    p["anchor_args"].update({"W": W, "H": H, "cav_lidar_range": list(lidar_range)})
    p["gt_range"] = list(GT_RANGE)
    return vp.VoxelPostprocessor(p, train=False)


def _reference(cavs, post):
    data = {f"cav{k}": {"transformation_matrix": torch.from_numpy(c["tfm"]), "anchor_box": torch.from_numpy(c["anchors"])}
            for k, c in enumerate(cavs)}
    out = {f"cav{k}": {"cls_preds": torch.from_numpy(c["cls"]), "reg_preds": torch.from_numpy(c["reg"]),
                       "dir_preds": torch.from_numpy(c["dir"])} for k, c in enumerate(cavs)}
    with torch.no_grad():
        pred, score = post.post_process(data, out)
    return pred.numpy(), score.numpy()


def main():
    rng = np.random.default_rng(2024)
    sq = [-12.8, -12.8, -3, 12.8, 12.8, 1]
    rect = [-16.0, -9.6, -3, 16.0, 9.6, 1]
    post = _post(sq, 64, 64)
    anchors_sq = post.generate_anchor_box()                            # [32,32,2,7] f64
    anchors_rect = _post(rect, 80, 48).generate_anchor_box()           # [24,40,2,7] f64
    assert anchors_sq.shape == (32, 32, 2, 7) and anchors_rect.shape == (24, 40, 2, 7)
    poses = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [3.0, -2.0, 0.1, 0.0, 25.0, 0.0], [-4.0, 5.0, -0.2, 0.3, -70.0, 0.2],
             [6.0, 6.0, 0.05, -0.4, 140.0, 0.3], [-7.0, -3.0, 0.15, 0.2, 200.0, -0.3]]
    tf = lambda k: synth.x_to_world(poses[k])
    case_a = [M.make_cav(rng, anchors_sq, tf(0), 22), M.make_cav(rng, anchors_sq, tf(1), 22),
              M.make_cav(rng, anchors_sq, tf(2), 0, "empty"), M.make_cav(rng, anchors_rect, tf(3), 18),
              M.make_cav(rng, anchors_sq, tf(4), 10, "filtered")]
    M.deal_ladder(rng, case_a)
    case_b = [M.make_cav(rng, anchors_sq, tf(k), 75) for k in (0, 1, 3)]
    M.deal_ladder(rng, case_b)
    out = {"gt_range": np.array(GT_RANGE), "score_thr": np.array(post.params["target_args"]["score_threshold"]),
           "nms_thr": np.array(post.params["nms_thresh"]), "dir_offset": np.array(post.params["dir_args"]["dir_offset"]),
           "num_bins": np.array(post.params["dir_args"]["num_bins"])}
    params = (post.params["target_args"]["score_threshold"], post.params["dir_args"]["dir_offset"],
              post.params["dir_args"]["num_bins"], post.params["nms_thresh"], GT_RANGE)
    for tag, cavs in (("a", case_a), ("b", case_b)):
        info = M.settle(cavs, *params)
        pred, score = _reference(cavs, post)
        print(tag, info, "kept", pred.shape[0])
        out[f"{tag}_n"] = np.array(len(cavs))
        for k, c in enumerate(cavs):
            for name in ("cls", "reg", "dir", "anchors", "tfm"):
                out[f"{tag}{k}_{name}"] = c[name]
        out[f"{tag}_pred"], out[f"{tag}_score"] = pred, score
    assert M.offenders(case_a, *params)[1]["per_agent_above"][2] == 0
    path = os.path.join(OUT, "late_decode.npz")
    np.savez_compressed(path, **out)
    print(f"late_decode: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
