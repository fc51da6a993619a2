"""The configurations and seeded inputs of the uncertainty criterion's tests, shared by the generator
(tests/golden/gen_unc_golden.py), tests/test_unc_cpu.py and tests/test_gpu_unc_loss.py."""
import copy

import torch

from heal_amd import configs

# tag -> (dim, xy_loss_type, angle_loss_type, limit_period, with_dir): dim 3 with l2 + von Mises, limit_period on and off; dim 3
# with l1 + l2; dim 7; dim 2 -- with and without the direction term
CONFIGS = {
    "d3_vm_lp": (3, "l2", "von-mise", True, True),
    "d3_vm": (3, "l2", "von-mise", False, True),
    "d3_l1_l2": (3, "l1", "l2", False, False),
    "d7": (7, "l2", "l2", False, True),
    "d2": (2, "l2", "l2", False, False),
}
S_RANGE = 4.0            # s ~ U(-4, 4): kappa = exp(-s) <= 54.6, the reference's own exp(kappa) stays finite in float32
GOLDEN_SHAPE = (2, 9, 15)


def loss_args(tag, weight=None):
    """The `loss.args` block of configs.lidar_uncertainty for configuration `tag`."""
    dim, xy, angle, limit, with_dir = CONFIGS[tag]
    args = copy.deepcopy(configs.lidar_uncertainty(dim=dim, dir_head=with_dir)["loss"]["args"])
    args["uncertainty"].update({"xy_loss_type": xy, "angle_loss_type": angle, "limit_period": limit})
    if weight is not None:
        args["uncertainty"]["weight"] = weight
    return args


def loss_inputs(seed, n, H, W, dim, A=2, positives=0.08):
    """Seeded head maps and labels: (out, tgt) of CPU float32 tensors, `positives` of the anchors positive."""
    g = torch.Generator().manual_seed(seed)
    out = {"cls_preds": torch.randn((n, A, H, W), generator=g), "reg_preds": torch.randn((n, 7 * A, H, W), generator=g) * 0.3,
           "dir_preds": torch.randn((n, 2 * A, H, W), generator=g),
           "unc_preds": (torch.rand((n, dim * A, H, W), generator=g) * 2 - 1) * S_RANGE}
    pos = (torch.rand((n, H, W, A), generator=g) > 1 - positives).float()
    neg = ((torch.rand((n, H, W, A), generator=g) > 0.2).float()) * (1 - pos)
    tgt = torch.randn((n, H, W, 7 * A), generator=g) * 0.4
    return out, {"pos_equal_one": pos, "neg_equal_one": neg, "targets": tgt}


def golden_inputs(tag):
    dim = CONFIGS[tag][0]
    return loss_inputs(4100 + dim, *GOLDEN_SHAPE, dim)
