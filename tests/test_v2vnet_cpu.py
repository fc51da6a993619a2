"""V2VNet fusion (fusion_method: v2vnet) on the CPU: the mirror's torch arithmetic against the reference's outputs
(tests/golden/v2vnet_small.npz) and its parameter layout against the reference's (tests/golden/v2vnet_state_dict_keys.json, one
entry per reference YAML that selects v2vnet; also against the live reference where its tree is present).  No GPU."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from heal_amd import configs
from tests.golden.detfill import fill_module

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E2E_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]        # the end-to-end case of v2vnet_small.npz (a 16 x 16 fusion map)
C_SMALL = 128
# prefix -> (overrides of lidar_v2vnet.yaml's v2vnet block, (H, W)); as tests/golden/gen_golden_v2vnet.py:CASES
CASES = {"n5_": ({}, (8, 8)), "n3_": ({}, (8, 8)), "n1_": ({}, (8, 8)), "b2_": ({}, (8, 8)),
         "max_": ({"agg_operator": "max"}, (8, 8)), "nogru_": ({"gru_flag": False}, (8, 8)), "it1_": ({"num_iteration": 1}, (8, 8)),
         "it3_": ({"num_iteration": 3}, (8, 8)), "l2_": ({"layers": 2}, (8, 8)), "odd_": ({}, (13, 11))}


def rel_err(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def v2vnet_args(overrides, hw, channels=C_SMALL):
    args = {"num_iteration": 2, "in_channels": channels, "gru_flag": True, "agg_operator": "avg",
            "conv_gru": {"H": hw[0], "W": hw[1], "num_layers": 1, "kernel_size": [[3, 3]]}}
    for k, v in overrides.items():
        if k == "layers":
            args["conv_gru"]["num_layers"] = v
            args["conv_gru"]["kernel_size"] = [[3, 3]] * v
        else:
            args[k] = v
    return args


def make_v2vnet(prefix, channels=C_SMALL):
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import V2VNetFusion
    over, hw = CASES[prefix]
    return fill_module(V2VNetFusion(v2vnet_args(over, hw, channels))).eval()


def case_inputs(g, prefix):
    """(x, record_len, affine) of a module case: int8-coded maps, the affines normalised as HeterModelBaseline does."""
    from oracle import oracle_np as O
    x = torch.from_numpy(g[f"{prefix}x_code"].astype(np.float32) / np.float32(g["x_scale"]))
    return x, torch.from_numpy(g[f"{prefix}record_len"]), O.normalize_pairwise_tfm(g[f"{prefix}pairwise"], *g["HW_m"], 1)


def e2e_data(g):
    return {"inputs_m1": {"voxel_features": torch.from_numpy(g["e2e_voxel_features"]),
                          "voxel_coords": torch.from_numpy(g["e2e_voxel_coords"]).to(torch.int32),
                          "voxel_num_points": torch.from_numpy(g["e2e_voxel_num_points"]).to(torch.int32)},
            "agent_modality_list": ["m1"] * 3, "record_len": torch.tensor([3]),
            "pairwise_t_matrix": torch.from_numpy(g["e2e_pairwise"])}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "v2vnet_small.npz"))


@pytest.mark.parametrize("prefix", sorted(CASES))
def test_v2vnet_module_matches_reference(g, prefix):
    model = make_v2vnet(prefix)
    with torch.no_grad():
        got = model(*case_inputs(g, prefix)).numpy()
    want = g[f"{prefix}out"]
    assert got.shape == want.shape
    assert rel_err(got, want) <= 1e-4, rel_err(got, want)


@pytest.mark.grad
def test_heter_model_baseline_v2vnet_matches_reference(g):
    from heal_amd.opencood.tools.train_utils import create_model
    model = fill_module(create_model(configs.lidar_baseline("v2vnet", E2E_RANGE))).eval()
    out = model(e2e_data(g))      # autograd records: the encoders run their (CPU) gradient path
    for key, name in (("cls_preds", "cls"), ("reg_preds", "reg"), ("dir_preds", "dir")):
        e = rel_err(out[key].detach().numpy(), g[f"e2e_{name}"])
        assert e <= 1e-4, (key, e)


def test_lidar_baseline_v2vnet_config_builds():
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import V2VNetFusion
    from heal_amd.opencood.tools.train_utils import create_model
    hy = configs.lidar_baseline("v2vnet")
    a = hy["model"]["args"]["v2vnet"]
    assert a == {"num_iteration": 2, "in_channels": 256, "gru_flag": True, "agg_operator": "avg",
                 "conv_gru": {"H": 128, "W": 128, "num_layers": 1, "kernel_size": [[3, 3]]}}
    model = create_model(hy)
    assert isinstance(model.fusion_net, V2VNetFusion)
    assert configs.lidar_baseline("v2vnet", E2E_RANGE)["model"]["args"]["v2vnet"]["conv_gru"]["H"] == 16


def test_v2vnet_conv_gru_size_mismatch_raises(g):
    model = make_v2vnet("n3_")                     # conv_gru built for 8 x 8
    x, rl, aff = case_inputs(g, "n3_")
    with pytest.raises(ValueError, match="conv_gru"):
        with torch.no_grad():
            model(torch.nn.functional.pad(x, (0, 8, 0, 8)), rl, aff)
    model.gru_flag = False                         # without the GRU the reference never reads conv_gru's size
    with torch.no_grad():
        model(torch.nn.functional.pad(x, (0, 8, 0, 8)), rl, aff)


def test_v2vnet_bad_agg_operator_raises(g):
    model = make_v2vnet("n1_")
    model.agg_operator = "sum"
    with pytest.raises(ValueError, match="agg_operator"):
        with torch.no_grad():
            model(*case_inputs(g, "n1_"))


def test_v2vnet_sharded_split_is_refused():
    from heal_amd import dist
    from heal_amd.opencood.tools.train_utils import create_model
    model = create_model(configs.lidar_baseline("v2vnet", E2E_RANGE))
    with pytest.raises(NotImplementedError, match="V2VNet"):
        dist.make_sharded(model, 0, 2)


def _yaml_table():
    with open(os.path.join(GOLD, "v2vnet_state_dict_keys.json")) as fh:
        return json.load(fh)


def test_v2vnet_state_dict_table_covers_the_three_yamls():
    t = _yaml_table()
    assert sorted(t) == ["opv2v/CameraOnly/camera_v2vnet.yaml", "opv2v/LiDAROnly/lidar_v2vnet.yaml",
                         "opv2v/MoreModality/2_modality_end2end_training/lidar_camera_v2vnet.yaml"]
    assert all(v["model"]["args"]["fusion_method"] == "v2vnet" for v in t.values())


@pytest.mark.parametrize("rel", sorted(_yaml_table()))
def test_v2vnet_state_dict_matches_reference_yaml(rel):
    """The YAML's model constructs through create_model; its keys and shapes equal the reference's (the committed table, and the
    reference itself where its tree is present); a dict keyed like the reference's loads strictly."""
    from heal_amd.opencood.tools.train_utils import create_model
    entry = _yaml_table()[rel]
    model = create_model({"model": copy.deepcopy(entry["model"])})
    mine = {k: list(v.shape) for k, v in model.state_dict().items()}
    if entry["scope"] == "fusion_net":
        mine = {k: v for k, v in mine.items() if k.startswith("fusion_net.")}
    assert mine == entry["keys"], rel
    a = entry["model"]["args"]["v2vnet"]
    C = a["in_channels"]
    assert entry["keys"]["fusion_net.conv_gru.cell_list.0.conv_gates.weight"] == [2 * C, 3 * C, 3, 3]
    assert entry["keys"]["fusion_net.conv_gru.cell_list.0.conv_can.weight"] == [C, 3 * C, 3, 3]
    if os.path.isdir("/root/reference/opencood"):      # the live reference, where it is present
        from tests.golden import ref_import as R
        fio = R.ref("opencood.models.fuse_modules.fusion_in_one")
        live = {f"fusion_net.{k}": list(v.shape) for k, v in fio.V2VNetFusion(copy.deepcopy(a)).state_dict().items()}
        assert {k: v for k, v in mine.items() if k.startswith("fusion_net.")} == live
    sd = model.state_dict()
    ref_keyed = {k: (sd[k].clone() if not sd[k].dtype.is_floating_point else torch.randn(shape))
                 for k, shape in entry["keys"].items()}
    if entry["scope"] == "fusion_net":
        model.fusion_net.load_state_dict({k[len("fusion_net."):]: v for k, v in ref_keyed.items()}, strict=True)
    else:
        model.load_state_dict(ref_keyed, strict=True)


@pytest.mark.grad
@pytest.mark.parametrize("prefix", ["n3_", "max_", "nogru_"])
def test_v2vnet_gradient_path_reaches_every_parameter(g, prefix):
    model = make_v2vnet(prefix)
    x, rl, aff = case_inputs(g, prefix)
    x = x.clone().requires_grad_(True)
    out = model(x, rl, aff)
    assert rel_err(out.detach().numpy(), g[f"{prefix}out"]) <= 1e-4
    out.square().mean().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    for name, p in model.named_parameters():
        if not model.gru_flag and name.startswith("conv_gru."):
            continue                               # gru_flag false: the reference never calls conv_gru
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
