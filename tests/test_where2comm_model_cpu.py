"""The Where2comm model without a GPU: Communication's torch composition, Where2comm and CenterPointWhere2comm against the reference's
recordings (tests/golden/w2c_comm_small.npz), the parameter layout (w2c_comm_state_dict_keys.json), the refusals, the config /
factory wiring and the C header (include/heal_amd_comm.h)."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from heal_amd import _capi, configs
from heal_amd.opencood.tools import train_utils
from tests.golden import w2c_comm_margins as WM
from tests.golden.detfill import fill_module

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M_RANGE = [-12.8, -12.8, -3, 12.8, 12.8, 1]
TOL = 1e-3            # tests/test_where2comm_cpu.py's bar for fused feature maps
TOL_HEADS = 1e-5      # tests/test_center_point_cpu.py's bar
OUT_STRIDE = {"ss": 8, "ms": 48}              # the channels the fixture keeps (tests/golden/gen_golden_w2c_comm.py)
BACKBONE = {"layer_nums": [1, 1, 1], "layer_strides": [1, 2, 2], "num_filters": [64, 128, 256], "upsample_strides": [1, 2, 4],
            "num_upsample_filter": [128, 128, 128]}
SYMBOLS = ("heal_comm_fused_enabled", "heal_comm_mask_supported", "heal_comm_mask_workspace", "heal_comm_mask", "heal_warp_att_fuse_levels_masked")


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-12))


def module_input(n, C, H, W):
    """The module cases' feature maps: the closed form of tests/golden/gen_golden_w2c_comm.py (integer codes over 8)."""
    idx = np.arange(n * C * H * W, dtype=np.float64)
    code = np.round(12.0 * np.sin(idx * 0.6180339887 + 0.37) * np.cos(idx * 0.0137))
    return (code / 8.0).astype(np.float32).reshape(n, C, H, W)


def module_args(mode, multi_scale, thre):
    return {"voxel_size": [WM.MODULE_VOXEL, WM.MODULE_VOXEL, 4], "downsample_rate": 1, "multi_scale": multi_scale,
            "layer_nums": BACKBONE["layer_nums"], "num_filters": BACKBONE["num_filters"],
            "agg_operator": {"mode": mode, "feature_dim": 64},
            "communication": {"thre": thre, "gaussian_smooth": {"k_size": 5, "c_sigma": 1.0}}}


def make_module(g, prefix, device="cpu"):
    """(Where2comm, backbone | None, inputs) of a module case."""
    from heal_amd.opencood.models.fuse_modules.where2comm_attn import Where2comm
    from heal_amd.opencood.models.sub_modules.base_bev_backbone import BaseBEVBackbone
    from heal_amd.opencood.models.sub_modules.base_bev_backbone_resnet import ResNetBEVBackbone
    mode, multi_scale, form = WM.MODULE_CASES[prefix]
    module = Where2comm(module_args(mode, multi_scale, float(g["mod_thre"]))).to(device).eval()
    backbone = None
    if form is not None:
        cls = ResNetBEVBackbone if form == "resnet" else BaseBEVBackbone
        backbone = fill_module(cls(copy.deepcopy(BACKBONE), 64)).to(device).eval()
    n = sum(WM.RECORD_LEN)
    inputs = (torch.from_numpy(module_input(n, 64, WM.MODULE_HW, WM.MODULE_HW)).to(device), torch.from_numpy(g["mod_rm"]).to(device),
              torch.tensor(WM.RECORD_LEN), torch.from_numpy(g["mod_pairwise"].copy()).to(device))
    return module, backbone, inputs


def kept(y, prefix):
    return y[:, ::OUT_STRIDE["ms" if WM.MODULE_CASES[prefix][1] else "ss"]]


def model_hypes(g, **kw):
    return configs.lidar_centerpoint_where2comm("ATTEN", True, "resnet", True, M_RANGE, thre=float(g["m_thre"]), **kw)


def model_data(center, device="cpu"):
    return {"processed_lidar": {k: torch.from_numpy(center["m3_" + k]).to(device)
                                for k in ("voxel_features", "voxel_coords", "voxel_num_points")},
            "record_len": torch.tensor([3]), "pairwise_t_matrix": torch.from_numpy(center["m3_pairwise"].copy()).to(device)}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "w2c_comm_small.npz"))


@pytest.fixture(scope="module")
def center():
    return np.load(os.path.join(GOLD, "center_small.npz"))


# ---- Communication -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", sorted(WM.MASK_CASES))
def test_communication_composition_matches_reference(g, prefix):
    """The CPU composition: masks of every level and the rate exact."""
    from heal_amd.opencood.models.comm_modules.where2comm import Communication
    c = WM.mask_case(g, prefix)
    args = {"thre": c["thre"]}
    if c["k"]:
        args["gaussian_smooth"] = {"k_size": c["k"], "c_sigma": 1.0}
    module = Communication(args).eval()
    if c["k"]:
        if prefix != "par_":                                                  # the constructor's own values are the reference's
            assert np.array_equal(module.gaussian_filter.weight.detach().numpy().reshape(c["k"], c["k"]), c["weight"])
            assert float(module.gaussian_filter.bias) == 0
        module.load_state_dict({"gaussian_filter.weight": torch.from_numpy(c["weight"]).view(1, 1, c["k"], c["k"]),
                                "gaussian_filter.bias": torch.from_numpy(c["bias"])}, strict=True)
    else:
        assert not module.state_dict()
    psm = torch.from_numpy(c["psm"])
    maps, mask, rate = module(torch.split(psm, c["record_len"]), torch.tensor(c["record_len"]), None)
    assert np.array_equal(mask.numpy(), g[prefix + "mask0"].astype(np.float32))
    assert np.float32(rate) == g[prefix + "rate"]
    assert len(maps) == 2 and tuple(maps[0].shape) == (3, 1) + psm.shape[2:]
    masks, rate2 = module.level_masks(psm, c["record_len"], c["n_levels"])
    assert np.float32(rate2) == g[prefix + "rate"]
    for l, m in enumerate(masks):
        assert np.array_equal(m.numpy(), g[f"{prefix}mask{l}"].astype(np.float32)), (prefix, l)


# ---- Where2comm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.grad
@pytest.mark.parametrize("prefix", sorted(WM.MODULE_CASES))
def test_where2comm_module_matches_reference(g, prefix):
    module, backbone, inputs = make_module(g, prefix)
    y, rate, extra = module(*inputs, backbone)          # autograd records: the backbones run their (CPU) gradient path
    assert extra == {} and np.float32(rate) == g["mod_rate"]
    want = g[prefix + "out"]
    got = kept(y.detach().numpy(), prefix)
    assert got.shape == want.shape
    e = rel_err(got, want)
    print(prefix, e)
    assert e <= TOL


def test_where2comm_module_fixture_has_a_footprint_off_the_map(g):
    from heal_amd.opencood.models.fuse_modules.fusion_in_one import _warp_affine_simple
    from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm
    HW = WM.MODULE_HW
    aff = normalize_pairwise_tfm(torch.from_numpy(g["mod_pairwise"].copy()), HW, HW, WM.MODULE_VOXEL, 1)
    cover = _warp_affine_simple(torch.ones((3, 1, HW, HW)), aff[0, 0, :3].float(), (HW, HW))
    share = float((cover[1] == 0).float().mean())
    assert 0.1 < share < 0.9, share


@pytest.mark.grad
def test_where2comm_without_communication_has_a_zero_rate_and_no_parameters(g):
    from heal_amd.opencood.models.fuse_modules.where2comm_attn import Where2comm
    args = module_args("MAX", False, 0.0)
    del args["communication"]
    module = Where2comm(args).eval()
    assert not module.state_dict() and not module.communication
    _, _, inputs = make_module(g, "max_ss_")
    y, rate, extra = module(*inputs)
    assert rate.dtype == torch.int64 and int(rate) == 0 and rate.device == inputs[0].device and extra == {}
    assert rel_err(kept(y.numpy(), "max_ss_"), g["max_ss_out"]) > 1e-2        # the mask matters


def test_where2comm_refuses_transformer_and_more_than_eight_agents(g):
    from heal_amd.opencood.models.fuse_modules.where2comm_attn import Where2comm
    args = module_args("Transformer", False, 0.1)
    args["agg_operator"].update({"n_head": 8, "with_spe": True, "with_scm": True})
    with pytest.raises(NotImplementedError, match="cannot run in the reference") as e:
        Where2comm(args)
    assert "ATTEN and MAX" in str(e.value) and "fuse_network" in str(e.value)
    with pytest.raises(NotImplementedError, match="ATTEN and MAX"):
        Where2comm(module_args("MEAN", False, 0.1))
    module = Where2comm(module_args("MAX", False, 0.1)).eval()
    n = 9
    pw = np.tile(np.eye(4), (1, n, n, 1, 1))
    with pytest.raises(ValueError, match="9 agents"):
        module(torch.zeros((n, 64, 8, 8)), torch.zeros((n, 1, 8, 8)), torch.tensor([n]), torch.from_numpy(pw))


# ---- CenterPointWhere2comm -------------------------------------------------------------------------------------------------------------
@pytest.mark.grad
def test_center_point_where2comm_matches_reference(g, center):
    model = WM.model_fill(train_utils.create_model(model_hypes(g))).eval()
    out = model(model_data(center))
    assert sorted(out) == sorted(WM.MODEL_KEYS)
    assert np.float32(out["comm_rate"]) == g["m_comm_rate"]
    for key in WM.MODEL_KEYS[:-1]:
        want = g["m_" + key]
        got = out[key].detach().numpy()
        assert got.shape == want.shape, key
        e = rel_err(got, want)
        print(key, e)
        assert e <= (TOL_HEADS if "single" in key else TOL), (key, e)


def test_state_dict_names_and_shapes_match_the_reference():
    want = json.load(open(os.path.join(GOLD, "w2c_comm_state_dict_keys.json")))
    built = {"ms_resnet": configs.lidar_centerpoint_where2comm("ATTEN", True, "resnet"),
             "ms_plain": configs.lidar_centerpoint_where2comm("MAX", True, "plain"),
             "ss": configs.lidar_centerpoint_where2comm("ATTEN", False, "resnet"),
             "no_comm": configs.lidar_centerpoint_where2comm("MAX", False, "plain", communication=False)}
    assert sorted(built) == sorted(want)
    for name, hypes in built.items():
        model = train_utils.create_model(hypes)
        got = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert got == want[name], (name, sorted(set(got) ^ set(want[name])))
        model.load_state_dict({k: torch.zeros(shape) for k, shape in want[name].items()}, strict=True)
    pre = "fusion_net.naive_communication.gaussian_filter."
    assert want["ms_resnet"][pre + "weight"] == [1, 1, 5, 5] and want["ms_resnet"][pre + "bias"] == [1]
    assert sorted(k for k in want["ms_resnet"] if k.startswith("fusion_net.")) == [pre + "bias", pre + "weight"]
    assert not [k for k in want["no_comm"] if k.startswith("fusion_net.")]
    assert any(k.startswith("backbone.resnet.") for k in want["ss"]) and any(k.startswith("backbone.blocks.") for k in want["ms_plain"])


def test_gaussian_filter_initial_values():
    """1 / (2 pi sigma) exp(-(x^2 + y^2) / (2 sigma^2)): sigma, not sigma squared, in the prefactor (where2comm.py:28)."""
    from heal_amd.opencood.models.comm_modules.where2comm import Communication
    m = Communication({"thre": 0.01, "gaussian_smooth": {"k_size": 5, "c_sigma": 2.0}})
    w = m.gaussian_filter.weight.detach().numpy().reshape(5, 5)
    assert abs(w[2, 2] - 1 / (4 * np.pi)) < 1e-7 and abs(w[2, 3] - np.exp(-1 / 8) / (4 * np.pi)) < 1e-7
    assert np.array_equal(w, WM.gaussian_weight(5, 2.0)) and float(m.gaussian_filter.bias) == 0
    assert m.gaussian_filter.padding == (2, 2) and m.smooth and not Communication({"thre": 0.5}).smooth


def test_backbone_fix_freezes_all_but_the_fusion_net(g):
    hypes = model_hypes(g)
    hypes["model"]["args"]["backbone_fix"] = True
    model = train_utils.create_model(hypes)
    free = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    assert free == ["fusion_net.naive_communication.gaussian_filter.bias", "fusion_net.naive_communication.gaussian_filter.weight"]
    assert abs(float(model.cls_head.bias[0]) + np.log(99.0)) < 1e-6 and float(model.reg_head.weight.std()) < 2e-3     # init_weight


def test_factory_configs_and_yaml_round_trip(tmp_path):
    from heal_amd.opencood.hypes_yaml import yaml_utils
    for agg, ms, bb, comm in (("ATTEN", True, "resnet", True), ("MAX", True, "plain", True), ("MAX", False, "plain", False)):
        hy = configs.lidar_centerpoint_where2comm(agg, ms, bb, comm, M_RANGE)
        assert hy["model"]["core_method"] == "center_point_where2comm" and hy["loss"]["core_method"] == "center_point_loss"
        fa = hy["model"]["args"]["fusion_args"]
        assert fa["agg_operator"]["mode"] == agg and fa["multi_scale"] is ms and ("communication" in fa) is comm
        assert fa["downsample_rate"] == (1 if ms else 2) and ("resnet" in hy["model"]["args"]["base_bev_backbone"]) is (bb == "resnet")
        model = train_utils.create_model(hy)
        assert type(model).__name__ == "CenterPointWhere2comm" and type(model.fusion_net).__name__ == "Where2comm"
        p = tmp_path / f"{agg}_{ms}_{bb}.yaml"
        configs.dump_yaml(hy, str(p))
        back = yaml_utils.load_yaml(str(p))
        assert back["model"]["args"]["fusion_args"] == fa and back["model"]["core_method"] == "center_point_where2comm"
        assert type(train_utils.create_model(back)).__name__ == "CenterPointWhere2comm"
    with pytest.raises(ValueError, match="backbone"):
        configs.lidar_centerpoint_where2comm(backbone="resnext")


def test_sharded_split_is_refused(g):
    from heal_amd import dist
    model = train_utils.create_model(model_hypes(g))
    with pytest.raises(NotImplementedError, match="CenterPointWhere2comm") as e:
        dist.make_sharded(model, 0, 2)
    assert "unwarped" in str(e.value).lower()


# ---- header, bindings, switch ----------------------------------------------------------------------------------------------------------
def test_header_parses_and_the_library_exports_every_symbol():
    sig = _capi.signatures_comm()
    assert sorted(sig) == sorted(SYMBOLS)
    I, P, F, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
    assert sig["heal_comm_mask_supported"] == (I, [I] * 7) and sig["heal_comm_fused_enabled"] == (I, [])
    assert sig["heal_comm_mask_workspace"] == (Z, [I, I, I])
    assert sig["heal_comm_mask"] == (I, [P, I, I, I, I, P, I, P, P, I, F, I, P, P, P, P, Z, P])
    assert sig["heal_warp_att_fuse_levels_masked"] == (I, [I, P, P, I, P, P, P, P, P, P, I, I, P, P])
    unmasked = _capi.signatures()["heal_warp_att_fuse_levels"]
    assert sig["heal_warp_att_fuse_levels_masked"][1] == unmasked[1][:2] + [P] + unmasked[1][2:]     # one more host array
    assert not set(sig) & set(_capi.signatures())                    # outside the versioned table, whose size and version stay
    assert len(_capi.signatures(False)) == 126 and _capi.abi_version_of_header() == 13
    assert _capi.header_define("HEAL_COMM_MAX_K", _capi.HEADER_COMM) == 9
    from heal_amd import build
    assert _capi.HEADER_COMM in build._deps()
    build.build()
    lib = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libheal_amd.so does not export {name}"
        assert getattr(lib, name).argtypes == sig[name][1]
    header = open(_capi.HEADER_COMM).read()
    for cite in ("comm_modules/where2comm.py:34-78", "where2comm_attn.py:264-275", ":69-71"):
        assert cite in header, cite


def test_supported_and_workspace_are_host_arithmetic():
    q = lambda *a: _capi.query("heal_comm_mask_supported", *a)        # noqa: E731
    assert q(5, 2, 2, 13, 11, 5, 3) == 1 and q(5, 2, 1, 1, 1, 1, 1) == 1 and q(5, 2, 2, 13, 11, 9, 4) == 1
    assert q(5, 2, 2, 13, 11, 4, 3) == 0 and q(5, 2, 2, 13, 11, 11, 3) == 0 and q(5, 2, 2, 13, 11, 0, 3) == 0      # even, too large, 0
    assert q(5, 2, 2, 13, 11, 5, 0) == 0 and q(5, 2, 2, 13, 11, 5, 5) == 0                                          # levels
    assert q(1, 2, 2, 13, 11, 5, 3) == 0 and q(5, 0, 2, 13, 11, 5, 3) == 0 and q(5, 2, 0, 13, 11, 5, 3) == 0
    assert q(5, 2, 2, 0, 11, 5, 3) == 0 and q(513, 2, 2, 13, 11, 5, 3) == 0 and q(5, 2, 1, 65536, 32768, 5, 3) == 0
    ws = lambda *a: _capi.query("heal_comm_mask_workspace", *a)       # noqa: E731
    assert ws(2, 13, 11) == 256 and ws(2, 45, 38) == 256 and ws(40, 65, 33) == 1024 and ws(0, 13, 11) == 0


def test_ops_refuse_cpu_tensors(g):
    from heal_amd import ops
    c = WM.mask_case(g, "odd_")
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.comm_mask(torch.from_numpy(c["psm"]), c["record_len"], None, None, c["thre"], 3)
    z = torch.zeros((2, 4, 8, 8))
    with pytest.raises(_capi.HealAmdError, match="CUDA/HIP"):
        ops.warp_att_fuse_levels([z], np.zeros((2, 2, 3)), masks=[torch.zeros((2, 1, 8, 8))])


def test_switch_is_declared_and_read_by_the_library(monkeypatch):
    """HEAL_COMM_FUSED is one of the library's own variables (heal_comm_fused_enabled reads it when called)."""
    from heal_amd import ops, switches
    assert switches.SWITCHES["HEAL_COMM_FUSED"].where == "library"
    assert "`HEAL_COMM_FUSED=0`" in open(os.path.join(os.path.dirname(GOLD), "..", "README.md")).read()
    monkeypatch.delenv("HEAL_COMM_FUSED", raising=False)
    assert ops.comm_fused_enabled() is True
    for text, want in (("0", False), ("1", True), ("", True)):
        monkeypatch.setenv("HEAL_COMM_FUSED", text)
        assert ops.comm_fused_enabled() is want
    monkeypatch.setenv("HEAL_COMM_FUSED", "yes")
    with pytest.raises(_capi.HealAmdError, match="HEAL_COMM_FUSED"):
        ops.comm_fused_enabled()
