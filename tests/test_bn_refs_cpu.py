"""The references and bounds of tests/bn_refs.py proved on the CPU: against float64 torch autograd of
F.relu(F.batch_norm(x, ...) + r), the fixtures' properties, the cancellation fixture against a plain fp32 E[x^2] - mean^2, six seeded
defects against the bounds, and the routing of bev_blocks.grad_bn_act / ops.bn_grad on CPU tensors.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_refs as R

F32 = np.float32


def _torch_case(fx, training, use_res, relu):
    """float64 torch autograd of the composition on a fixture -> dict of numpy arrays."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))     # noqa: E731
    x = t(fx["x"]).requires_grad_(True)
    r = t(fx["residual"]).requires_grad_(True) if use_res else None
    g, b = t(fx["gamma"]).requires_grad_(True), t(fx["beta"]).requires_grad_(True)
    rm, rv = t(fx["running_mean"]).clone(), t(fx["running_var"]).clone()
    z = F.batch_norm(x, rm, rv, g, b, training, fx["momentum"], fx["eps"])
    if r is not None:
        z = z + r
    y = F.relu(z) if relu else z
    (y * t(fx["dy"])).sum().backward()
    return {"y": y.detach().numpy(), "dx": x.grad.numpy(), "dresidual": r.grad.numpy() if r is not None else None,
            "dgamma": g.grad.numpy(), "dbeta": b.grad.numpy(), "running_mean": rm.numpy(), "running_var": rv.numpy()}


def _ref_case(fx, training, use_res, relu, defect=None):
    """The same through tests/bn_refs.py with float64 statistics (no fp32 rounding anywhere)."""
    st = R.stats_ref(fx["x"], fx["eps"], fx["momentum"], fx["running_mean"], fx["running_var"], defect=defect)
    if training:
        mean, rstd = st["mean"], st["rstd"]
    else:
        mean, rstd = fx["running_mean"].astype(np.float64), 1.0 / np.sqrt(fx["running_var"].astype(np.float64) + fx["eps"])
    y, _, _ = R.forward_ref(fx["x"], fx["residual"] if use_res else None, mean, rstd, fx["gamma"], fx["beta"], relu)
    bw = R.backward_ref(fx["dy"], fx["x"], y if relu else None, mean, rstd, fx["gamma"], relu, training, defect=defect)
    return st, y, bw


@pytest.mark.grad
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("use_res", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["odd", "wide", "pixel"])
def test_references_equal_float64_autograd(name, training, use_res, relu):
    shape, seed = R.RANDOM_FIXTURES[name]
    fx = R.fixture(shape, seed)
    want = _torch_case(fx, training, use_res, relu)
    st, y, bw = _ref_case(fx, training, use_res, relu)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())     # noqa: E731
    assert close(y, want["y"])
    assert close(bw["dx"], want["dx"])
    assert close(bw["dgamma"], want["dgamma"]) and close(bw["dbeta"], want["dbeta"])
    if use_res:
        assert close(bw["dresidual"], want["dresidual"])
    if training:
        assert close(st["running_mean"], want["running_mean"]) and close(st["running_var"], want["running_var"])
    else:
        assert np.array_equal(want["running_mean"], fx["running_mean"].astype(np.float64))


@pytest.mark.parametrize("name", sorted(R.RANDOM_FIXTURES))
def test_random_fixtures_put_outputs_on_both_sides_of_zero(name):
    shape, seed = R.RANDOM_FIXTURES[name]
    for use_res in (True, False):
        fx = R.fixture(shape, seed, residual=use_res)
        st = R.stats_ref(fx["x"], fx["eps"])
        _, z, _ = R.forward_ref(fx["x"], fx["residual"], st["mean"].astype(F32), st["rstd"].astype(F32), fx["gamma"], fx["beta"], False)
        assert (z > 0).mean() >= 0.1 and (z < 0).mean() >= 0.1, (name, use_res, (z > 0).mean())
        assert (fx["gamma"] != 0).all()


def test_cancellation_fixture_defeats_plain_fp32_moments():
    shape, seed = R.CANCELLATION
    fx = R.fixture(shape, seed, kind="cancellation")
    st = R.stats_ref(fx["x"], fx["eps"])
    assert np.abs(st["mean"] - 1000.0).max() < 0.01 and np.abs(np.sqrt(st["var"]) - 0.01).max() < 0.002
    mean32, var32 = R.stats_naive_f32(fx["x"])
    rstd32 = 1.0 / np.sqrt(np.maximum(var32.astype(np.float64), 0.0) + fx["eps"])
    assert R.ulps(rstd32, st["rstd"]) > R.STAT_ULPS
    # the fp32-rounded reference itself holds the bound
    assert R.ulps(st["mean"].astype(F32), st["mean"]) <= 0.5 and R.ulps(st["rstd"].astype(F32), st["rstd"]) <= 0.5


def _ratios(fx, defect, training=True, use_res=True, relu=True):
    """err / bound of the fp32-rounded (possibly defective) reference against the clean one, per tensor kind.  The statistics go
    through fp32 as in the kernels: the defective and the clean backward see the same fp32 mean / rstd / y."""
    clean = R.stats_ref(fx["x"], fx["eps"], fx["momentum"], fx["running_mean"], fx["running_var"])
    bad = R.stats_ref(fx["x"], fx["eps"], fx["momentum"], fx["running_mean"], fx["running_var"], defect=defect)
    mean, rstd = clean["mean"].astype(F32), clean["rstd"].astype(F32)
    res = fx["residual"] if use_res else None
    y, _, T = R.forward_ref(fx["x"], res, mean, rstd, fx["gamma"], fx["beta"], relu)
    y32 = y.astype(F32)
    want = R.backward_ref(fx["dy"], fx["x"], y32 if relu else None, mean, rstd, fx["gamma"], relu, training)
    got = R.backward_ref(fx["dy"], fx["x"], y32 if relu else None, mean, rstd, fx["gamma"], relu, training, defect=defect)
    out = {
        "mean": R.ulps(bad["mean"].astype(F32), clean["mean"]) / R.STAT_ULPS,
        "rstd": R.ulps(bad["rstd"].astype(F32), clean["rstd"]) / R.STAT_ULPS,
        "running_mean": R.max_ratio(bad["running_mean"].astype(F32), clean["running_mean"], R.K_RUNNING * R.EPS * clean["T_running_mean"]),
        "running_var": R.max_ratio(bad["running_var"].astype(F32), clean["running_var"], R.K_RUNNING * R.EPS * clean["T_running_var"]),
        "y": R.max_ratio(y32, y, R.K_FORWARD * R.EPS * T),
        "dx": R.max_ratio(got["dx"].astype(F32), want["dx"], want["k_dx"] * R.EPS * want["T_dx"]),
        "dgamma": R.max_ratio(got["dgamma"].astype(F32), want["dgamma"], R.K_DGAMMA * R.EPS * want["T_dgamma"]),
        "dbeta": R.max_ratio(got["dbeta"].astype(F32), want["dbeta"], R.K_DBETA * R.EPS * want["T_dbeta"]),
        "dresidual": 0.0 if np.array_equal(got["dresidual"], want["dresidual"]) else float("inf"),
    }
    return out


BROKEN_BY = {"mask_ge": ("dx", "dgamma", "dbeta", "dresidual"), "running_var_biased": ("running_var",), "no_dgamma_term": ("dx",),
             "no_dbeta_term": ("dx",), "eps_outside_sqrt": ("rstd",), "momentum_swapped": ("running_mean", "running_var")}


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_the_rounded_reference_holds_every_bound(name):
    shape, seed = R.RANDOM_FIXTURES[name]
    fx = R.fixture(shape, seed)
    for training in (True, False):
        for relu in (True, False):
            ratios = _ratios(fx, None, training=training, relu=relu)
            assert all(v <= 1.0 for v in ratios.values()), (training, relu, ratios)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_seeded_defect_breaks_a_bound(defect):
    assert set(BROKEN_BY) == set(R.DEFECTS)
    shape, seed = R.RANDOM_FIXTURES["odd"]
    fx = R.fixture(shape, seed)
    ratios = _ratios(fx, defect)
    for kind in BROKEN_BY[defect]:
        assert ratios[kind] > 1.0, (defect, kind, ratios)
    for kind, v in ratios.items():
        if kind not in BROKEN_BY[defect]:
            assert v <= 1.0, (defect, kind, v)


# ------------------------------------------------------------------------------------------------------------------- routing
def test_bn_grad_is_a_setter_and_a_context_manager():
    from heal_amd import ops
    assert not ops.bn_grad_enabled()                      # the default is "torch"
    with ops.bn_grad("kernel"):
        assert ops.bn_grad_enabled()
        with ops.bn_grad("torch"):
            assert not ops.bn_grad_enabled()
        assert ops.bn_grad_enabled()
    assert not ops.bn_grad_enabled()
    ops.bn_grad("kernel")
    try:
        assert ops.bn_grad_enabled()
    finally:
        ops.bn_grad("torch")
    assert not ops.bn_grad_enabled()
    with pytest.raises(ValueError):
        ops.bn_grad("fast")
    assert not ops.bn_grad_enabled()


def test_the_mode_is_not_an_environment_switch(monkeypatch):
    from heal_amd import ops, switches
    monkeypatch.setenv("HEAL_BN_GRAD", "kernel")
    assert not ops.bn_grad_enabled()
    with pytest.raises(Exception):
        switches.get("HEAL_BN_GRAD")


@pytest.mark.grad
def test_cpu_basic_block_is_bit_equal_in_kernel_mode_and_counts_module_only():
    """A training-mode BasicBlock on CPU tensors: ops.bn_grad("kernel") changes nothing (outputs, gradients, running statistics bit
    for bit) and every BatchNorm site is counted as "module"."""
    from heal_amd import ops
    from heal_amd.opencood.models.sub_modules.bev_blocks import BasicBlock
    x = torch.randn((2, 8, 6, 10), generator=torch.Generator().manual_seed(4))
    res = {}
    for mode in ("torch", "kernel"):
        torch.manual_seed(9)
        block = BasicBlock(8, 8).train()
        before = dict(ops.BN_GRAD_CALLS)
        with ops.bn_grad(mode):
            xi = x.clone().requires_grad_(True)
            out = block(xi)
            out.square().mean().backward()
        after = dict(ops.BN_GRAD_CALLS)
        assert after["forward"] == before["forward"] and after["backward"] == before["backward"]
        assert after["module"] == before["module"] + 2, (mode, before, after)
        res[mode] = ([out.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in block.parameters()]
                     + [b.clone() for b in block.buffers()])
    assert len(res["torch"]) == len(res["kernel"])
    for a, b in zip(res["torch"], res["kernel"]):
        assert torch.equal(a, b)


def test_header_declares_the_entry_points_and_every_build_has_them():
    from heal_amd import _capi, build
    sig = _capi.signatures_train_bn()
    assert set(sig) == {"heal_bn_train_supported", "heal_bn_train_workspace", "heal_bn_train_max_blocks", "heal_bn_stats",
                        "heal_bn_act_forward", "heal_bn_act_backward"}
    for other in (_capi.signatures(), _capi.signatures_train(), _capi.signatures_ext(), _capi.signatures_train_attn()):
        assert not set(sig) & set(other)
    assert _capi.HEADER_TRAIN_BN in build._deps()
    assert len(_capi.signatures(False)) == 126 and _capi.abi_version_of_header() == 13      # the inference ABI is untouched
    L = _capi.lib()
    for name, (res, args) in sig.items():
        assert hasattr(L, name), name
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == list(args), name
    assert L.heal_bn_train_supported(2, 64, 256 * 256) == 1
    assert L.heal_bn_train_supported(0, 64, 16) == 0 and L.heal_bn_train_supported(2, 0, 16) == 0
    assert L.heal_bn_train_supported(2, 64, 0) == 0 and L.heal_bn_train_supported(2, 64, 2 ** 30 + 1) == 0
    assert _capi.query("heal_bn_train_workspace", 2, 0, 16) == 0
    segs = 2 * 64 * 16
    assert _capi.query("heal_bn_train_workspace", 2, 64, 256 * 256) >= segs * 16 + 64 * 8


def test_wrappers_refuse_cpu_tensors():
    from heal_amd import _capi, ops
    x = torch.zeros(2, 3, 4, 4)
    v = torch.zeros(3)
    assert not ops.bn_train_supported(x)
    with pytest.raises(_capi.HealAmdError):
        ops.bn_stats(x, 1e-5)
    with pytest.raises(_capi.HealAmdError):
        ops.bn_act_forward(x, None, v, v, v, v, True)
    with pytest.raises(_capi.HealAmdError):
        ops.bn_act_backward(x, x, x, v, v, v, True, True)
