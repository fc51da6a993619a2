"""Host side of the dense convolution weight gradient (include/heal_amd_train.h, ops.conv_wgrad / ops.ConvGrad, bev_blocks.grad_conv):
the third header and its ctypes signatures, the exported symbols, the split policy, the switch and the CPU behaviour of the module
helper.  Needs the built library, no GPU."""
import ctypes

import pytest
import torch

from heal_amd import _capi

I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
SHAPE = [I] * 7                                     # n, cin, cout, H, W, k, stride
EXPECTED = {
    "heal_conv_wgrad_supported": (I, SHAPE),
    "heal_conv_wgrad_splits": (I, SHAPE),
    "heal_conv_wgrad_workspace": (Z, SHAPE),
    "heal_conv_wgrad": (I, [P, P] + SHAPE + [P, P, Z, P]),
}


def test_train_header_declares_the_weight_gradient_entry_points():
    """include/heal_amd_train.h holds exactly the four entry points, parsed to the ctypes lists the prototypes spell out."""
    sig = _capi.signatures_train()
    assert set(sig) == set(EXPECTED)
    for name, (res, args) in EXPECTED.items():
        assert sig[name][0] is res, name
        assert list(sig[name][1]) == args, name


def test_library_exports_and_binds_them():
    L = _capi.lib()
    for name, (res, args) in EXPECTED.items():
        assert hasattr(L, name), name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name


def test_inference_abi_is_unchanged():
    """The versioned ABI does not see the new header: the same 126 + 7 names, version 13, and no overlap."""
    assert len(_capi.signatures(False)) == 126 and len(_capi.signatures(True)) == 7
    assert set(_capi.signatures()) == set(_capi.signatures(False)) | set(_capi.signatures(True))
    assert len(_capi.declared_symbols()) == 126 and len(_capi.declared_symbols(True)) == 7
    assert not set(_capi.signatures_train()) & set(_capi.signatures())
    assert _capi.abi_version_of_header() == 13


def _tiles(n, H, W, stride):
    """Pixel tiles of heal_conv_wgrad as the header states them: R output rows x 32 output columns, R = 4 (stride 1) | 2 (stride 2)."""
    Ho, Wo, R = (H - 1) // stride + 1, (W - 1) // stride + 1, 4 if stride == 1 else 2
    return n * -(-Ho // R) * -(-Wo // 32)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("cin,cout", [(8, 16), (64, 64), (200, 300)])
def test_splits_are_monotone_in_the_pixels_and_never_empty(cin, cout, k, stride):
    """More pixels never means fewer splits, and a split always holds at least one pixel tile (splits <= tiles); the workspace is
    splits partials, or nothing for a single split."""
    L = _capi.lib()
    last = 0
    for n, H, W in [(1, 1, 1), (1, 3, 5), (1, 8, 8), (1, 9, 33), (1, 17, 64), (2, 17, 65), (2, 40, 100), (3, 64, 128),
                    (4, 128, 128), (4, 256, 256), (8, 256, 512)]:
        assert L.heal_conv_wgrad_supported(n, cin, cout, H, W, k, stride) == 1
        s = L.heal_conv_wgrad_splits(n, cin, cout, H, W, k, stride)
        assert 1 <= s <= _tiles(n, H, W, stride), (n, H, W, s)
        assert s >= last, (n, H, W, s, last)
        last = s
        ws = _capi.query("heal_conv_wgrad_workspace", n, cin, cout, H, W, k, stride)
        assert ws == (0 if s == 1 else s * cout * cin * k * k * 4)
    assert last > 1


def test_unsupported_shapes_are_refused_by_the_queries():
    L = _capi.lib()
    for bad in [(1, 8, 8, 8, 8, 5, 1), (1, 8, 8, 8, 8, 3, 3), (0, 8, 8, 8, 8, 3, 1), (1, 0, 8, 8, 8, 3, 1), (1, 8, 8, 0, 8, 1, 1)]:
        assert L.heal_conv_wgrad_supported(*bad) == 0
        assert L.heal_conv_wgrad_splits(*bad) == 0
        assert _capi.query("heal_conv_wgrad_workspace", *bad) == 0


def test_switch_is_off_by_default(monkeypatch):
    from heal_amd import ops
    monkeypatch.delenv("HEAL_CONV_GRAD", raising=False)
    assert ops.conv_grad_enabled() is False
    monkeypatch.setenv("HEAL_CONV_GRAD", "torch")
    assert ops.conv_grad_enabled() is False
    monkeypatch.setenv("HEAL_CONV_GRAD", "kernel")
    assert ops.conv_grad_enabled() is True


@pytest.mark.grad
def test_module_helper_is_inert_on_the_cpu(monkeypatch):
    """CPU tensors never reach ConvGrad: a BasicBlock with a stride-2 downsample, a DoubleConv and a plain backbone stage give
    bit-identical outputs and gradients with the switch on and off."""
    import torch.nn as nn
    from heal_amd import ops
    from heal_amd.opencood.models.sub_modules.base_bev_backbone import _PlainStage
    from heal_amd.opencood.models.sub_modules.bev_blocks import BasicBlock, DoubleConv, conv1x1
    torch.manual_seed(5)
    down = nn.Sequential(conv1x1(8, 16, 2), nn.BatchNorm2d(16))
    stage = _PlainStage([nn.ZeroPad2d(1), nn.Conv2d(8, 16, 3, stride=2, padding=0, bias=False), nn.BatchNorm2d(16), nn.ReLU(),
                         nn.Conv2d(16, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16), nn.ReLU()])
    mods = [BasicBlock(8, 16, 2, down), DoubleConv(8, 16, 3, 1, 1), stage]
    x = torch.randn(2, 8, 12, 12)
    before = dict(ops.CONV_GRAD_CALLS)
    res = {}
    for mode in ("kernel", None):
        if mode is None:
            monkeypatch.delenv("HEAL_CONV_GRAD", raising=False)
        else:
            monkeypatch.setenv("HEAL_CONV_GRAD", mode)
        outs = []
        for m in mods:
            m.train()
            m.zero_grad()
            xi = x.clone().requires_grad_(True)
            y = m(xi)
            y.square().sum().backward()
            outs.append([y.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in m.parameters()])
        res[mode] = outs
    for a, b in zip(res["kernel"], res[None]):
        assert len(a) == len(b)
        for ta, tb in zip(a, b):
            assert torch.equal(ta, tb)
    assert ops.CONV_GRAD_CALLS == before


def test_conv_wgrad_refuses_cpu_tensors():
    from heal_amd import ops
    x, g = torch.zeros(1, 8, 8, 8), torch.zeros(1, 16, 8, 8)
    assert not ops.conv_wgrad_supported(x, g, 3, 1)
    with pytest.raises(_capi.HealAmdError):
        ops.conv_wgrad(x, g, 3, 1)
