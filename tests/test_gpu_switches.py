"""heal_amd.switches is what the launch path consults: a switch set between two calls of one process changes the kernel that runs,
and a value outside the declared set raises before anything is launched."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAMES = ("HEAL_C3_ALGO", "HEAL_C3_KSPLIT", "HEAL_WG_WAVES", "HEAL_WG_KC", "HEAL_CONV1X1", "HEAL_C1_KSPLIT", "HEAL_C1_TILED",
         "HEAL_ARITH")


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def test_switch_set_between_calls_reroutes_the_launch():
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    from heal_amd.opencood.models.sub_modules import bev_blocks
    saved_env = {k: os.environ.pop(k, None) for k in NAMES}
    saved_timing, saved_shapes = ops.TIMING, dict(bev_blocks.LIBRARY_CONV_SHAPES)
    g = torch.Generator().manual_seed(5)
    try:
        # 1. dense 3x3, one Winograd block: below the 96-block crossover the implicit GEMM runs unless the switch says otherwise.
        # Exact on both kernels: |x| <= 3, |w| <= 2, 8 input channels -- every partial sum is a quarter-integer far below 2^24.
        x, w = _ints(g, (1, 8, 16, 16), -3, 3), _ints(g, (16, 8, 3, 3), -2, 2)
        ref = F.conv2d(x.double(), w.double(), padding=1).float()
        ops.TIMING = {}
        direct = ops.conv3x3(x.cuda(), w.cuda())
        assert sorted(ops.TIMING) == ["conv3x3_8_16"]
        os.environ["HEAL_C3_ALGO"] = "winograd"
        wino = ops.conv3x3(x.cuda(), w.cuda())
        assert sorted(ops.TIMING) == ["conv3x3_8_16", "conv3x3w_8_16"] and all(len(v) == 1 for v in ops.TIMING.values())
        assert torch.equal(direct.cpu(), ref) and torch.equal(wino.cpu(), ref)
        os.environ["HEAL_C3_ALGO"] = "winograd3"
        before = {k: len(v) for k, v in ops.TIMING.items()}
        with pytest.raises(HealAmdError, match="HEAL_C3_ALGO.*winograd3"):
            ops.conv3x3(x.cuda(), w.cuda())
        assert {k: len(v) for k, v in ops.TIMING.items()} == before
        del os.environ["HEAL_C3_ALGO"]

        # 2. pointwise convolution through the model's dispatcher: HEAL_CONV1X1 is read per call, not when the module is imported
        x, w = _ints(g, (1, 32, 8, 8), -3, 3), _ints(g, (64, 32, 1, 1), -2, 2)
        ref = F.conv2d(x.double(), w.double()).float()
        ops.TIMING = {}
        key = (32, 64, (1, 1), 1, 0, 1, 1, 8, 8)
        bev_blocks.LIBRARY_CONV_SHAPES.pop(key, None)            # the library path warns once per shape and process
        shapes = dict(bev_blocks.LIBRARY_CONV_SHAPES)
        kernel = bev_blocks.conv_bias_act(x.cuda(), w.cuda(), None, 1, 0, relu=False)
        assert sorted(ops.TIMING) == ["conv1x1_32_64"] and bev_blocks.LIBRARY_CONV_SHAPES == shapes
        os.environ["HEAL_CONV1X1"] = "0"
        ops.TIMING = {}
        with pytest.warns(RuntimeWarning, match="library"):
            library = bev_blocks.conv_bias_act(x.cuda(), w.cuda(), None, 1, 0, relu=False)
        assert bev_blocks.LIBRARY_CONV_SHAPES == {**shapes, key: 1}
        assert not [k for k in ops.TIMING if k.startswith("conv1x1_")]
        assert torch.equal(kernel.cpu(), ref) and torch.equal(library.cpu(), ref)
    finally:
        ops.TIMING = saved_timing
        bev_blocks.LIBRARY_CONV_SHAPES.clear()
        bev_blocks.LIBRARY_CONV_SHAPES.update(saved_shapes)
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
