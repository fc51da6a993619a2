"""The region-of-interest need plan of a pyramid stage (pyramid_fuse.stage_roi_plan) against a torch reference stack, on the CPU: with
every convolution's output replaced by NaN outside its planned box (what the ROI kernels leave undefined), the stage output inside the
final box is finite and equal to the plain run -- and the plan is tight: one row or column less, on any side of any layer's box, puts
a NaN into the final box.  No GPU, no library."""
import pytest
import torch
import torch.nn.functional as F

from heal_amd.opencood.models.fuse_modules.pyramid_fuse import box_union, crop_window, k5_read_box, stage_roi_plan

NAN = float("nan")
C, WIDTH, GROUPS = 4, 8, 2      # a narrow ResNeXt bottleneck: the plan depends on kernel sizes and strides alone

# the fusion pyramid's three stages (layer_nums 3 / 5 / 8, strides 1 / 2 / 2 on a 256 x 256 input): (block strides, stage input H = W)
STAGES = {"stage0": ((1, 1, 1), 256), "stage1": ((2, 1, 1, 1, 1), 256), "stage2": ((2,) + (1,) * 7, 128)}


def _boxes(name):
    strides, size = STAGES[name]
    out = size
    for s in strides:
        out = (out - 1) // s + 1
    k5 = k5_read_box(out, out, crop_window(out, out, 2.0, 2.0))             # what K5 reads of a camera agent at this level
    return [k5, (0, out, 0, out), (0, 9, out - 12, out), (out // 2, out // 2 + 1, 5, 6), (3, 20, 0, out)]


@pytest.fixture(scope="module")
def stacks():
    g = torch.Generator().manual_seed(5)
    out = {}
    for name, (strides, size) in STAGES.items():
        blocks = []
        for j, s in enumerate(strides):
            blocks.append({"stride": s,
                           "conv1": torch.randn((WIDTH, C, 1, 1), generator=g, dtype=torch.float64),
                           "conv2": torch.randn((WIDTH, WIDTH // GROUPS, 3, 3), generator=g, dtype=torch.float64) * 0.3,
                           "conv3": torch.randn((C, WIDTH, 1, 1), generator=g, dtype=torch.float64) * 0.3,
                           "downsample": torch.randn((C, C, 1, 1), generator=g, dtype=torch.float64) if j == 0 else None})
        out[name] = (blocks, torch.randn((1, C, size, size), generator=g, dtype=torch.float64))
    return out


def _poison(t, box):
    """t with everything outside box = (y0, y1, x0, x1) replaced by NaN."""
    out = torch.full_like(t, NAN)
    y0, y1, x0, x1 = box
    out[:, :, y0:y1, x0:x1] = t[:, :, y0:y1, x0:x1]
    return out


def _run(blocks, x, plan=None, need_in=None):
    """The stage: per block relu(conv1) -> relu(grouped conv2, stride s) -> relu(conv3 + identity), identity = the input or its
    1x1 stride-s downsample.  plan: stage_roi_plan's per-block boxes -- each convolution's output is poisoned outside its box."""
    keep = (lambda t, j, name: t) if plan is None else (lambda t, j, name: _poison(t, plan[j][name]))
    if need_in is not None:
        x = _poison(x, need_in)
    for j, b in enumerate(blocks):
        s = b["stride"]
        identity = x if b["downsample"] is None else keep(F.conv2d(x, b["downsample"], stride=s), j, "downsample")
        y = keep(F.relu(F.conv2d(x, b["conv1"])), j, "conv1")
        y = keep(F.relu(F.conv2d(y, b["conv2"], stride=s, padding=1, groups=GROUPS)), j, "conv2")
        x = keep(F.relu(F.conv2d(y, b["conv3"]) + identity), j, "conv3")
    return x


CASES = [(name, i) for name in STAGES for i in range(5)]


@pytest.mark.parametrize("name,which", CASES, ids=[f"{n}-box{i}" for n, i in CASES])
def test_outputs_in_the_box_do_not_see_anything_outside_the_plan(stacks, name, which):
    blocks, x = stacks[name]
    strides, size = STAGES[name]
    box = _boxes(name)[which]
    plan, need_in = stage_roi_plan(box, strides, size, size)
    assert len(plan) == len(strides) and plan[-1]["conv3"] == box
    want = _run(blocks, x)
    got = _run(blocks, x, plan, need_in)
    y0, y1, x0, x1 = box
    assert torch.isfinite(got[:, :, y0:y1, x0:x1]).all()
    assert torch.equal(got[:, :, y0:y1, x0:x1], want[:, :, y0:y1, x0:x1])
    if box != (0, want.shape[2], 0, want.shape[3]):
        assert torch.isnan(got).any()                      # ... and the poison was really there


@pytest.mark.parametrize("name", list(STAGES))
def test_the_plan_is_tight(stacks, name):
    """Shrinking any convolution's box (or the stage input's) by one row or column on any side makes a NaN appear in the final box."""
    blocks, x = stacks[name]
    strides, size = STAGES[name]
    for box in _boxes(name)[:3]:
        plan, need_in = stage_roi_plan(box, strides, size, size)
        y0, y1, x0, x1 = box
        shrunk = []
        for j in range(len(strides)):
            for conv in ("conv1", "conv2", "conv3") + (("downsample",) if blocks[j]["downsample"] is not None else ()):
                shrunk += [(j, conv, side) for side in range(4)]
        shrunk += [(None, "input", side) for side in range(4)]
        for j, conv, side in shrunk:
            p2 = [dict(b) for b in plan]
            b = list(need_in if j is None else p2[j][conv])
            b[side] += 1 if side in (0, 2) else -1
            if j is None:
                got = _run(blocks, x, p2, tuple(b))
            else:
                p2[j][conv] = tuple(b)
                got = _run(blocks, x, p2, need_in)
            assert torch.isnan(got[:, :, y0:y1, x0:x1]).any(), (name, box, j, conv, side)


def test_plan_values_at_the_benchmark_shape():
    """Stage 2 of the flagship scene (128 x 128 in, 64 x 64 out, crop ratio 2): K5 reads rows [17, 47) x columns [16, 48); block j's
    output is needed one more row per block going back; the first block's conv1 runs at the input resolution."""
    strides, size = STAGES["stage2"]
    box = k5_read_box(64, 64, crop_window(64, 64, 2.0, 2.0))
    assert box == (17, 47, 16, 48)
    plan, need_in = stage_roi_plan(box, strides, size, size)
    for j in range(8):
        assert plan[j]["conv3"] == plan[j]["conv2"] == (17 - (7 - j), 47 + (7 - j), 16 - (7 - j), 48 + (7 - j))
    assert plan[0]["conv1"] == need_in == (19, 108, 17, 110) and plan[0]["downsample"] == (10, 54, 9, 55)
    assert plan[3]["conv1"] == plan[2]["conv3"]


def test_empty_and_invalid_boxes():
    plan, need_in = stage_roi_plan((5, 5, 0, 8), (2, 1), 32, 32)
    assert need_in == (0, 0, 0, 0) and all(b["conv1"] == (0, 0, 0, 0) for b in plan)
    with pytest.raises(ValueError):
        stage_roi_plan((0, 17, 0, 8), (2, 1), 32, 32)
    assert box_union(None, (1, 2, 3, 4)) == (1, 2, 3, 4) and box_union((0, 5, 2, 3), (1, 7, 0, 3)) == (0, 7, 0, 3)
