"""K5 on per-agent source descriptors (heal_warp_fuse_levels_src) and the lean inference walk built on it: every agent's map is
fused from where its pyramid stage left it -- the LiDAR agents' tensor, the camera agents' crops -- instead of from a stack of
zero-padded full-size maps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_RANGE = [-25.6, -25.6, -3, 25.6, 25.6, 1]

LEVELS = [(16, 64, 64), (32, 32, 32), (64, 16, 16)]       # (C, H, W)
# agents 0 (ego) and 1: full maps, no crop window.  Agent 2: box == window +- 1 exactly.  Agent 3: a box on the map's border (its
# window touches the border too, so window +- 1 is clipped there; 48 x 48 at level 0: larger than the kernel's 32 x 32 staging tile).  Every x0 and every box width is a multiple of 4 floats: the
# dense-crop form of a box then meets the 16-byte rule.
WINDOWS = [[None, None, (13, 43, 9, 39), (0, 46, 20, 64)],
           [None, None, (7, 21, 5, 19), (0, 15, 20, 32)],
           [None, None, (3, 11, 5, 11), (0, 8, 10, 16)]]
BOXES = [[None, None, (12, 44, 8, 40), (0, 48, 16, 64)],
         [None, None, (6, 22, 4, 20), (0, 16, 16, 32)],
         [None, None, (2, 12, 4, 12), (0, 12, 8, 16)]]


def _rows(pose):
    """Affine rows (normalised coordinates): the ego, a rotation + shift, two milder poses.  pose "off" moves agent 2 wholly off the
    ego grid (all its scores are zero); "zoom" scales agent 3's row by 2.5, so that the source footprint of a 16 x 16 ego tile (40
    pixels) exceeds the 32 x 32 staging tile and that boxed agent goes through the kernel's direct-gather fallback at level 0."""
    def row(theta, tx, ty, k=1.0):
        c, s = k * np.cos(theta), k * np.sin(theta)
        return [[c, -s, tx], [s, c, ty]]
    return np.asarray([row(0.0, 0.0, 0.0), row(0.3, 0.21, -0.13), row(-0.2, 5.0 if pose == "off" else 0.11, 0.07),
                       row(0.1, -0.17, -0.35, 2.5 if pose == "zoom" else 1.0)], dtype=np.float64)


@pytest.fixture(scope="module")
def k5_case():
    """Seeded source maps (non-trivial everywhere, finite) and the stacked, zero-padded tensors heal_warp_fuse_levels reads."""
    g = torch.Generator().manual_seed(1234)
    src_f, src_o, ref_f, ref_o = [], [], [], []
    for l, (C, H, W) in enumerate(LEVELS):
        f = (torch.randn((4, C, H, W), generator=g) * 2 + 0.5).cuda()
        o = (torch.randn((4, 1, H, W), generator=g) * 1.5).cuda()
        rf, ro = f.clone(), o.clone()
        for a in (2, 3):
            y0, y1, x0, x1 = BOXES[l][a]
            rf[a], ro[a] = 0, 0
            rf[a, :, y0:y1, x0:x1] = f[a, :, y0:y1, x0:x1]
            ro[a, :, y0:y1, x0:x1] = o[a, :, y0:y1, x0:x1]
        src_f.append(f); src_o.append(o); ref_f.append(rf); ref_o.append(ro)
    return src_f, src_o, ref_f, ref_o


def _sources(src_f, src_o, form, boxes=BOXES):
    out = []
    for l, (C, H, W) in enumerate(LEVELS):
        level = []
        for a in range(4):
            y0, y1, x0, x1 = boxes[l][a] or (0, H, 0, W)
            f, o = src_f[l][a, :, y0:y1, x0:x1], src_o[l][a, 0, y0:y1, x0:x1]
            if form == "dense":
                f, o = f.contiguous(), o.contiguous()
            level.append((f, o, (y0, x0)))
        out.append(level)
    return out


SHAPES = [(H, W) for _, H, W in LEVELS]


@pytest.mark.parametrize("pose", ["plain", "off", "zoom"])
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("form", ["dense", "slice"])
def test_k5_sources_bit_equal_the_stacked_kernel(k5_case, form, f64, pose):
    """heal_warp_fuse_levels_src on dense crops / on windows of the (non-zero outside the boxes) source stack == heal_warp_fuse_levels
    on the zero-filled stack with the boxes pasted in, bit for bit."""
    from heal_amd import ops
    src_f, src_o, ref_f, ref_o = k5_case
    rows = _rows(pose)
    want = ops.warp_fuse_levels(ref_f, ref_o, rows, f64, WINDOWS)
    got = ops.warp_fuse_levels_src(_sources(src_f, src_o, form), SHAPES, rows, f64, WINDOWS)
    torch.cuda.synchronize()
    for l, (w, g) in enumerate(zip(want, got)):
        assert w.shape == g.shape and torch.isfinite(w).all()
        assert torch.equal(w, g), (l, float((w - g).abs().max()))
    if pose != "off" and form == "dense" and f64:
        # the boxed agents take part: without agent 2 the result differs
        only = [[w if a != 2 else (0, 1, 0, 1) for a, w in enumerate(ws)] for ws in WINDOWS]
        other = ops.warp_fuse_levels(ref_f, ref_o, rows, f64, only)
        assert all(not torch.equal(w, o) for w, o in zip(want, other))


def test_k5_sources_host_checks(k5_case):
    """A window that is not inside its box (+- 1), an agent without a window on less than the full map and a misaligned box are
    refused before anything is launched: the outputs keep what they held."""
    from heal_amd import ops
    from heal_amd._capi import HealAmdError
    src_f, src_o, _, _ = k5_case
    rows = _rows("plain")

    def boxes_with(level, agent, box):
        b = [list(r) for r in BOXES]
        b[level][agent] = box
        return b

    # message of the check that must refuse -> (form, boxes)
    cases = {"is not inside its box": ("slice", boxes_with(0, 2, (13, 43, 9, 39))),     # box == window: the bilinear ring is missing
             "must be the full": ("slice", boxes_with(1, 1, (0, 32, 4, 32))),            # no window, not the full map
             "misaligned box": ("dense", boxes_with(0, 2, (12, 44, 6, 42)))}             # ring inside, column 0 8 bytes off a 16-byte line
    for name, (form, boxes) in cases.items():
        outs = [torch.full((C, H, W), 7.0, device="cuda") for C, H, W in LEVELS]
        with pytest.raises(HealAmdError, match=name):
            ops.warp_fuse_levels_src(_sources(src_f, src_o, form, boxes), SHAPES, rows, True, WINDOWS, outs=outs)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs), name


# ---- the model: lean key on against off ---------------------------------------------------------------------------------------------
def _small_pipe_and_scene_cls(golden):
    from heal_amd import configs
    from heal_amd.pipeline import Scene, ScenePipeline
    g = golden("hetero_small")
    dims = {m: tuple(int(v) for v in g[f"{m}_imgs"].shape[-2:]) for m in ("m2", "m4")}

    class SmallScene(Scene):
        CAMERA_DIMS = dims

    pipe = ScenePipeline(configs.heal_heter(("m1", "m2", "m4"), SMALL_RANGE, cam_bound=12.8, cam_dims=dims), "cuda:0", seed=0)
    return pipe, SmallScene


@pytest.fixture(scope="module")
def small():
    import os
    root = os.path.dirname(os.path.abspath(__file__))
    return _small_pipe_and_scene_cls(lambda name: np.load(os.path.join(root, "golden", name + ".npz")))


@pytest.mark.parametrize("mods,lean_taken", [(["m1", "m1", "m2", "m4"], True), (["m2", "m4", "m1"], True),
                                             (["m1", "m2", "m1"], False)])
def test_lean_walk_equals_the_stacked_walk(small, mods, lean_taken):
    """HeterPyramidCollab with the lean key on against off at the reduced size of the hetero golden test: cls / reg / dir to 1e-5 of
    their scale (the bar of test_round6_work_skipping_paths_equal_the_plain_walk; whether they are bit-equal goes on record).  A
    camera agent between two LiDAR agents has no contiguous split: the model takes the plain walk by itself (the full output)."""
    from heal_amd.opencood.models._heter_common import LEAN_WALK_KEY
    from tests.report import note
    pipe, SmallScene = small
    scene = SmallScene(len(mods), seed=31, device="cuda:0", modalities=mods)
    with torch.no_grad():
        off = pipe.model(scene.model_input())
        off = {k: off[k].clone() for k in ("cls_preds", "reg_preds", "dir_preds")}
        on = pipe.model(dict(scene.model_input(), **{LEAN_WALK_KEY: True}))
    torch.cuda.synchronize()
    assert ("occ_single_list" not in on) == lean_taken
    errs, equal = {}, {}
    for k, a in off.items():
        assert a.shape == on[k].shape and float(a.abs().max()) > 0
        errs[k] = float((a - on[k]).abs().max() / a.abs().max())
        equal[k] = bool(torch.equal(a, on[k]))
    note("lean_walk_vs_stacked_" + "_".join(mods), **errs, **{f"bit_equal_{k}": v for k, v in equal.items()})
    print("lean walk", mods, errs, equal)
    assert all(v < 1e-5 for v in errs.values()), errs


def test_lean_walk_with_a_cropped_second_stage_equals_the_stacked_walk(small, monkeypatch):
    """At full size (256^2 maps, camera content on 64..192) stage 1 of the camera agents is a crop too -- the branch the benchmark's
    scene takes: its input is the cached zero response pre-cropped to the stage's input crop with the valid stage-0 box pasted in.
    PyramidFusion.forward_collab_lean on the LiDAR tensor + unpadded camera maps against forward_collab on the zero-padded stack,
    synthetic inputs: the decoded fused map to 1e-5 of its scale.  Under capture the lean walk applies only once the pre-cropped
    response is cached (else the plain walk is taken)."""
    from heal_amd import derived
    pipe, _ = small
    model, pyr = pipe.model, pipe.model.pyramid_backbone
    mods = ["m1", "m2", "m4"]
    g = torch.Generator().manual_seed(77)
    lidar = torch.randn((1, 64, 256, 256), generator=g).cuda()
    cams = [torch.randn((64, 128, 128), generator=g).cuda() for _ in range(2)]
    stack = torch.zeros((3, 64, 256, 256), device="cuda")
    stack[0] = lidar[0]
    for j, c in enumerate(cams):
        stack[1 + j, :, 64:192, 64:192] = c
    boxes = {"m2": (64, 192, 64, 192), "m4": (64, 192, 64, 192)}
    affine = np.tile(np.asarray([[1.0, 0, 0], [0, 1.0, 0]]), (1, 5, 5, 1, 1))
    for a, (th, tx, ty) in enumerate([(0.0, 0.0, 0.0), (0.25, 0.2, -0.1), (-0.4, -0.15, 0.3)]):
        affine[0, 0, a] = [[np.cos(th), -np.sin(th), tx], [np.sin(th), np.cos(th), ty]]
    with torch.no_grad():
        plan = pyr._camcrop_plan(stack, (1, 3), boxes["m2"])
        assert plan[0] is not None and plan[1] is not None       # the case under test: stage 1 is a crop
        want, _ = pyr.forward_collab(stack, [3], affine, mods, model.cam_crop_info, True, cam_boxes=boxes)
        # capture readiness of the new cached tensor: stale weights -> rebuild the zero response alone -> the crop slot is not ready
        next(pyr.resnet.parameters()).add_(0)
        pyr._zero_response(stack)
        monkeypatch.setattr(derived, "capturing", lambda: True)
        assert pyr.lean_plan(lidar, [3], mods, boxes, model.cam_crop_info) is None
        monkeypatch.setattr(derived, "capturing", lambda: False)
        lean = pyr.lean_plan(lidar, [3], mods, boxes, model.cam_crop_info)
        assert lean is not None
        got = pyr.forward_collab_lean(lidar, cams, lidar, lean, affine, mods, model.cam_crop_info, boxes, True)
        monkeypatch.setattr(derived, "capturing", lambda: True)
        assert pyr.lean_plan(lidar, [3], mods, boxes, model.cam_crop_info) is not None
        monkeypatch.setattr(derived, "capturing", lambda: False)
    torch.cuda.synchronize()
    assert want.shape == got.shape and float(want.abs().max()) > 0
    err = float((want - got).abs().max() / want.abs().max())
    print("lean walk, cropped stage 1:", err, "bit-equal:", bool(torch.equal(want, got)))
    assert err < 1e-5, err


def test_lean_walk_graph_replay_equals_eager(small, monkeypatch):
    """Capture the step on one frame, replay it on another: the boxes equal the eager lean step's (tolerances of
    test_shared_k4_launch_equals_one_launch_per_modality)."""
    from heal_amd import ops
    pipe, SmallScene = small
    mods = ["m1", "m2", "m4"]
    calls, real = [], ops.warp_fuse_levels_src
    monkeypatch.setattr(ops, "warp_fuse_levels_src", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    scene, other = SmallScene(3, seed=21, device="cuda:0", modalities=mods), SmallScene(3, seed=22, device="cuda:0", modalities=mods)
    with torch.no_grad():
        pipe.calibrate_cls_bias(scene, target_candidates=200)      # random heads: make decode + NMS return boxes
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
        pipe.capture(scene, warmup=1)
        pipe.replay(other)
        gb, gs = pipe.replay(other)
        eb, es = pipe.step(other)
    torch.cuda.synchronize()
    assert len(calls) == 3          # warm-up, capture, eager step: all by the lean walk
    assert (gb is None) == (eb is None)
    assert eb is not None and eb.shape[0] > 0
    assert gb.shape == eb.shape and torch.allclose(gb, eb, atol=1e-3) and torch.allclose(gs, es, atol=1e-4)
