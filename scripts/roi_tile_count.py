"""Tiles and workgroups the region-of-interest launches of the fusion pyramid's lean walk skip, counted on the host from the plan
(PyramidFusion.lean_roi_plan) -- no GPU needed.

    python scripts/roi_tile_count.py            # the flagship scene: m1 m1 m1 m2 m4 at 256 x 256

Per convolution of every ROI stage: the 64-pixel tiles of the pointwise launch that leave at once -- box rule (heal_conv1x1_box_roi, what
the walk launches: the tiles enumerate each agent's aligned box, ops.conv1x1_box_tiles) -- or the TH x TW tiles
(heal_grouped_small_conv3x3_roi) of the camera agents' maps that hold no pixel of the agent's box, out of all tiles of all agents, and the
same in workgroups (tiles x Cout chunks of 64, or x 16-channel super-groups).  `total_tile_rule` is the same count with the pointwise
launches under heal_conv1x1_roi's tile rule (what the walk launched before the box rule).  Prints one JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def conv1x1_tiles(box, Ho, Wo, rule="box"):
    """(tiles, skipped) of one image: the rules of include/heal_amd_roi.h (a width that is no multiple of 4 keeps the tile rule)."""
    if rule == "box" and Wo % 4 == 0:
        from heal_amd import ops
        total = -(-Ho * Wo // 64)
        return total, total - len(ops.conv1x1_box_tiles(box, Ho, Wo))
    y0, y1, x0, x1 = box
    total = skipped = 0
    for p0 in range(0, Ho * Wo, 64):
        pl = min(p0 + 64, Ho * Wo) - 1
        r0, r1 = p0 // Wo, pl // Wo
        keep = y0 < y1 and x0 < x1 and r0 < y1 and r1 >= y0
        if keep and r0 == r1:
            keep = p0 - r0 * Wo < x1 and pl - r0 * Wo >= x0
        total += 1
        skipped += not keep
    return total, skipped


def gconv_tiles(box, Ho, Wo, th, tw):
    y0, y1, x0, x1 = box
    total = skipped = 0
    for oy in range(0, Ho, th):
        for ox in range(0, Wo, tw):
            keep = y0 < y1 and x0 < x1 and oy < y1 and min(oy + th, Ho) > y0 and ox < x1 and min(ox + tw, Wo) > x0
            total += 1
            skipped += not keep
    return total, skipped


def main():
    import torch
    from heal_amd import configs
    from heal_amd.opencood.models.heter_pyramid_collab import HeterPyramidCollab
    mods = ["m1", "m1", "m1", "m2", "m4"]
    model = HeterPyramidCollab(configs.heal_heter(("m1", "m2", "m4"), max_cav=5)["model"]["args"]).eval()
    pyr = model.pyramid_backbone
    H = W = 256
    c0, c1 = 3, 5
    plan = pyr._camcrop_plan(torch.zeros((3, 64, H, W)), (c0, c1), (64, 192, 64, 192))
    rois = pyr.lean_roi_plan((H, W), plan, c0, c1, mods, model.cam_crop_info)
    rows, tot = [], {"tiles": 0, "tiles_skipped": 0, "workgroups": 0, "workgroups_skipped": 0, "camera_tiles": 0}
    old = {"tiles_skipped": 0, "workgroups_skipped": 0}
    size = (H, W)
    for i in range(pyr.layernum_):
        layer = getattr(pyr.resnet, f"layer{i}")
        for j, blk in enumerate(layer):
            s = blk.stride
            out = ((size[0] - 1) // s + 1, (size[1] - 1) // s + 1)
            if i in rois:
                width, cg = blk.conv2.out_channels, blk.conv2.in_channels // blk.conv2.groups
                th, tw = (16 if cg == 4 and s == 1 else 8), (32 if s == 1 else 16)
                convs = [("conv1", size, width // 64, None), ("conv2", out, width // 16, (th, tw)), ("conv3", out, blk.conv3.out_channels // 64, None)]
                if blk.downsample is not None:
                    convs.append(("downsample", out, blk.conv3.out_channels // 64, None))
                for name, (ho, wo), chunks, tile in convs:
                    t = k = cam = 0
                    for a, box in enumerate(rois[i][j][name]):
                        ta, ka = conv1x1_tiles(box, ho, wo) if tile is None else gconv_tiles(box, ho, wo, *tile)
                        t, k = t + ta, k + ka
                        ko = conv1x1_tiles(box, ho, wo, "tile")[1] if tile is None else ka
                        old["tiles_skipped"] += ko
                        old["workgroups_skipped"] += ko * chunks
                        cam += ta if c0 <= a < c1 else 0
                    rows.append({"stage": i, "block": j, "conv": name, "map": [ho, wo], "camera_box": list(rois[i][j][name][c0]),
                                 "tiles": t, "camera_tiles": cam, "tiles_skipped": k, "workgroups": t * chunks, "workgroups_skipped": k * chunks})
                    for key in tot:
                        tot[key] += rows[-1][key]
            size = out
    tot["skipped_fraction_of_camera_tiles"] = round(tot["tiles_skipped"] / max(tot["camera_tiles"], 1), 4)
    tot["skipped_fraction_of_workgroups"] = round(tot["workgroups_skipped"] / max(tot["workgroups"], 1), 4)
    old["skipped_fraction_of_camera_tiles"] = round(old["tiles_skipped"] / max(tot["camera_tiles"], 1), 4)
    old["skipped_fraction_of_workgroups"] = round(old["workgroups_skipped"] / max(tot["workgroups"], 1), 4)
    print(json.dumps({"scene": mods, "total": tot, "total_tile_rule": old, "launches": rows}))


if __name__ == "__main__":
    main()
