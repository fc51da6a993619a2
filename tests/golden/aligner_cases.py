"""The six aligner cases shared by tests/golden/gen_golden_aligners.py and the aligner tests: AlignNet's `args` per name and the
input shape.  CBAM's reduction is fixed at 16, so its `dim` is a multiple of 16; FANet pools twice, so its map is divisible by 4,
and at dim 16 its parameters are a few tens of thousands instead of 439 k at dim 64."""

SHAPE = (2, 64, 12, 20)            # N = 240 pixels, two different images
FANET_SHAPE = (2, 16, 12, 20)

CASES = {
    "resnet1x1": {"num_of_blocks": 2, "dim": 64},
    "resnet3x3": {"num_of_blocks": 1, "dim": 64},
    "scaligner": {"num_of_blocks": 2, "num_of_layers": 2, "dim": 64},
    "cbam": {"num_of_blocks": 2, "dim": 64},
    "fanet": {"dim": 16},
    "sdta": {"num_of_blocks": 1, "dim": 64},
}


def aligner_args(name):
    return {"core_method": name, "spatial_align": False, "args": dict(CASES[name])}


def input_shape(name):
    return FANET_SHAPE if name == "fanet" else SHAPE
