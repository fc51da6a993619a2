"""Parameter fill for models with DiscoNet fusion, shared by tests/golden/gen_golden_disconet.py (which fills the reference's
modules) and the tests (which fill this repository's).

detfill.fill_module alone leaves conv1_4's pre-activation between -0.66 and -0.33 at every pixel: the last ReLU clamps every logit
to zero, the softmax is uniform and the module degenerates to a plain mean, so a fixture filled that way proves nothing.  Here
conv1_4 gets alternating weights of +-4 and a zero bias: most pixels then have distinct weights per agent, and a few per cent of
the logits are still clamped (both branches of the ReLU are exercised)."""
import torch

from tests.golden.detfill import fill_module

CONV1_4_WEIGHT = [4.0, -4.0, 4.0, -4.0, 4.0, -4.0, 4.0, -4.0]


def fill_disco(module):
    """fill_module, then conv1_4.weight = [+4, -4, ...] and conv1_4.bias = 0 in every PixelWeightLayer below `module`."""
    fill_module(module)
    with torch.no_grad():
        for name, m in module.named_modules():
            if type(m).__name__ == "PixelWeightLayer":
                m.conv1_4.weight.copy_(torch.tensor(CONV1_4_WEIGHT).view(1, 8, 1, 1))
                m.conv1_4.bias.zero_()
    return module
