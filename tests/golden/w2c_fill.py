"""Parameter fill for models with Where2comm / Who2com fusion, shared by tests/golden/gen_golden_where2comm.py (which fills the
reference's modules) and the tests (which fill this repository's).

detfill.fill_module's sinusoids may leave the per-head logits of EncodeLayer's attention nearly equal over the agents (a uniform
softmax is a plain mean of the values: a fixture filled that way cannot tell the heads apart, nor a wrong scale from a right one).
Every EncodeLayer below `module` is therefore filled from seeded Gaussians (numpy's Generator, one stream per parameter name):
matrices with std 0.5 / sqrt(C), biases and LayerNorm offsets with std 0.2, LayerNorm gains 1 + std 0.2.  Everything else keeps
detfill's values (Who2comFusion's attention has no parameters)."""
import zlib

import numpy as np
import torch

from tests.golden.detfill import fill_module

SEED = 20240
MATRIX_STD = 0.5          # x 1 / sqrt(C)
OFFSET_STD = 0.2


def fill_encode_layer(layer, seed=SEED):
    with torch.no_grad():
        for name, p in layer.state_dict().items():
            rng = np.random.default_rng(seed + zlib.crc32(name.encode()) % 100000)
            v = rng.standard_normal(tuple(p.shape))
            if p.dim() == 2:
                v = v * (MATRIX_STD / np.sqrt(p.shape[1]))
            elif name.startswith("norm") and name.endswith("weight"):
                v = 1.0 + OFFSET_STD * v
            else:
                v = OFFSET_STD * v
            p.copy_(torch.from_numpy(v.astype(np.float32)))
    return layer


def fill_w2c(module, seed=SEED):
    """fill_module, then fill_encode_layer on every EncodeLayer below `module` (matched by class name: the reference's and this
    repository's)."""
    fill_module(module)
    for m in module.modules():
        if type(m).__name__ == "EncodeLayer":
            fill_encode_layer(m, seed)
    return module
