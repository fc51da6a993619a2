"""Generate tests/golden/aligners_small.npz and tests/golden/aligners_state_dict_keys.json by IMPORTING the reference (build
container only).

    python -m tests.golden.gen_golden_aligners

For each of the six aligners of opencood/models/sub_modules/feature_alignnet.py beyond identity / convnext (the cases of
tests/golden/aligner_cases.py), in eval() mode, fp32 on the CPU: the randomised state dict, an input and the reference's output;
for `sdta` also the output of every ConvEncoder / SDTAEncoder, taken by forward hooks (`sdta/hook/<index>`; the last one is the
aligner's output and is stored once).  The json lists every case's state-dict keys in the reference's order.

The parameters are drawn where the reference's initialisation would hide an error: gamma, gamma_xca (initialised to 1e-6) in
[0.5, 1.5]; a distinct temperature in [1, 8] per head; BatchNorm statistics and affine parameters random with variances in
[0.5, 2]; weights of fan-in f uniform in [-1, 1] / sqrt(f) x 1.5.  Every value is one of 17 levels of its range and the inputs are
multiples of 1/8, which is what lets six state dicts and nine maps fit a file below 1 MiB; nothing in the arithmetic is special
about such values.

Printed and asserted here, because the reference is not there when the tests run: tests/align_refs.py's float64 SDTAEncoder
against the reference's SDTAEncoder run in float64 (<= 1e-12 of the largest magnitude), and the reference's fp32 run against its
float64 run (the bound of tests/test_align_refs_cpu.py)."""
import copy
import json
import os

import numpy as np
import torch

from tests import align_refs
from tests.golden import aligner_cases as A
from tests.golden import ref_import as R
from tests.golden.gen_golden import OUT, save

TEMPERATURES = (1.5, 3.25, 5.0, 7.5)


def levels(gen, shape, lo, hi):
    k = torch.randint(0, 17, tuple(shape), generator=gen).to(torch.float32)
    return lo + (hi - lo) * k / 16.0


def randomise(model, gen):
    sd = model.state_dict()
    for name, v in sd.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            continue
        if leaf == "temperature":
            new = torch.tensor(TEMPERATURES[:v.numel()], dtype=torch.float32).reshape(v.shape)
        elif leaf == "running_var":
            new = levels(gen, v.shape, 0.5, 2.0)
        elif leaf in ("gamma", "gamma_xca") or (leaf == "weight" and v.dim() == 1):
            new = levels(gen, v.shape, 0.5, 1.5)
        elif v.dim() == 1:                                   # biases, running means
            new = levels(gen, v.shape, -0.5, 0.5)
        else:
            fan_in = int(np.prod(v.shape[1:]))
            new = levels(gen, v.shape, -1.0, 1.0) * (1.5 / np.sqrt(fan_in))
        v.copy_(new)
    model.load_state_dict(sd)
    return {k: v.clone() for k, v in sd.items()}


def main():
    R.install()
    F = R.ref("opencood.models.sub_modules.feature_alignnet")
    M = R.ref("opencood.models.sub_modules.feature_alignnet_modules")
    gen = torch.Generator().manual_seed(20)
    out, keys = {}, {}
    x64 = levels(gen, A.SHAPE, -2.0, 2.0)
    x16 = levels(gen, A.FANET_SHAPE, -2.0, 2.0)
    out["input"], out["input_fanet"] = x64.numpy(), x16.numpy()
    for name in A.CASES:
        model = F.AlignNet(copy.deepcopy(A.aligner_args(name))).eval()
        sd = randomise(model, gen)
        keys[name] = list(sd)
        for k, v in sd.items():
            out[f"{name}/sd/{k}"] = v.numpy()
        x = x16 if name == "fanet" else x64
        hooks = []
        if name == "sdta":
            blocks = list(model.channel_align.model)
            for m in blocks:
                m.register_forward_hook(lambda mod, inp, res: hooks.append(res.detach().clone()))
        with torch.no_grad():
            y = model(x.clone())
        assert y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and 0.1 < float(y.abs().max()) < 1e3, (name, y.abs().max())
        if name == "sdta":
            assert len(hooks) == len(blocks) and torch.equal(hooks[-1], y)
            for i, h in enumerate(hooks):
                out[f"sdta/hook/{i}"] = h.numpy()
            # the reference in float64 on the same parameters: the yardstick's yardstick
            m64 = copy.deepcopy(model).double()
            h64 = []
            for m in m64.channel_align.model:
                m.register_forward_hook(lambda mod, inp, res: h64.append(res.detach().clone()))
            with torch.no_grad():
                m64(x.double())
            h64 = h64[len(h64) - len(blocks):]
            for i, m in enumerate(blocks):
                scale = float(h64[i].abs().max())
                print(f"sdta block {i} ({type(m).__name__}): reference fp32 against its float64 run "
                      f"{float((hooks[i].double() - h64[i]).abs().max()) / scale:.3e} of the largest magnitude {scale:.3f}")
                if isinstance(m, M.SDTAEncoder):
                    prefix = f"channel_align.model.{i}."
                    got = align_refs.sdta_encoder(h64[i - 1].numpy(), {k: v.numpy() for k, v in sd.items()}, prefix)
                    err = float(np.abs(got - h64[i].numpy()).max()) / scale
                    print(f"sdta block {i}: align_refs.sdta_encoder against the reference in float64 {err:.3e}")
                    assert err <= 1e-12, err
        else:
            out[f"{name}/output"] = y.numpy()
    save("aligners_small", **out)
    size = os.path.getsize(os.path.join(OUT, "aligners_small.npz"))
    assert size < (1 << 20), size
    with open(os.path.join(OUT, "aligners_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
