"""Generate tests/golden/ssfa_small.npz and tests/golden/ssfa_state_dict_keys.json by IMPORTING the reference (build container
only).

    python -m tests.golden.gen_golden_ssfa

The reference's SSFA and Head (opencood/models/sub_modules/cia_ssd_utils.py, pure torch) in eval() mode, fp32 on the CPU: the
randomised state dicts, an input, SSFA's output with the hooked `x_middle_0` (deconv_block_0(x_trans_1) + x_trans_0, the input of
conv_0), `x_output_0` (the output of conv_0) and `x_weight` (the softmax over the two attention maps), and Head's four maps on
SSFA's output.  The json lists the state-dict keys in the reference's order: `ssfa`, `head` (use_dir) and `head_no_dir`,
`shrink_conv` (DownsampleConv), and the `ssfa.` / `shrink_conv.` / head subtrees of SecondSSFA and SecondSSFAUncertainty composed
from the classes that import here (the full models need spconv).

SSFA hard-codes 128 and 256 channels: 2.9 M weights.  To fit the committed-file limit every convolution weight is one of three
levels (-s, 0, +s with probabilities 1/8, 3/4, 1/8, s = 2 / sqrt(fan-in)), the BatchNorm parameters and statistics one of 17 levels
of a non-trivial range (variances in [0.5, 2], means in [-0.5, 0.5]), the input a multiple of 1/8 on a 2 x 128 x 6 x 10 map (x_1 is
3 x 5: odd, so the transposed convolution's last odd row and column are in play).  Nothing in the arithmetic is special about such
values.

Printed here, because the reference is not there when the tests run: the reference's fp32 run against its float64 run."""
import copy
import json
import os

import numpy as np
import torch
import torch.nn as nn

from tests.golden import ref_import as R
from tests.golden.gen_golden import OUT, save

SHAPE = (2, 128, 6, 10)
HEAD = {"num_input": 128, "num_pred": 14, "num_cls": 2, "num_iou": 2, "use_dir": True, "num_dir": 4}
SHRINK = {"kernal_size": [3], "stride": [1], "padding": [1], "dim": [128], "input_dim": 128}


def levels(gen, shape, lo, hi):
    k = torch.randint(0, 17, tuple(shape), generator=gen).to(torch.float32)
    return lo + (hi - lo) * k / 16.0


def randomise(model, gen):
    sd = model.state_dict()
    for name, v in sd.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            continue
        if leaf == "running_var":
            new = levels(gen, v.shape, 0.5, 2.0)
        elif leaf == "weight" and v.dim() == 1:
            new = levels(gen, v.shape, 0.5, 1.5)
        elif v.dim() == 1:                                   # biases, running means
            new = levels(gen, v.shape, -0.5, 0.5)
        else:                                                # convolutions; a transposed one sums over dim 0
            transposed = "deconv" in name
            fan_in = int(np.prod(v.shape[2:])) * int(v.shape[0] if transposed else v.shape[1])
            if transposed:
                fan_in //= 4                                 # 9 taps serve 4 outputs
            k = torch.randint(0, 8, tuple(v.shape), generator=gen)
            new = torch.tensor([-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])[k] * float(2.0 / np.sqrt(fan_in))
        v.copy_(new)
    model.load_state_dict(sd)
    return {k: v.clone() for k, v in sd.items()}


def main():
    R.install()
    C = R.ref("opencood.models.sub_modules.cia_ssd_utils")
    D = R.ref("opencood.models.sub_modules.downsample_conv")
    gen = torch.Generator().manual_seed(27)
    out = {}
    x = levels(gen, SHAPE, -2.0, 2.0)
    out["input"] = x.numpy()

    ssfa = C.SSFA({"feature_num": 128}).eval()
    sd = randomise(ssfa, gen)
    for k, v in sd.items():
        out[f"ssfa/sd/{k}"] = v.numpy()
    hooks = {}
    ssfa.conv_0.register_forward_hook(lambda mod, inp, res: hooks.update(x_middle_0=inp[0].detach().clone(),
                                                                         x_output_0=res.detach().clone()))
    ssfa.w_0.register_forward_hook(lambda mod, inp, res: hooks.update(w0=res.detach().clone()))
    ssfa.w_1.register_forward_hook(lambda mod, inp, res: hooks.update(w1=res.detach().clone()))
    with torch.no_grad():
        y = ssfa(x.clone())
    hooks["x_weight"] = torch.softmax(torch.cat([hooks.pop("w0"), hooks.pop("w1")], dim=1), dim=1)
    assert y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and 0.1 < float(y.abs().max()) < 1e3, y.abs().max()
    pa = hooks["x_weight"][:, 0]
    print(f"output magnitude {float(y.abs().max()):.3f}; attention weight of branch 0 in [{float(pa.min()):.3f}, "
          f"{float(pa.max()):.3f}], mean {float(pa.mean()):.3f}")
    assert 0.02 < float(pa.mean()) < 0.98 and float(pa.max()) - float(pa.min()) > 0.2     # the softmax is not saturated one way
    out["output"] = y.numpy()
    for k, v in hooks.items():
        out[k] = v.numpy()
    m64 = copy.deepcopy(ssfa).double()
    with torch.no_grad():
        y64 = m64(x.double())
    print(f"reference fp32 against its float64 run: {float((y.double() - y64).abs().max()) / float(y64.abs().max()):.3e} "
          "of the largest magnitude")

    head = C.Head(**HEAD).eval()
    hsd = randomise(head, gen)
    for k, v in hsd.items():
        out[f"head/sd/{k}"] = v.numpy()
    with torch.no_grad():
        h = head(y)
    for k, v in h.items():
        out[f"head/{k}"] = v.numpy()

    save("ssfa_small", **out)
    size = os.path.getsize(os.path.join(OUT, "ssfa_small.npz"))
    assert size < (1 << 20), size

    no_dir = list(C.Head(**dict(HEAD, use_dir=False)).state_dict())
    shrink = list(D.DownsampleConv(copy.deepcopy(SHRINK)).state_dict())
    conv = lambda name: [f"{name}.weight", f"{name}.bias"]                      # noqa: E731  (nn.Conv2d with bias)
    assert list(nn.Conv2d(4, 4, 1).state_dict()) == ["weight", "bias"]
    keys = {"ssfa": list(sd), "head": list(hsd), "head_no_dir": no_dir, "shrink_conv": shrink,
            # second_ssfa.py:28-36 and second_ssfa_uncertainty.py:29-51: the registration order after the sparse trunk
            "second_ssfa": ["ssfa." + k for k in sd] + ["shrink_conv." + k for k in shrink] + ["head." + k for k in hsd],
            "second_ssfa_uncertainty": (["ssfa." + k for k in sd] + ["shrink_conv." + k for k in shrink] + conv("cls_head")
                                        + conv("reg_head") + conv("unc_head") + conv("dir_head"))}
    with open(os.path.join(OUT, "ssfa_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
