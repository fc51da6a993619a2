"""The BatchNorm training kernels on the MI355X (include/heal_amd_train_bn.h; ops.bn_stats / bn_act_forward / bn_act_backward /
BatchNormAct; bev_blocks.grad_bn_act in ops.bn_grad("kernel") mode).

Kernel level: every output lies in a NaN-filled buffer between guard regions and is compared element by element with the float64
references and the derived bounds of tests/bn_refs.py (proved on the CPU by tests/test_bn_refs_cpu.py).  Module level: the blocks of
the gradient path against a float64 CPU copy, held to the library composition's own error."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import bn_refs as R
from tests.golden.detfill import fill_module

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

F32 = np.float32
GUARD = 64                 # floats in front of and behind every device buffer (256 B: the payload stays 16-byte aligned at offset 0)
SENTINEL = 777.0


class Dev:
    """An fp32 array on the device between two guard regions; offset: floats by which the payload is moved off 16-byte alignment.
    value None: the payload is NaN (an output the kernel has to write completely)."""

    def __init__(self, shape, value=None, offset=0):
        shape = tuple(shape)
        n = int(np.prod(shape))
        self.buf = torch.full((2 * GUARD + offset + n,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        flat = self.buf[self.lo:self.hi]
        if value is None:
            flat.fill_(float("nan"))
        else:
            flat.copy_(torch.from_numpy(np.ascontiguousarray(value, dtype=F32).ravel()))
        self.t = flat.view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 * offset) % 16

    def guards_intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())

    def numpy(self):
        assert self.guards_intact(), "a kernel wrote outside its output"
        return self.t.detach().cpu().numpy()


def _poison_workspace(x):
    """The library's scratch of these operators holds NaN before every call: it need not be initialised."""
    from heal_amd import _capi, ops
    need = _capi.query("heal_bn_train_workspace", int(x.shape[0]), int(x.shape[1]), int(x.shape[2] * x.shape[3]))
    ops._workspace("bn_train", need, x.device).fill_(255)


RATIOS = {}        # tensor kind -> largest err / bound seen in this session (printed by every case)


def _note(kind, ratio, label):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)
    assert ratio <= 1.0, (label, kind, ratio)


def run_case(fx, use_res, relu, batch_stats, offset=0, label=""):
    """stats -> forward -> backward of one fixture through the wrappers, everything compared per element.  The forward and the
    backward take the KERNEL's own fp32 mean / rstd / y as inputs, as do their references.  -> dict of the results (numpy)."""
    from heal_amd import ops
    shape = fx["x"].shape
    C = shape[1]
    x = Dev(shape, fx["x"], offset)
    res = Dev(shape, fx["residual"], offset) if use_res else None
    dy = Dev(shape, fx["dy"], offset)
    gamma, beta = Dev((C,), fx["gamma"]), Dev((C,), fx["beta"])
    rm, rv = Dev((C,), fx["running_mean"]), Dev((C,), fx["running_var"])
    mean, rstd = Dev((C,)), Dev((C,))
    # ---- statistics (always checked; the frozen cases then use the running statistics instead)
    _poison_workspace(x.t)
    ops.bn_stats(x.t, fx["eps"], fx["momentum"], rm.t, rv.t, out=(mean.t, rstd.t))
    st = R.stats_ref(fx["x"], fx["eps"], fx["momentum"], fx["running_mean"], fx["running_var"])
    got_mean, got_rstd = mean.numpy(), rstd.numpy()
    _note("save_mean", R.ulps(got_mean, st["mean"]) / R.STAT_ULPS, label)
    _note("save_rstd", R.ulps(got_rstd, st["rstd"]) / R.STAT_ULPS, label)
    _note("running_mean", R.max_ratio(rm.numpy(), st["running_mean"], R.K_RUNNING * R.EPS * st["T_running_mean"]), label)
    _note("running_var", R.max_ratio(rv.numpy(), st["running_var"], R.K_RUNNING * R.EPS * st["T_running_var"]), label)
    assert x.guards_intact()
    if batch_stats:
        mu, rs = got_mean, got_rstd
        mu_t, rs_t = mean.t, rstd.t
    else:
        mu = fx["running_mean"]
        rs = (F32(1) / np.sqrt(fx["running_var"] + F32(fx["eps"]))).astype(F32)
        frozen = (Dev((C,), mu), Dev((C,), rs))
        mu_t, rs_t = frozen[0].t, frozen[1].t
    # ---- forward
    y = Dev(shape, None, offset)
    ops.bn_act_forward(x.t, res.t if res else None, mu_t, rs_t, gamma.t, beta.t, relu, out=y.t)
    want_y, _, T = R.forward_ref(fx["x"], fx["residual"] if use_res else None, mu, rs, fx["gamma"], fx["beta"], relu)
    got_y = y.numpy()
    _note("y", R.max_ratio(got_y, want_y, R.K_FORWARD * R.EPS * T), label)
    # ---- backward
    dx, dres = Dev(shape, None, offset), Dev(shape, None, offset)
    dgamma, dbeta = Dev((C,)), Dev((C,))
    _poison_workspace(x.t)
    ops.bn_act_backward(dy.t, x.t, y.t if relu else None, mu_t, rs_t, gamma.t, relu, batch_stats,
                        out=(dx.t, dres.t, dgamma.t, dbeta.t))
    bw = R.backward_ref(fx["dy"], fx["x"], got_y if relu else None, mu, rs, fx["gamma"], relu, batch_stats)
    got = {"dx": dx.numpy(), "dresidual": dres.numpy(), "dgamma": dgamma.numpy(), "dbeta": dbeta.numpy(), "y": got_y,
           "mean": got_mean, "rstd": got_rstd, "running_mean": rm.numpy(), "running_var": rv.numpy()}
    _note("dx_batch" if batch_stats else "dx_frozen", R.max_ratio(got["dx"], bw["dx"], bw["k_dx"] * R.EPS * bw["T_dx"]), label)
    _note("dgamma", R.max_ratio(got["dgamma"], bw["dgamma"], R.K_DGAMMA * R.EPS * bw["T_dgamma"]), label)
    _note("dbeta", R.max_ratio(got["dbeta"], bw["dbeta"], R.K_DBETA * R.EPS * bw["T_dbeta"]), label)
    assert np.array_equal(got["dresidual"], bw["dresidual"].astype(F32)), (label, "dresidual is not dz bit for bit")
    for d in (x, dy, gamma, beta) + ((res,) if res else ()):
        assert d.guards_intact()
    print(label, "max err/bound so far:", " ".join(f"{k}={v:.3f}" for k, v in sorted(RATIOS.items())))
    return got


# ------------------------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("batch_stats", [1, 0])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("use_res", [True, False])
@pytest.mark.parametrize("name", sorted(R.RANDOM_FIXTURES))
def test_kernels_per_element(name, use_res, relu, batch_stats):
    """(1,1,1,2), (2,3,3,5), (3,65,7,9), (2,8,1,1), (1,4,64,64), a plane of HEAL_BN_SEGMENT + 1 elements (two segments, a
    one-element tail, dword path) and a 16-byte-path map of 2.25 segments per plane; residual, ReLU and batch_stats on and off."""
    assert R.RANDOM_FIXTURES["tail"][0][3] == 4096 + 1
    shape, seed = R.RANDOM_FIXTURES[name]
    run_case(R.fixture(shape, seed), use_res, relu, batch_stats, label=f"{name} res={use_res} relu={relu} batch={batch_stats}")


def test_segment_constant_is_what_the_fixtures_assume():
    import re
    from heal_amd import _capi
    with open(_capi.HEADER_TRAIN_BN) as f:
        assert int(re.search(r"#define\s+HEAL_BN_SEGMENT\s+(\d+)", f.read()).group(1)) == 4096


@pytest.mark.parametrize("name,use_res,relu,batch_stats", [("plane", True, True, 1), ("plane", False, False, 0), ("multi", True, True, 1),
                                                          ("odd", True, True, 1)])
def test_base_pointers_offset_by_one_float(name, use_res, relu, batch_stats):
    """Every map starts one float past a 16-byte boundary: H * W % 4 == 0 alone must not select the 16-byte path.  The element-wise
    results (y, dresidual) equal the aligned call's bit for bit; the reductions, whose threads own other elements, hold the bounds."""
    shape, seed = R.RANDOM_FIXTURES[name]
    fx = R.fixture(shape, seed)
    moved = run_case(fx, use_res, relu, batch_stats, offset=1, label=f"{name} offset 1")
    base = run_case(fx, use_res, relu, batch_stats, offset=0, label=f"{name} offset 0")
    for k in ("y", "dresidual"):
        assert np.array_equal(moved[k], base[k]), k


@pytest.mark.parametrize("batch_stats", [1, 0])
def test_each_nullable_output_omitted(batch_stats):
    """dx / dresidual / dgamma / dbeta left out one at a time, and asked for one at a time: what is produced equals the full call
    bit for bit and nothing else is written."""
    from heal_amd import ops
    shape, seed = R.RANDOM_FIXTURES["wide"]
    fx = R.fixture(shape, seed)
    full = run_case(fx, True, True, batch_stats, label="nullable full")
    names = ("dx", "dresidual", "dgamma", "dbeta")
    x, dy, y = Dev(shape, fx["x"]), Dev(shape, fx["dy"]), Dev(shape, full["y"])
    C = shape[1]
    if batch_stats:
        mean, rstd = Dev((C,), full["mean"]), Dev((C,), full["rstd"])
    else:
        mean = Dev((C,), fx["running_mean"])
        rstd = Dev((C,), (F32(1) / np.sqrt(fx["running_var"] + F32(fx["eps"]))).astype(F32))
    gamma = Dev((C,), fx["gamma"])
    for want in [tuple(j != i for j in range(4)) for i in range(4)] + [tuple(j == i for j in range(4)) for i in range(4)]:
        outs = [Dev(shape if i < 2 else (C,)) for i in range(4)]
        _poison_workspace(x.t)
        got = ops.bn_act_backward(dy.t, x.t, y.t, mean.t, rstd.t, gamma.t, True, batch_stats, want=want,
                                  out=tuple(o.t if w else None for o, w in zip(outs, want)))
        for i, name in enumerate(names):
            if want[i]:
                assert got[i].data_ptr() == outs[i].t.data_ptr()
                assert np.array_equal(outs[i].numpy(), full[name]), (want, name)
            else:
                assert got[i] is None
                assert bool(torch.isnan(outs[i].t).all()) and outs[i].guards_intact(), (want, name)
    assert ops.bn_act_backward(dy.t, x.t, y.t, mean.t, rstd.t, gamma.t, True, batch_stats, want=(False,) * 4) == (None,) * 4


def test_zero_gamma_constant_channel_and_cancellation():
    """gamma = 0 in one channel (dx exactly zero there, dgamma still the sum), a constant channel (var = 0: mean exact, rstd =
    1 / sqrt(eps), xh = 0) and the cancellation fixture (channel means 1000, standard deviation 0.01), all within the bounds."""
    shape, seed = R.RANDOM_FIXTURES["odd"]
    fx = R.fixture(shape, seed)
    fx["gamma"][1] = 0.0
    fx["x"][:, 2] = F32(3.7)
    for relu in (True, False):
        got = run_case(fx, True, relu, 1, label=f"gamma0/const relu={relu}")
        assert bool((got["dx"][:, 1] == 0).all()) and np.abs(got["dgamma"][1]) > 0
        assert got["mean"][2] == F32(3.7)
        assert bool((got["y"][:, 2] == np.maximum((fx["beta"][2] + fx["residual"][:, 2]).astype(F32), 0 if relu else -np.inf)).all())
    cshape, cseed = R.CANCELLATION
    cfx = R.fixture(cshape, cseed, kind="cancellation")
    for batch in (1, 0):
        run_case(cfx, True, True, batch, label=f"cancellation batch={batch}")


def test_all_negative_output_under_relu_gives_exact_zeros():
    shape, seed = R.RANDOM_FIXTURES["wide"]
    fx = R.fixture(shape, seed)
    fx["beta"][:] = -100.0
    got = run_case(fx, False, True, 1, label="all negative")
    assert bool((got["y"] == 0).all())
    for k in ("dx", "dgamma", "dbeta", "dresidual"):
        assert bool((got[k] == 0).all()), k


@functools.lru_cache(maxsize=None)
def _determinism_inputs(name):
    shape, seed = R.RANDOM_FIXTURES[name]
    fx = R.fixture(shape, seed)
    return fx, {k: torch.from_numpy(fx[k]).cuda() for k in ("x", "dy", "residual", "gamma", "beta")}


def _pipeline(fx, t):
    """stats -> forward -> backward on plain tensors -> every result, cloned."""
    from heal_amd import ops
    rm, rv = torch.from_numpy(fx["running_mean"]).cuda(), torch.from_numpy(fx["running_var"]).cuda()
    mean, rstd = ops.bn_stats(t["x"], fx["eps"], fx["momentum"], rm, rv)
    y = ops.bn_act_forward(t["x"], t["residual"], mean, rstd, t["gamma"], t["beta"], True)
    grads = ops.bn_act_backward(t["dy"], t["x"], y, mean, rstd, t["gamma"], True, 1)
    torch.cuda.synchronize()
    return [v.clone() for v in (mean, rstd, rm, rv, y) + tuple(grads)]


@pytest.mark.parametrize("name", ["multi", "wide", "tail"])
def test_repeated_launches_and_a_one_block_grid_give_the_same_bits(name):
    """Two launches are bit-equal, and so is a launch whose grid is capped at ONE block (heal_bn_train_max_blocks, the testing hook):
    the partial sums belong to the segments, not to the blocks ("multi": 18 segments, "wide": 195, "tail": 8)."""
    from heal_amd import _capi
    fx, t = _determinism_inputs(name)
    first, second = _pipeline(fx, t), _pipeline(fx, t)
    L = _capi.lib()
    before = L.heal_bn_train_max_blocks(1)
    try:
        one_block = _pipeline(fx, t)
        assert L.heal_bn_train_max_blocks(3) == 1
        three_blocks = _pipeline(fx, t)
    finally:
        L.heal_bn_train_max_blocks(0)
    assert before == 2048 and L.heal_bn_train_max_blocks(0) == 2048
    for a, b, c, d in zip(first, second, one_block, three_blocks):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_running_statistics_after_two_consecutive_calls():
    from heal_amd import ops
    shape, seed = R.RANDOM_FIXTURES["wide"]
    fa, fb = R.fixture(shape, seed), R.fixture(shape, seed + 100)
    rm, rv = Dev((shape[1],), fa["running_mean"]), Dev((shape[1],), fa["running_var"])
    want_m, want_v = fa["running_mean"].astype(np.float64), fa["running_var"].astype(np.float64)
    T_m = T_v = 0.0
    for fx in (fa, fb):
        ops.bn_stats(torch.from_numpy(fx["x"]).cuda(), fa["eps"], fa["momentum"], rm.t, rv.t)
        st = R.stats_ref(fx["x"], fa["eps"], fa["momentum"], want_m, want_v)
        # the first call's rounding error (<= K EPS T) is carried through the second update with the factor (1 - momentum)
        T_m, T_v = (1.0 - fa["momentum"]) * T_m + st["T_running_mean"], (1.0 - fa["momentum"]) * T_v + st["T_running_var"]
        want_m, want_v = st["running_mean"], st["running_var"]
    _note("running_mean", R.max_ratio(rm.numpy(), want_m, R.K_RUNNING * R.EPS * T_m), "two calls")
    _note("running_var", R.max_ratio(rv.numpy(), want_v, R.K_RUNNING * R.EPS * T_v), "two calls")


def test_refusals(monkeypatch):
    """Wrong device or dtype, non-contiguous tensors, mismatched shapes and M < 2 in training mode raise before anything is launched."""
    from heal_amd import _capi, ops
    launched = []
    real = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    x = torch.zeros((2, 4, 6, 8), device="cuda")
    v = torch.ones(4, device="cuda")
    E = _capi.HealAmdError
    bad_maps = [x.cpu(), x.double(), x.half(), x[:, :, :, ::2], x.permute(0, 1, 3, 2), x[0], x.to(memory_format=torch.channels_last)]
    for m in bad_maps:
        assert not ops.bn_train_supported(m)
        with pytest.raises(E):
            ops.bn_stats(m, 1e-5)
        with pytest.raises(E):
            ops.bn_act_forward(m, None, v, v, v, v, True)
        with pytest.raises(E):
            ops.bn_act_backward(x, m, x, v, v, v, True, 1)
    other = [x.cpu(), x.double(), x[:, :, :, ::2], x[:1], torch.zeros((2, 4, 8, 6), device="cuda")]
    for m in other:
        with pytest.raises(E):
            ops.bn_act_forward(x, m, v, v, v, v, True)                   # residual
        with pytest.raises(E):
            ops.bn_act_forward(x, None, v, v, v, v, True, out=m)         # destination
        with pytest.raises(E):
            ops.bn_act_backward(m, x, x, v, v, v, True, 1)               # dy
        with pytest.raises(E):
            ops.bn_act_backward(x, x, m, v, v, v, True, 1)               # y
        with pytest.raises(E):
            ops.bn_act_backward(x, x, x, v, v, v, True, 1, out=(m, None, None, None))
    for w in [v.cpu(), v.double(), torch.ones(5, device="cuda"), torch.ones(8, device="cuda")[::2], v.view(4, 1)]:
        with pytest.raises(E):
            ops.bn_act_forward(x, None, w, v, v, v, True)
        with pytest.raises(E):
            ops.bn_act_forward(x, None, v, v, w, v, True)
        with pytest.raises(E):
            ops.bn_act_backward(x, x, x, v, w, v, True, 1)
        with pytest.raises(E):
            ops.bn_stats(x, 1e-5, 0.1, w, v)
        with pytest.raises(E):
            ops.bn_stats(x, 1e-5, out=(v, w))
    with pytest.raises(E):
        ops.bn_stats(x, 1e-5, 0.1, v, None)                              # running buffers go together
    with pytest.raises(E):
        ops.bn_act_backward(x, x, None, v, v, v, True, 1)                # relu without y
    with pytest.raises(E):
        ops.bn_act_backward(x, x, x, v, v, v, False, 1)                  # y without relu
    one = torch.zeros((1, 4, 1, 1), device="cuda")
    with pytest.raises(E):
        ops.bn_stats(one, 1e-5, 0.1, v.clone(), v.clone())               # M = 1: no unbiased variance
    with pytest.raises(E):
        ops.BatchNormAct.apply(one, None, v, v, v.clone(), v.clone(), True, 0.1, 1e-5, True)
    assert launched == []
    assert ops.bn_train_supported(x) and ops.bn_train_supported(one)


def test_forward_and_backward_replay_in_a_captured_graph():
    """stats + forward + backward captured once in a torch.cuda.graph, replayed with new input contents: the replay's results are
    the eager call's on the new contents, bit for bit (no host synchronisation, no pointer changes; the scratch is the capture's)."""
    from heal_amd import ops
    shape, seed = R.RANDOM_FIXTURES["multi"]
    fa, fb = R.fixture(shape, seed), R.fixture(shape, seed + 1)
    keys = ("x", "dy", "residual", "gamma", "beta")
    static = {k: torch.from_numpy(fa[k]).cuda() for k in keys}
    C = shape[1]

    def step(t, rm, rv):
        mean, rstd = ops.bn_stats(t["x"], fa["eps"], 0.1, rm, rv)
        y = ops.bn_act_forward(t["x"], t["residual"], mean, rstd, t["gamma"], t["beta"], True)
        return (mean, rstd, y) + ops.bn_act_backward(t["dy"], t["x"], y, mean, rstd, t["gamma"], True, 1)

    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static, rm, rv)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static, rm, rv)
    for k in keys:
        static[k].copy_(torch.from_numpy(fb[k]).cuda())
    rm.zero_(), rv.fill_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs] + [rm.clone(), rv.clone()]
    erm, erv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    eager = list(step({k: torch.from_numpy(fb[k]).cuda() for k in keys}, erm, erv)) + [erm, erv]
    torch.cuda.synchronize()
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    st = R.stats_ref(fb["x"], fa["eps"])
    assert R.ulps(replayed[0].cpu().numpy(), st["mean"]) <= R.STAT_ULPS and R.ulps(replayed[1].cpu().numpy(), st["rstd"]) <= R.STAT_ULPS


# ------------------------------------------------------------------------------------------------------------------ module level
def _build(kind):
    from heal_amd.opencood.models.sub_modules import bev_blocks as B
    from heal_amd.opencood.models.sub_modules.base_bev_backbone import _PlainStage
    torch.manual_seed(5)
    if kind in ("basic_s2", "basic_frozen"):
        if kind == "basic_frozen":
            m, shape = B.BasicBlock(8, 8), (2, 8, 10, 12)
        else:
            down = nn.Sequential(B.conv1x1(8, 16, 2), nn.BatchNorm2d(16))
            m, shape = B.BasicBlock(8, 16, stride=2, downsample=down), (2, 8, 11, 20)
    elif kind == "bottleneck_g32":
        m, shape = B.Bottleneck(64, 64, groups=32, base_width=4, expansion=1), (2, 64, 6, 10)
        assert m.conv2.groups == 32
    elif kind == "deblock_t":
        m = B._Deblock(nn.ConvTranspose2d(16, 8, 2, stride=2, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01))
        shape = (2, 16, 5, 7)
    else:
        m = _PlainStage([nn.ZeroPad2d(1), nn.Conv2d(8, 16, 3, stride=2, padding=0, bias=False),
                         nn.BatchNorm2d(16, eps=1e-3, momentum=0.01), nn.ReLU(),
                         nn.Conv2d(16, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16, eps=1e-3, momentum=0.01), nn.ReLU()])
        shape = (2, 8, 12, 14)
    m = fill_module(m)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(6))
    return m, x


# kind -> BatchNorm sites of one forward
SITES = {"basic_s2": 3, "bottleneck_g32": 3, "deblock_t": 1, "plain_stage": 2, "basic_frozen": 2}


def _module_run(module, x, dev, dtype, frozen):
    m = copy.deepcopy(module).to(dev).to(dtype)
    if frozen:
        m.eval().requires_grad_(False)
    else:
        m.train()
    xi = x.to(dev).to(dtype).requires_grad_(True)
    out = m(xi)
    w = torch.linspace(-1.0, 1.0, out.numel(), dtype=dtype, device=dev).view_as(out)
    (out * w).sum().backward()           # a gradient of both signs (a mean of squares would make dbeta of every site cancel)
    res = {"out": out.detach().double().cpu(), "x.grad": xi.grad.double().cpu()}
    res.update({n: p.grad.double().cpu() for n, p in m.named_parameters() if p.grad is not None})
    res.update({n: b.detach().double().cpu() for n, b in m.named_buffers()})
    return res


@pytest.mark.parametrize("kind", sorted(SITES))
def test_module_kernel_path_against_float64(kind):
    """A stride-2 BasicBlock with downsample (the three ConvBN.run forms: ReLU, no ReLU, residual + ReLU), a 32-group Bottleneck, a
    transposed-convolution _Deblock, a _PlainStage and a frozen eval-mode BasicBlock whose input carries gradient, in
    ops.bn_grad("kernel") mode: outputs, input gradient, parameter gradients and BatchNorm buffers are as close to the float64 CPU
    module as the library composition is within a factor 2, with a floor of 1e-6 of the tensor's scale; num_batches_tracked is equal.
    The routes are counted."""
    from heal_amd import ops
    module, x = _build(kind)
    frozen = kind == "basic_frozen"
    ref = _module_run(module, x, "cpu", torch.float64, frozen)
    c0 = dict(ops.BN_GRAD_CALLS)
    torch_path = _module_run(module, x, "cuda", torch.float32, frozen)
    c1 = dict(ops.BN_GRAD_CALLS)
    assert (c1["forward"], c1["backward"], c1["module"]) == (c0["forward"], c0["backward"], c0["module"] + SITES[kind])
    with ops.bn_grad("kernel"):
        kernel_path = _module_run(module, x, "cuda", torch.float32, frozen)
    c2 = dict(ops.BN_GRAD_CALLS)
    assert (c2["forward"], c2["backward"], c2["module"]) == (c1["forward"] + SITES[kind], c1["backward"] + SITES[kind], c1["module"])
    assert set(ref) == set(torch_path) == set(kernel_path)
    assert frozen == (not any(n.endswith(".weight") for n in ref))
    failures = []
    for name in ref:
        if name.endswith("num_batches_tracked"):
            assert torch.equal(kernel_path[name], ref[name]) and float(ref[name]) == (0.0 if frozen else 1.0), name
            continue
        scale = float(ref[name].abs().max())
        assert scale > 0, name
        e_kernel = float((kernel_path[name] - ref[name]).abs().max()) / scale
        e_torch = float((torch_path[name] - ref[name]).abs().max()) / scale
        print(f"{kind} {name}: kernel {e_kernel:.3e} torch {e_torch:.3e}")
        if not e_kernel <= max(2.0 * e_torch, 1e-6):
            failures.append((name, e_kernel, e_torch))
    assert not failures, failures


def test_default_mode_never_reaches_the_kernels(monkeypatch):
    from heal_amd import ops
    assert not ops.bn_grad_enabled()

    def never(*a, **k):
        raise AssertionError("BatchNormAct ran in the default mode")
    monkeypatch.setattr(ops.BatchNormAct, "forward", staticmethod(never))
    module, x = _build("basic_s2")
    res = _module_run(module, x, "cuda", torch.float32, False)
    assert bool(torch.isfinite(res["x.grad"]).all())


# Adam's first steps are lr * sign(g): a gradient entry whose sign the fp32 rounding decides moves its parameter by 2 lr, and the
# next loss by an amount proportional to lr.  At lr = 1e-4 that noise is 2e-5 .. 7e-4 of the loss for ANY fp32 run (CPU fp32 against
# float64: 2.4e-5, 3.9e-4; MI355X "torch": 2.1e-6, 6.6e-4; "kernel": 3.9e-5, 4.8e-4), i.e. a factor between two such figures says
# nothing.  At lr = 1e-6 a step still lowers the loss by 3e-3 of its size -- a wrong BatchNorm gradient would move it differently by
# a fraction of that -- while the rounding noise stays below 1e-6 (CPU fp32 against float64: 8.6e-7, 6.6e-7).
LIDAR_LR = 1e-6


def _lidar_training(device, dtype, mode):
    """Three Adam steps of the small pyramid LiDAR model (configs.lidar_pyramid on the 51.2 m range, the golden's LiDAR agents'
    voxels) on train.py's criterion with synthetic anchor labels, from one seeded initial state -> the loss before each step.
    (The library's default initialisation and the real criterion: with the closed-form test fill, or with a mean of squares of the
    heads as the loss, the fp32 gradient itself is 1 - 10 % away from the float64 one -- the loss's gradient then lies almost
    entirely in the directions a training-mode BatchNorm projects out -- and any two fp32 runs differ by as much.)"""
    import os
    from heal_amd import configs, ops
    from heal_amd.opencood.tools.train_utils import create_loss, create_model
    from tests.test_train_path import GOLD, SMALL_RANGE, synthetic_targets
    g = np.load(os.path.join(GOLD, "hetero_small.npz"), allow_pickle=True)
    n = int(g["voxel_coords"][:, 0].max()) + 1

    def t(a, d=None):
        v = torch.from_numpy(np.ascontiguousarray(a))
        return (v.to(d) if d is not None else v).to(device)
    data = {"inputs_m1": {"voxel_features": t(g["voxel_features"], dtype), "voxel_coords": t(g["voxel_coords"], torch.int32),
                          "voxel_num_points": t(g["voxel_num_points"], torch.int32)},
            "agent_modality_list": ["m1"] * n, "record_len": torch.tensor([n]), "pairwise_t_matrix": t(g["pairwise"], dtype)}
    hypes = configs.lidar_pyramid(SMALL_RANGE)
    torch.manual_seed(0)
    model = create_model(hypes).to(device).to(dtype).train()      # built on the CPU: the same parameters for every device and dtype
    criterion = create_loss(hypes)
    opt = torch.optim.Adam(model.parameters(), lr=LIDAR_LR)
    losses = []
    with ops.bn_grad(mode):
        for _ in range(3):
            opt.zero_grad()
            out = model(data)
            tgt = {k: v.to(dtype) for k, v in synthetic_targets(out, device=device).items()}
            n_agents = out["occ_single_list"][0].shape[0]
            single = {k: v.expand(n_agents, *v.shape[1:]).contiguous() for k, v in tgt.items()}
            loss = criterion(out, tgt) + criterion(out, single, suffix="_single")
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    return losses


def test_three_adam_steps_of_the_small_lidar_model():
    """Finite losses in "kernel" mode, and each step's loss as close to the float64 CPU run from the same initial state as the
    "torch"-mode run's is, within a factor 2 (floor: 1e-6 of the loss)."""
    from heal_amd import ops
    ref = _lidar_training("cpu", torch.float64, "torch")
    c0 = dict(ops.BN_GRAD_CALLS)
    torch_losses = _lidar_training("cuda", torch.float32, "torch")
    c1 = dict(ops.BN_GRAD_CALLS)
    kernel_losses = _lidar_training("cuda", torch.float32, "kernel")
    c2 = dict(ops.BN_GRAD_CALLS)
    assert c1["forward"] == c0["forward"] and c1["module"] > c0["module"]
    sites = (c1["module"] - c0["module"])
    assert c2["forward"] - c1["forward"] > 0 and c2["backward"] - c1["backward"] == c2["forward"] - c1["forward"]
    assert (c2["forward"] - c1["forward"]) + (c2["module"] - c1["module"]) == sites
    print("float64", ref, "torch", torch_losses, "kernel", kernel_losses, "kernel sites", c2["forward"] - c1["forward"], "of", sites)
    assert all(np.isfinite(v) for v in kernel_losses)
    assert kernel_losses[2] < kernel_losses[1] < kernel_losses[0] * (1.0 - 1e-3), kernel_losses      # the steps do move the loss
    for step, (r, a, b) in enumerate(zip(ref, torch_losses, kernel_losses)):
        e_torch, e_kernel = abs(a - r) / abs(r), abs(b - r) / abs(r)
        assert e_kernel <= max(2.0 * e_torch, 1e-6), (step, r, a, b)
