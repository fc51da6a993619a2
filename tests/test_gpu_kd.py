"""DiscoNet distillation on the MI355X: heal_kd_kl_loss against the fp64 torch composition (the project's bar for backward
kernels: loss within 1e-5 relative, gradient x N*C*H*W within 1e-5 absolute), exact zeros for identical operands, bit-equal
repeats wherever the data lies, huge logits, the read-only mode, strided inputs, autograd scaling, captured-graph replay, the
loss module with the kernel on and off, and one training step of the student against the frozen teacher."""
import contextlib
import os

import numpy as np
import pytest
import torch

from heal_amd import configs, ops
from tests.test_kd_cpu import LOSS_CASES, M_RANGE, TOL, check_student, check_teacher, loss_case, m_data, m_models

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the golden cases (register-resident C = 256 and 64 with an odd map, generic C = 7 and 2, the underflow case) + C = 128
SHAPES = dict(LOSS_CASES, c128_=(2, 128, 8, 8))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "kd_small.npz"))


@pytest.fixture(scope="module")
def maps(g):
    """prefix -> (student, teacher) on the device: the fixture's maps (standard deviation 1.5, teacher independent of the student)
    and a seeded C = 128 pair of the same kind.  Read-only."""
    out = {}
    for prefix in LOSS_CASES:
        o, _ = loss_case(g, prefix, DEV)
        out[prefix] = (o["feature"].detach(), o["teacher_feature"])
    gen = torch.Generator().manual_seed(128)
    out["c128_"] = tuple((torch.randn(SHAPES["c128_"], generator=gen) * 1.5).to(DEV) for _ in range(2))
    return out


def fp64(student, teacher):
    """(loss, gradient x numel) of the reference's composition in fp64, with kl_div's 0 * log 0 = 0."""
    C = student.shape[1]
    s = student.double().permute(0, 2, 3, 1).reshape(-1, C)
    t = teacher.double().permute(0, 2, 3, 1).reshape(-1, C)
    ls, lt = torch.log_softmax(s, 1), torch.log_softmax(t, 1)
    pt = lt.exp()
    loss = (torch.xlogy(pt, pt) - pt * ls).sum() / student.numel()
    grad = (ls.exp() - pt).reshape(student.shape[0], student.shape[2], student.shape[3], C).permute(0, 3, 1, 2)
    return float(loss), grad


def check_fp64(student, teacher, tag):
    loss, grad = ops.kd_kl_loss(student, teacher)
    want_loss, want_grad = fp64(student, teacher)
    e_loss = abs(float(loss) - want_loss) / abs(want_loss) if want_loss != 0 else abs(float(loss))
    e_grad = float((grad.double() * student.numel() - want_grad).abs().max())
    print(f"kd_kl_loss {tag} {tuple(student.shape)}: loss {float(loss):.9e} (fp64 {want_loss:.9e}), relative error {e_loss:.3e}; "
          f"gradient x numel error {e_grad:.3e}")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    assert e_loss <= 1e-5, (tag, e_loss)
    assert e_grad <= 1e-5, (tag, e_grad)
    return loss, grad


@pytest.mark.parametrize("prefix", sorted(SHAPES))
def test_kd_kernel_against_fp64(maps, prefix):
    s, t = maps[prefix]
    assert tuple(s.shape) == SHAPES[prefix]
    loss, _ = check_fp64(s, t, prefix)
    assert float(loss) > 1e-3          # far from 0: the relative bound means something


@pytest.mark.parametrize("prefix", sorted(SHAPES))
def test_kd_identical_operands_give_exact_zeros(maps, prefix):
    s = maps[prefix][0]
    loss, grad = ops.kd_kl_loss(s, s.clone())
    assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0
    loss, grad = ops.kd_kl_loss(s, s)
    assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0


@pytest.mark.parametrize("prefix", ["c256_", "c64_", "c7_"])
def test_kd_is_bit_equal_across_launches_and_addresses(maps, prefix):
    s, t = maps[prefix]
    a_loss, a_grad = ops.kd_kl_loss(s, t)
    b_loss, b_grad = ops.kd_kl_loss(s, t)
    assert torch.equal(a_loss, b_loss) and torch.equal(a_grad, b_grad)

    def shifted(x, words):      # the same values `words` floats into a fresh allocation: 4-B aligned only
        buf = torch.empty(x.numel() + 64, dtype=torch.float32, device=DEV)
        view = buf[words:words + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == (buf.data_ptr() + 4 * words) % 16
        return view
    for ws, wt in ((1, 3), (2, 0)):
        c_loss, c_grad = ops.kd_kl_loss(shifted(s, ws), shifted(t, wt), grad_out=shifted(torch.zeros_like(s), 1))
        assert torch.equal(a_loss, c_loss) and torch.equal(a_grad, c_grad)


@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (1, 256, 9, 8), (2, 7, 5, 3)])
def test_kd_large_logits_and_constant_maps_stay_finite(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    big = lambda: ((torch.randint(0, 2, shape, generator=gen).float() * 2 - 1) * 1e4).to(DEV)      # noqa: E731
    s, t = big(), big()
    check_fp64(s, t, "+-1e4")
    check_fp64(torch.randn(shape, generator=gen).to(DEV) * 1e4, big(), "1e4 x normal")
    const = torch.full(shape, 3.25, device=DEV)
    loss, grad = check_fp64(const, const.clone() - 7.0, "constant")
    assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0      # both softmaxes are uniform
    check_fp64(const, t, "constant student")
    huge = torch.full(shape, 3.0e38, device=DEV)
    huge[:, 0] = -3.0e38
    loss, grad = ops.kd_kl_loss(huge, -huge)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("prefix", ["c256_", "c7_"])
def test_kd_without_gradient_only_reads(maps, prefix):
    s, t = maps[prefix]
    loss, _ = ops.kd_kl_loss(s, t)
    poison = torch.full_like(s, float("nan"))
    keep = poison.clone()
    ro_loss, ro_grad = ops.kd_kl_loss(s, t, need_grad=False, grad_out=poison)
    torch.cuda.synchronize()
    assert ro_grad is None and torch.equal(ro_loss, loss)
    assert torch.equal(poison.view(torch.int32), keep.view(torch.int32))
    with torch.no_grad():
        assert torch.equal(ops.KdKlLoss.apply(s, t), loss.reshape(()))


def test_kd_accepts_strided_inputs(maps):
    s, t = maps["c64_"]
    want_loss, want_grad = ops.kd_kl_loss(s, t)
    s_cl = s.contiguous(memory_format=torch.channels_last)
    wide = torch.zeros(t.shape[:3] + (t.shape[3] + 5,), device=DEV)
    wide[..., 2:2 + t.shape[3]] = t
    t_sl = wide[..., 2:2 + t.shape[3]]
    assert not s_cl.is_contiguous() and not t_sl.is_contiguous()
    assert ops.kd_kl_supported(s_cl, t_sl)
    loss, grad = ops.kd_kl_loss(s_cl, t_sl)
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    leaf = s_cl.clone().requires_grad_(True)
    ops.KdKlLoss.apply(leaf, t_sl).backward()
    assert torch.equal(leaf.grad, want_grad)


def test_kd_backward_scales_the_saved_gradient(maps):
    s, t = maps["c256_"]
    _, grad = ops.kd_kl_loss(s, t)
    leaf = s.clone().requires_grad_(True)
    loss = ops.KdKlLoss.apply(leaf, t)
    (10000 * loss).backward()
    assert torch.equal(leaf.grad, 10000 * grad)
    assert float(leaf.grad.abs().max()) > 0


def test_kd_supported_routes_other_inputs_to_torch(maps):
    s, t = maps["c7_"]
    assert ops.kd_kl_supported(s, t)
    assert not ops.kd_kl_supported(s.cpu(), t.cpu()) and not ops.kd_kl_supported(s.half(), t.half())
    assert not ops.kd_kl_supported(s, t[:, :5]) and not ops.kd_kl_supported(s[0], t[0])
    assert not ops.kd_kl_supported(s, t.clone().requires_grad_(True))
    with env("HEAL_KD_FUSED", "0"):
        assert not ops.kd_kl_supported(s, t)
    want, _ = fp64(s, t)
    assert abs(float(ops.kd_kl_torch(s, t)) - want) <= 1e-5 * want


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def test_kd_graph_replay_equals_eager(maps):
    s, t = maps["c256_"]
    other_s, other_t = t * 0.5 + 0.25, s.flip(1)
    want_loss, want_grad = ops.kd_kl_loss(other_s, other_t)
    static_s, static_t = s.clone().requires_grad_(True), t.clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2):                      # warm-up: the workspace of this stream is allocated outside the capture
            (3.0 * ops.KdKlLoss.apply(static_s, static_t)).backward()
        static_s.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            loss = ops.KdKlLoss.apply(static_s, static_t)
            (3.0 * loss).backward()
        with torch.no_grad():
            static_s.copy_(other_s)
            static_t.copy_(other_t)
        graph.replay()
        st.synchronize()
        assert torch.equal(loss.detach().reshape(1), want_loss) and torch.equal(static_s.grad, 3.0 * want_grad)
        with torch.no_grad():
            static_s.copy_(s)
            static_t.copy_(t)
        graph.replay()
        st.synchronize()
        first_loss, first_grad = ops.kd_kl_loss(s, t)
        assert torch.equal(loss.detach().reshape(1), first_loss) and torch.equal(static_s.grad, 3.0 * first_grad)


class _SmallStudent(torch.nn.Module):
    """1x1 convolutions from a fixed 8-channel input to a 64-channel `feature` and the three heads."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.body = torch.nn.Conv2d(8, 64, 1)
        self.cls_head, self.reg_head, self.dir_head = torch.nn.Conv2d(64, 2, 1), torch.nn.Conv2d(64, 14, 1), torch.nn.Conv2d(64, 4, 1)

    def forward(self, x):
        f = self.body(x) * 4.0
        return {"feature": f, "cls_preds": self.cls_head(f), "reg_preds": self.reg_head(f), "dir_preds": self.dir_head(f)}


def test_loss_module_is_the_same_with_the_kernel_on_and_off(g):
    from heal_amd.opencood.tools.train_utils import create_loss
    crit = create_loss(configs.lidar_disco_kd())
    o, tgt = loss_case(g, "c64_", DEV)
    x = torch.randn((1, 8, 13, 11), generator=torch.Generator().manual_seed(9)).to(DEV)
    results = {}
    for fused in ("1", "0"):
        model = _SmallStudent().to(DEV)
        with env("HEAL_KD_FUSED", fused):
            out = model(x)
            out["teacher_feature"] = o["teacher_feature"]
            calls = {}
            ops.TIMING = calls
            try:
                total = crit(out, tgt)
                total.backward()
                torch.cuda.synchronize()
            finally:
                ops.TIMING = None
        assert ("kd_kl_loss_c64" in calls) == (fused == "1")
        results[fused] = (float(total.detach()), dict(crit.loss_dict), {n: p.grad.clone() for n, p in model.named_parameters()})
    (ta, da, ga), (tb, db, gb) = results["1"], results["0"]
    print(f"loss module: fused {ta!r}, torch {tb!r}; kd {da['kd_loss']!r} vs {db['kd_loss']!r}")
    assert abs(ta - tb) <= 1e-5 * abs(tb) and abs(da["kd_loss"] - db["kd_loss"]) <= 1e-5 * abs(db["kd_loss"])
    for name, want in gb.items():
        e = float((ga[name] - want).abs().max()) / float(want.abs().max())
        assert e <= 1e-5, (name, e)
    assert float(gb["body.weight"].abs().max()) > 0


def test_one_training_step_then_inference(g):
    """train_w_kd.py:136-157 on the 32 x 32 scene: student (training mode) and frozen teacher forward, the teacher's outputs merged
    over the student's, loss, backward, Adam.  The merge replaces the student's dir_preds by the teacher's (the reference's
    behaviour), so the student's dir_head -- and nothing else -- is left without a gradient.  Afterwards the model runs inference
    (eval, no_grad) through heal_disco_fuse; the golden belongs to the fixture's weights, so those are loaded back for the
    comparison with it."""
    from heal_amd.opencood.tools import train_utils as tu
    hy = configs.lidar_disco_kd(M_RANGE)
    student, teacher = m_models(DEV)
    fixture_state = {k: v.clone() for k, v in student.state_dict().items()}
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher_before = {k: v.clone() for k, v in teacher.state_dict().items()}
    crit, optim = tu.create_loss(hy), tu.setup_optimizer(hy, student)
    data = m_data(g, DEV)
    gen = torch.Generator().manual_seed(3)
    pos = (torch.rand((1, 32, 32, 2), generator=gen) > 0.97).float()
    tgt = {"pos_equal_one": pos.to(DEV), "neg_equal_one": ((torch.rand((1, 32, 32, 2), generator=gen) > 0.2).float() * (1 - pos)).to(DEV),
           "targets": (torch.randn((1, 32, 32, 14), generator=gen) * 0.4).to(DEV)}
    student.train()
    student.zero_grad()
    calls = {}
    ops.TIMING = calls
    try:
        out = student(data)
        t_out = teacher(data)
        assert not t_out["teacher_feature"].requires_grad
        out.update(t_out)
        total = crit(out, tgt)
        total.backward()
        optim.step()
        torch.cuda.synchronize()
    finally:
        ops.TIMING = None
    assert "kd_kl_loss_c256" in calls and bool(torch.isfinite(total))
    assert crit.loss_dict["kd_loss"] > 0
    for name, p in student.named_parameters():
        if name.startswith("dir_head."):
            assert p.grad is None, name
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(student.fusion_net.pixel_weight_layer.conv1_1.weight.grad.abs().max()) > 0
    assert not torch.equal(student.cls_head.weight, fixture_state["cls_head.weight"])          # the step moved the weights
    assert all(p.grad is None for p in teacher.parameters())
    assert all(torch.equal(v, teacher_before[k]) for k, v in teacher.state_dict().items())
    student.eval()
    with torch.no_grad():
        calls = {}
        ops.TIMING = calls
        try:
            stepped = student(data)
            torch.cuda.synchronize()
        finally:
            ops.TIMING = None
        assert "disco_fuse_c256" in calls and all(bool(torch.isfinite(v).all()) for v in stepped.values())
        student.load_state_dict(fixture_state)
        calls = {}
        ops.TIMING = calls
        try:
            out = student(data)
            t_out = teacher(data)
            torch.cuda.synchronize()
        finally:
            ops.TIMING = None
        assert "disco_fuse_c256" in calls          # the kernel ran: no quiet torch path
    check_student(g, out)
    check_teacher(g, t_out)
    assert TOL == 1e-3
