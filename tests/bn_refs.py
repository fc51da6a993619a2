"""Float64 numpy references, fixtures and per-element bounds of the BatchNorm training kernels (include/heal_amd_train_bn.h:
heal_bn_stats, heal_bn_act_forward, heal_bn_act_backward) -- numpy only, so that tests/test_bn_refs_cpu.py can prove every reference
against float64 torch autograd on a machine without a GPU.  tests/test_gpu_bn_train.py compares the kernels with them.

Conventions of tests/backward_refs.py: next to each value the reference returns T, the sum of the ABSOLUTE values of the terms of
that element, and a test asserts |got - ref| <= k * 2^-24 * T + tiny element by element.  EPS = 2^-24 is half an ulp: one fp32
rounding is a relative error of at most EPS.  k counts the roundings of the kernel's operation sequence (the library is built with
-ffp-contract=off, every fp32 operation is rounded on its own); each k is derived in the docstring of the reference that uses it, none
was tuned on a kernel's output.  The kernels take mean / rstd / y as INPUTS (fp32 values); the references take the same fp32 values,
so those carry no error of their own.

`defect=`: the six seeded mistakes that tests/test_bn_refs_cpu.py shows each bound to catch."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
TINY = 1e-30

K_FORWARD = 6
K_DX_BATCH = 10
K_DX_FROZEN = 2
K_DGAMMA = 3
K_DBETA = 2
K_RUNNING = 2
STAT_ULPS = 2.0

DEFECTS = ("mask_ge", "running_var_biased", "no_dgamma_term", "no_dbeta_term", "eps_outside_sqrt", "momentum_swapped")


def max_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the elements: <= 1 means the bound holds.  A non-finite value counts as infinite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        raise ValueError(f"shapes differ: {got.shape} and {ref.shape}")
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    return float((err / (np.asarray(bound, np.float64) + TINY)).max()) if err.size else 0.0


def ulps(got, ref):
    """Largest |got - ref| in units of the fp32 spacing at |ref| (ref: the float64 value the fp32 result is a single rounding of)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / np.spacing(np.abs(ref).astype(F32)).astype(np.float64)).max())


def _per_channel(v):
    return np.asarray(v, np.float64)[None, :, None, None]


# ------------------------------------------------------------------------------------------------------------------ statistics
def stats_ref(x, eps, momentum=0.0, running_mean=None, running_var=None, defect=None):
    """heal_bn_stats in float64: x [n, C, H, W] -> dict(mean, var (biased), rstd = 1 / sqrt(var + eps), and with running buffers
    running_mean / running_var after the update r <- (1 - momentum) r + momentum stat (the unbiased variance var M / (M - 1)), with
    T_running_* = |(1 - momentum) r| + |momentum stat|).

    Bounds.  mean and rstd are single roundings of fp64 results whose own error (fp64 sums of at most 2^30 shifted terms) is far
    below an fp32 ulp: they must lie within STAT_ULPS = 2 ulp of the reference (1/2 ulp for the rounding; the rest covers the
    kernel's fp64 sqrt / division and summation order).  The running buffers are formed in fp64 and rounded once: EPS |value| <=
    EPS T; K_RUNNING = 2 leaves one more EPS T for the fp64 summation order, which moves the statistic by at most M 2^-53 of its
    size (below 2^-24 for every supported M)."""
    x = np.asarray(x, np.float64)
    n, C, H, W = x.shape
    M = n * H * W
    mean = x.mean((0, 2, 3))
    var = ((x - _per_channel(mean)) ** 2).mean((0, 2, 3))
    rstd = 1.0 / (np.sqrt(var) + eps) if defect == "eps_outside_sqrt" else 1.0 / np.sqrt(var + eps)
    out = {"mean": mean, "var": var, "rstd": rstd}
    if running_mean is not None:
        rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
        stat_var = var if defect == "running_var_biased" else var * (M / (M - 1.0))
        keep, take = (momentum, 1.0 - momentum) if defect == "momentum_swapped" else (1.0 - momentum, momentum)
        out["running_mean"] = keep * rm + take * mean
        out["running_var"] = keep * rv + take * stat_var
        out["T_running_mean"] = np.abs((1.0 - momentum) * rm) + np.abs(momentum * mean)
        out["T_running_var"] = np.abs((1.0 - momentum) * rv) + np.abs(momentum * var * (M / (M - 1.0)))
    return out


def stats_naive_f32(x):
    """The textbook one-pass statistics in fp32, E[x^2] - mean^2 (sequential fp32 sums): what the shifted fp64 sums replace."""
    x = np.asarray(x, F32)
    n, C, H, W = x.shape
    rows = np.moveaxis(x, 1, 0).reshape(C, -1)
    s1 = np.zeros(C, F32)
    s2 = np.zeros(C, F32)
    for i in range(rows.shape[1]):
        s1 = (s1 + rows[:, i]).astype(F32)
        s2 = (s2 + (rows[:, i] * rows[:, i]).astype(F32)).astype(F32)
    M = F32(rows.shape[1])
    mean = (s1 / M).astype(F32)
    var = ((s2 / M).astype(F32) - (mean * mean).astype(F32)).astype(F32)
    return mean, var


# --------------------------------------------------------------------------------------------------------------------- forward
def forward_ref(x, residual, mean, rstd, gamma, beta, relu):
    """heal_bn_act_forward in float64 -> (y, z, T): z = (x - mean) rstd gamma + beta (+ residual), y = relu ? max(z, 0) : z,
    T = |xh gamma| + |beta| (+ |residual|) with xh = (x - mean) rstd.

    K_FORWARD.  xh = fl(fl(x - mean) * rstd): 2 roundings; * gamma: 1 -> 3 EPS |xh gamma|; + beta: 1 EPS (|xh gamma| + |beta|);
    + residual: 1 EPS T; max(., 0) does not increase an error.  5 EPS T to first order; K_FORWARD = 6 leaves one for the
    second-order terms."""
    x = np.asarray(x, np.float64)
    xh = (x - _per_channel(mean)) * _per_channel(rstd)
    t = xh * _per_channel(gamma)
    z = t + _per_channel(beta)
    T = np.abs(t) + np.abs(_per_channel(beta))
    if residual is not None:
        z = z + np.asarray(residual, np.float64)
        T = T + np.abs(np.asarray(residual, np.float64))
    return (np.maximum(z, 0.0) if relu else z), z, T


# -------------------------------------------------------------------------------------------------------------------- backward
def backward_ref(dy, x, y, mean, rstd, gamma, relu, batch_stats, defect=None):
    """heal_bn_act_backward in float64, closed form -> dict(dx, dresidual, dgamma, dbeta, T_dx, T_dgamma, T_dbeta, k_dx).
    dz = relu ? dy [y > 0] : dy (y: the forward's fp32 result, the mask torch's ReLU backward uses); xh = (x - mean) rstd;
    dbeta = sum dz; dgamma = sum dz xh; with batch statistics dx = gamma rstd (dz - dbeta / M - xh dgamma / M), frozen
    dx = gamma rstd dz; dresidual = dz (exact: the test compares it bit for bit).

    K_DBETA.  fp64 sum of fp32 values rounded once: EPS |dbeta| <= EPS T_dbeta, T_dbeta = sum |dz|; 2 leaves one for the fp64
    summation order.
    K_DGAMMA.  xh carries 2 roundings, the product and the sum are fp64: 2 EPS T_dgamma, T_dgamma = sum |dz xh|; + 1 for the
    final rounding = 3.
    K_DX_BATCH, with A = sum |dz| / M and B = sum |dz xh| / M, T_dx = |gamma rstd| (|dz| + A + |xh| B):
      m1 = fl32(dbeta / M): 1 EPS A;  t1 = fl(dz - m1): + 1 EPS (|dz| + A)  -> 2 EPS (|dz| + A);
      m2 = fl32(dgamma / M): 2 EPS B from xh + 1 for the rounding = 3 EPS B;  xh: 2 EPS |xh|;
      t2 = fl(xh * m2): (2 + 3 + 1) EPS |xh| B = 6;  t3 = fl(t1 - t2): + 1 EPS (|t1| + |t2|) -> 3 EPS (|dz| + A) + 7 EPS |xh| B;
      a = fl(gamma * rstd): 1;  fl(a * t3): 1  ->  at most 9 EPS T_dx to first order; 10 leaves one for the second-order terms.
    K_DX_FROZEN.  fl(fl(gamma * rstd) * dz): 2 roundings, T_dx = |gamma rstd dz|."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    n, C, H, W = x.shape
    M = n * H * W
    if relu:
        yy = np.asarray(y, np.float64)
        dz = dy * ((yy >= 0.0) if defect == "mask_ge" else (yy > 0.0))
    else:
        dz = dy
    xh = (x - _per_channel(mean)) * _per_channel(rstd)
    dbeta = dz.sum((0, 2, 3))
    dgamma = (dz * xh).sum((0, 2, 3))
    A = np.abs(dz).sum((0, 2, 3)) / M
    B = np.abs(dz * xh).sum((0, 2, 3)) / M
    a = _per_channel(np.asarray(gamma, np.float64) * np.asarray(rstd, np.float64))
    if batch_stats:
        m1 = 0.0 if defect == "no_dbeta_term" else _per_channel(dbeta / M)
        m2 = 0.0 if defect == "no_dgamma_term" else _per_channel(dgamma / M)
        dx = a * (dz - m1 - xh * m2)
        T_dx = np.abs(a) * (np.abs(dz) + _per_channel(A) + np.abs(xh) * _per_channel(B))
    else:
        dx = a * dz
        T_dx = np.abs(a * dz)
    return {"dx": dx, "dresidual": dz, "dgamma": dgamma, "dbeta": dbeta, "T_dx": T_dx, "T_dgamma": B * M, "T_dbeta": A * M,
            "k_dx": K_DX_BATCH if batch_stats else K_DX_FROZEN}


# -------------------------------------------------------------------------------------------------------------------- fixtures
def fixture(shape, seed, residual=True, kind="random"):
    """fp32 inputs of one case: dict(x, residual | None, dy, gamma, beta, running_mean, running_var, eps, momentum).
    kind "random": per-channel offsets and scales around N(0, 1) data; gamma of either sign; beta and the residual small enough that
    the outputs fall on both sides of zero (tests/test_bn_refs_cpu.py asserts at least 10 % on each).
    kind "cancellation": channel means of 1000 with a standard deviation of 0.01 (E[x^2] - mean^2 in fp32 loses every digit)."""
    n, C, H, W = shape
    rng = np.random.default_rng(seed)
    if kind == "cancellation":
        x = 1000.0 + 0.01 * rng.standard_normal(shape)
        eps = 1e-5
    else:
        x = rng.standard_normal(shape) * rng.uniform(0.5, 3.0, (1, C, 1, 1)) + rng.uniform(-2.0, 2.0, (1, C, 1, 1))
        eps = 1e-3
    sign = np.where(rng.random(C) < 0.3, -1.0, 1.0)
    out = {
        "x": x.astype(F32),
        "residual": (0.3 * rng.standard_normal(shape)).astype(F32) if residual else None,
        "dy": rng.standard_normal(shape).astype(F32),
        "gamma": (sign * rng.uniform(0.5, 1.5, C)).astype(F32),
        "beta": (0.2 * rng.standard_normal(C)).astype(F32),
        "running_mean": (0.5 * rng.standard_normal(C)).astype(F32),
        "running_var": rng.uniform(0.5, 2.0, C).astype(F32),
        "eps": eps,
        "momentum": 0.1 if seed % 2 else 0.01,
    }
    return out


# name -> (shape, seed): the random fixtures of the suite (HEAL_BN_SEGMENT = 4096: 4097 spans two segments with a one-element tail)
RANDOM_FIXTURES = {
    "two": ((1, 1, 1, 2), 3),
    "odd": ((2, 3, 3, 5), 11),
    "wide": ((3, 65, 7, 9), 12),
    "pixel": ((2, 8, 1, 1), 13),
    "plane": ((1, 4, 64, 64), 14),
    "tail": ((2, 2, 1, 4097), 15),
    "multi": ((2, 3, 96, 96), 16),
}
CANCELLATION = ((2, 3, 24, 20), 21)
