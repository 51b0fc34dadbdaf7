"""Float64 restatement of ``cough_adamw_step`` (clip_grad_norm_ + torch.optim.AdamW over one flat buffer), the error
budget of its float32 kernels, a float32 transcription of the same formula, and the cases the optimizer tests share.

``ref_step`` is written from the formula in ``include/cough_amd.h`` and torch's single-tensor AdamW order::

    norm = sqrt(sum g^2);  coef = min(max_norm / (norm + 1e-6), 1);  g *= coef          (written back)
    p *= 1 - lr * wd;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)

The float scalars (lr, betas, eps, weight_decay, max_norm) are used as the ABI receives them -- rounded to float32, then
widened -- and ``bc1`` / ``bc2`` as given, in double.  A NaN norm gives a NaN coefficient (``torch.clamp`` keeps NaN).

Error budget (``bounds``)
-------------------------
u = 2^-24 is the largest relative error of one float32 operation (round to nearest; the build has no fast-math, so
sqrt and the divisions are correctly rounded too).  Every bound is the first-order propagation of one u per float32
operation of ``grad_norm_kernel`` / ``adamw_kernel``; the counts below were made from the kernels' source, before any
kernel output was looked at, and are not fitted to it.  FMA contraction only removes roundings from these counts.

* total_norm (relative ``r_n``).  A thread accumulates k = ceil(n / 1024) squares one after the other: one rounding
  for each square and one for each add, and the running sum of positive terms never exceeds the final one, so at most
  (k + 1) u on a thread's sum.  Then 6 cross-lane adds of the wave reduction and 16 serial adds over the waves: k + 23
  roundings on the sum of squares; the budget carries k + 26.  The square root halves the relative error and adds one
  rounding of its own: r_n = 0.5 (k + 26) u + u.
* g.  coef = max_norm / (norm + 1e-6f): one add, one division, and the product g * coef: r_g = r_n + 3 u + d6, with
  d6 = |float32(1e-6) - 1e-6| / (norm + 1e-6) for the constant that the kernel holds as a float.  Where even the
  smallest coefficient the kernel can arrive at, max_norm / (norm + 1e-6) * (1 - r_n - 2 u - d6), is >= 1, both sides
  clamp to exactly 1 and g is written back bit for bit: the bound is 0 there.
* Local roundings of m, v and p are charged TWICE their first-order worst case W.  The factor is fixed here, ahead of
  any measurement: it covers the second-order terms and an evaluation that associates differently, and it is what
  allows the host test to demand that a plain float32 evaluation in the kernel's order stays within HALF of every
  bound, i.e. within W itself plus half of what it inherits from the norm.
* m = m + (1 - beta1) (g - m), the lerp form.  1 - beta1, the difference and the product each put one u on a term of
  magnitude (1 - beta1) |g - m| <= 2 (1 - beta1) M, the final add one u on |m_new| <= M, with M = max(|m_old|, |g|):
  W_m = (6 (1 - beta1) + 1) u M, relative to M and not to |m_new| (the lerp may cancel).  Inherited: (1 - beta1) e_g.
* v = v beta2 + (1 - beta2) g g.  Five operations (v beta2, 1 - beta2, two products, the add) on non-negative terms
  none of which exceeds v_new: W_v = 5 u v_new.  Inherited: 2 (1 - beta2) |g| e_g, twice g's bound.
* update U = step_size * (m / (sqrt(v) / bc2_sqrt + eps)), step_size = float(lr / bc1), bc2_sqrt = float(sqrt(bc2)).
  Seven local roundings (sqrt, the cast of bc2_sqrt, the division by it, the add of eps, the quotient, the cast of
  step_size, the product): W_U = 7 u |U|.  Inherited: step_size (e_m / D + |m| / D * 0.5 e_v / sqrt(v) / bc2_sqrt / D)
  with D the denominator.
* p = p (1 - lr wd) - U.  lr * wd (one u on a term lr wd |p|), 1 - lr wd, the product and the final subtraction
  (one u each on at most P = max(|p_old|, |p_new|)): W_p = (3 + lr wd) u P, so k_p = 2 (3 + lr wd), plus the update's
  bound.

Underflow is outside the budget: the cases keep every square and every second moment a normal float32.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
NORM_THREADS = 1024                  # grad_norm_kernel's one workgroup
GRID_CAP_ELEMENTS = 4096 * 256       # adamw_kernel covers this many elements per pass of its grid-stride loop

Step = namedtuple("Step", "p g m v total_norm update")
Bounds = namedtuple("Bounds", "p g m v total_norm")


def f32(x: float) -> float:
    """The value a C float argument carries."""
    return float(np.float32(x))


def bias_corrections(beta1: float, beta2: float, t: int):
    """bc1, bc2 of step t from the betas as the ABI carries them (a self-consistent AdamW of those betas)."""
    return 1.0 - f32(beta1) ** t, 1.0 - f32(beta2) ** t


def ref_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, max_norm, bc1, bc2, total_norm=None) -> Step:
    """One step in float64.  ``total_norm`` replaces sqrt(sum g^2) where float32 arithmetic cannot hold it (finite
    gradients whose squares overflow: the kernel's norm, like torch's float32 one, is +inf there)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd, max_norm = (f32(s) for s in (lr, beta1, beta2, eps, weight_decay, max_norm))
    with np.errstate(invalid="ignore", over="ignore"):
        norm = float(np.sqrt(np.sum(g * g))) if total_norm is None else float(total_norm)
        ratio = max_norm / (norm + 1e-6)
        coef = 1.0 if ratio > 1.0 else ratio            # a NaN ratio stays NaN, as torch.clamp(max=1.0) leaves it
        g = g * coef
        p = p * (1.0 - lr * wd)
        m = m + (1.0 - beta1) * (g - m)
        v = v * beta2 + (1.0 - beta2) * g * g
        update = (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
        p = p - update
    return Step(p, g, m, v, norm, update)


def norm_rel_bound(n: int) -> float:
    return 0.5 * (-(-n // NORM_THREADS) + 26) * U + U


def bounds(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, max_norm, bc1, bc2, total_norm=None) -> Bounds:
    """Per-element absolute bounds of the float32 kernels' p, g, m, v against ``ref_step`` of the same arguments, and
    the absolute bound of total_norm.  See the module docstring for every count."""
    p0, g0, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    r = ref_step(p0, g0, m0, v0, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, max_norm=max_norm,
                 bc1=bc1, bc2=bc2, total_norm=total_norm)
    lr, beta1, beta2, eps, wd, max_norm = (f32(s) for s in (lr, beta1, beta2, eps, weight_decay, max_norm))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r_n = norm_rel_bound(g0.size)
        d6 = abs(f32(1e-6) - 1e-6) / (r.total_norm + 1e-6)
        r_c = r_n + 2 * U + d6
        ratio = max_norm / (r.total_norm + 1e-6)
        e_g = np.zeros_like(g0) if ratio * (1.0 - r_c) >= 1.0 else np.abs(r.g) * (r_c + U)
        M = np.maximum(np.abs(m0), np.abs(r.g))
        e_m = (1.0 - beta1) * e_g + 2 * (6 * (1.0 - beta1) + 1) * U * M
        e_v = 2 * (1.0 - beta2) * np.abs(r.g) * e_g + 2 * 5 * U * r.v
        s = np.sqrt(r.v) / np.sqrt(bc2)
        D = s + eps
        e_s = np.where(r.v > 0, 0.5 * e_v / np.where(r.v > 0, np.sqrt(r.v), 1.0) / np.sqrt(bc2), 0.0)
        step = lr / bc1
        e_u = step * (e_m / D + np.abs(r.m) / D * e_s / D) + 2 * 7 * U * np.abs(r.update)
        e_u = np.where(step == 0.0, 0.0, e_u)
        P = np.maximum(np.abs(p0), np.abs(r.p))
        e_p = 2 * (3 + lr * wd) * U * P + e_u
    return Bounds(e_p, e_g, e_m, e_v, r_n * r.total_norm)


# ------------------------------------------------------------------ float32 transcription, in the kernels' order
_LANE = np.arange(64)
_WAVE_PERMS = (_LANE ^ 1, _LANE ^ 2, (_LANE & ~7) | (7 - (_LANE & 7)), (_LANE & ~15) | (15 - (_LANE & 15)), _LANE ^ 16,
               _LANE ^ 32)           # wave_sum: two quad swaps, half-row mirror, row mirror, two cross-row swaps


def f32_norm(g32: np.ndarray) -> np.float32:
    """grad_norm_kernel in numpy float32: thread t sums g[t], g[t + 1024], ... in order, each wave folds its 64 sums
    with the six exchanges of ``wave_sum``, thread 0 adds the 16 wave sums in order."""
    g32 = np.asarray(g32, dtype=np.float32)
    k = -(-g32.size // NORM_THREADS)
    rows = np.zeros(k * NORM_THREADS, dtype=np.float32)
    rows[:g32.size] = g32
    rows = rows.reshape(k, NORM_THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(NORM_THREADS, dtype=np.float32)
        for row in rows:
            s = s + row * row
        w = s.reshape(NORM_THREADS // 64, 64)
        for perm in _WAVE_PERMS:
            w = w + w[:, perm]
        t = np.float32(0)
        for x in w[:, 0]:
            t = np.float32(t + x)
        return np.float32(np.sqrt(t))


def f32_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, max_norm, bc1, bc2) -> Step:
    """The header's formula evaluated in float32, one rounding per operation, in adamw_kernel's order."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd, max_norm = (F(s) for s in (lr, beta1, beta2, eps, weight_decay, max_norm))
    one = F(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = f32_norm(g)
        ratio = F(max_norm / F(norm + F(1e-6)))
        coef = one if ratio > one else ratio
        g = g * coef
        p = p * F(one - F(lr * wd))
        m = m + F(one - beta1) * (g - m)
        v = v * beta2 + F(one - beta2) * g * g
        step_size, bc2_sqrt = F(float(lr) / bc1), F(np.sqrt(bc2))
        update = step_size * (m / (np.sqrt(v) / bc2_sqrt + eps))
        p = p - update
    assert all(a.dtype == F for a in (p, g, m, v, update))
    return Step(p, g, m, v, norm, update)


# ------------------------------------------------------------------ cases
# (lr, beta1, beta2, eps, weight_decay)
HYPERS = {
    "defaults": (1e-3, 0.9, 0.999, 1e-8, 0.01),
    "other": (3e-4, 0.8, 0.99, 1e-7, 0.05),
    "betas0": (1e-3, 0.0, 0.0, 1e-8, 0.01),
    "wd0": (1e-3, 0.9, 0.999, 1e-8, 0.0),
    "lr0": (0.0, 0.9, 0.999, 1e-8, 0.01),
    "eps0": (1e-3, 0.9, 0.999, 0.0, 0.01),
}
STEPS = (1, 2, 1000, 100000)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 21122, 290370, 421954, GRID_CAP_ELEMENTS + 77,
         3 * GRID_CAP_ELEMENTS + 5)
N_GRID = 4099            # the hyperparameter / clip-regime grids: four passes of the norm loop plus a tail of 3
N_STRESS = 421954        # the Standard model's parameter count
WARMUP_CAP = 1500        # gradient steps behind a consistent state (see consistent_case)

Case = namedtuple("Case", "name p g m v kw t norm_override")


def hyper_kw(hyper, max_norm=1.0):
    lr, b1, b2, eps, wd = HYPERS[hyper] if isinstance(hyper, str) else hyper
    return dict(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, max_norm=max_norm)


def _grad(rng, base, scale):
    """A gradient with a persistent component (so that the first moment does not average out) plus noise."""
    return scale * (0.5 * base + rng.standard_normal(base.size))


@functools.lru_cache(maxsize=None)
def _state(n, hyper, t, max_norm, scale, seed):
    """(p, m, v, base) at the start of step t: ``ref_step`` from zero moments over the gradients of the last
    min(t - 1, WARMUP_CAP) steps.  For a larger t - 1 that is the state of a run whose earlier gradients were all zero
    (zero gradients keep zero moments), so the moments are what this optimizer reaches, never drawn at random."""
    rng = np.random.default_rng(seed)
    p = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4.0, 0.0, n)
    base = rng.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    kw = hyper_kw(hyper, max_norm)
    first = max(1, t - WARMUP_CAP)
    for k in range(first, t):
        bc1, bc2 = bias_corrections(kw["beta1"], kw["beta2"], k)
        r = ref_step(p, _grad(rng, base, scale), m, v, bc1=bc1, bc2=bc2, **kw)
        p, m, v = r.p, r.m, r.v
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32), base


def consistent_case(name, n, hyper, t, *, max_norm=1.0, scale=1.0, grad="noise", seed=0, norm_to=None) -> Case:
    """The float32 buffers of one call at step t.  ``grad``: "noise" (persistent component + noise, times ``scale``),
    "zero", "equal" (every element ``scale``), "spike" (noise, element n // 3 times 1e6), "decades" (magnitudes
    log-uniform over 8 decades, 1e-6 .. 1e2, times ``scale``).  ``norm_to`` rescales the gradient to that L2 norm."""
    hyper = hyper if isinstance(hyper, str) else tuple(hyper)
    p, m, v, base = _state(n, hyper, t, float(max_norm), float(scale), seed)
    rng = np.random.default_rng([seed, 1, t])
    if grad == "noise":
        g = _grad(rng, base, scale)
    elif grad == "zero":
        g = np.zeros(n)
    elif grad == "equal":
        g = np.full(n, float(scale))
    elif grad == "spike":
        g = _grad(rng, base, scale)
        g[n // 3] *= 1e6
    elif grad == "decades":
        g = scale * rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 2.0, n)
    else:
        raise ValueError(grad)
    if norm_to is not None:
        g = g * (norm_to / np.sqrt(np.sum(g * g)))
    g = g.astype(np.float32)
    if HYPERS.get(hyper, hyper)[3] == 0.0:
        assert np.all(g != 0)
    kw = hyper_kw(hyper, max_norm)
    kw["bc1"], kw["bc2"] = bias_corrections(kw["beta1"], kw["beta2"], t)
    return Case(name, p.copy(), g, m.copy(), v.copy(), kw, t, None)


def size_cases():
    return [(f"n{n}", dict(n=n, hyper="defaults", t=3, seed=n)) for n in SIZES]


def hyper_cases():
    return [(f"{h}-t{t}", dict(n=N_GRID, hyper=h, t=t, seed=7)) for h in HYPERS for t in STEPS]


def clip_cases():
    d = dict(n=N_GRID, hyper="defaults", t=5, seed=11)
    return [("below", dict(d, norm_to=0.5)),                       # coef exactly 1: g comes back bit for bit
            ("just-above", dict(d, norm_to=1.001)),
            ("1e4-above", dict(d, norm_to=1e4, scale=1e4 / 72.0)),  # the earlier steps saw gradients of that size too
            ("max-norm-1e9", dict(d, max_norm=1e9)),
            ("zero-grad", dict(d, grad="zero")),
            ("far-below", dict(d, norm_to=1e-5, scale=1e-5 / 72.0))]   # |g| ~ 1.5e-7: eps weighs in the denominator


def stress_cases():
    d = dict(n=N_STRESS, hyper="defaults", t=3, seed=13)
    return [("equal", dict(d, grad="equal", scale=0.37)), ("spike", dict(d, grad="spike")),
            ("decades", dict(d, grad="decades"))]


def finite_cases():
    return size_cases() + hyper_cases() + clip_cases() + stress_cases()


def build(spec) -> Case:
    name, kw = spec
    return consistent_case(name, **kw)


NONFINITE = ("nan", "+inf", "-inf", "overflow")


def nonfinite_case(kind) -> Case:
    """n = 1025 at step 4 of the defaults; one element (in the tail that only thread 0 of the norm sees twice) is NaN /
    +inf / -inf, or three finite elements are 1e30, whose squares overflow float32."""
    c = consistent_case(kind, 1025, "defaults", 4, seed=17)
    g = c.g.copy()
    override = None
    if kind == "nan":
        g[1024] = np.nan
    elif kind == "+inf":
        g[517] = np.inf
    elif kind == "-inf":
        g[3] = -np.inf
    elif kind == "overflow":
        g[[0, 600, 1024]] = (1e30, -1e30, 1e30)
        override = np.inf
    else:
        raise ValueError(kind)
    return c._replace(g=g, norm_override=override)


def torch_step(p, g, m, v, t, *, lr, beta1, beta2, eps, weight_decay, max_norm, dtype) -> Step:
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step() on the CPU in ``dtype``, as step t from the moments
    m, v.  The scalars go to torch as given; torch forms the bias corrections from its own betas and step count."""
    import torch
    tp = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
    tp.grad = torch.tensor(np.asarray(g), dtype=dtype)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay)
    opt.state[tp] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(np.asarray(m), dtype=dtype),
                     "exp_avg_sq": torch.tensor(np.asarray(v), dtype=dtype)}
    norm = torch.nn.utils.clip_grad_norm_([tp], max_norm=max_norm)
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == float(t)
    return Step(tp.detach().numpy(), tp.grad.numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), float(norm), None)


def abi_scalars(kw):
    """The hyperparameters of a case as the ABI carries them (float32-rounded), without the bias corrections."""
    return {k: f32(kw[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")}


# ------------------------------------------------------------------ optimizer-level runs (HipAdamW over many steps)
# one step of a run: the float32 buffers before it, what the optimizer left (a Step), the group's hyperparameters as the
# user set them (Python doubles) and the 1-based step number
Record = namedtuple("Record", "p g m v post kw t")

ODD_SHAPES = [(3,), (1,), (7, 5), (2, 3, 5, 7), (129,), (1, 1, 3), (1025,)]
RUN_STEPS, RUN_SWITCH = 40, 20
RUN_START = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0)
RUN_SWITCHED = dict(betas=(0.8, 0.99), weight_decay=0.05, max_norm=0.5)     # set after RUN_SWITCH steps


def run_gradient(k: int, n: int) -> np.ndarray:
    """The synthetic gradient written before step k (0-based): a persistent component plus noise, at a scale that puts
    the norm below the clip on some steps (0.2, 0.7) and above it on others (7, 700)."""
    base = np.random.default_rng(99).standard_normal(n)
    scale = (3e-4, 1e-3, 1e-2, 1.0)[k % 4]
    return _grad(np.random.default_rng([99, k]), base, scale).astype(np.float32)


def run_initial_params(n: int) -> np.ndarray:
    return (0.05 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)


def record_case(rec: Record) -> Case:
    """The step of a record as a self-consistent AdamW: bias corrections from the betas as the ABI carries them."""
    kw = dict(rec.kw)
    kw["bc1"], kw["bc2"] = bias_corrections(kw["beta1"], kw["beta2"], rec.t)
    return Case(f"step{rec.t}", rec.p, rec.g, rec.m, rec.v, kw, rec.t, None)


def beta_cast_fraction(rec: Record, got_p=None) -> float:
    """max |p - p_torch| / bound against torch.optim.AdamW in float64 with the user's DOUBLE betas (every other scalar
    as the ABI carries it), one step from the record's state.  The bound is the float32 budget of p plus
    (|float32(beta1) - beta1| / (1 - beta1) + |float32(beta2) - beta2| / (1 - beta2)) |update|, the cost of carrying
    the betas as floats."""
    import torch
    c = record_case(rec)
    sc = abi_scalars(c.kw)
    b1, b2 = rec.kw["beta1"], rec.kw["beta2"]
    ts = torch_step(rec.p, rec.g, rec.m, rec.v, rec.t, dtype=torch.float64, **dict(sc, beta1=b1, beta2=b2))
    ref = ref_step(c.p, c.g, c.m, c.v, **c.kw)
    bnd = bounds(c.p, c.g, c.m, c.v, **c.kw)
    cost = (abs(f32(b1) - b1) / (1.0 - b1) + abs(f32(b2) - b2) / (1.0 - b2)) * np.abs(ref.update)
    got = rec.post.p if got_p is None else got_p
    err = np.abs(np.asarray(got, dtype=np.float64) - ts.p)
    return float(np.max(np.where(err == 0, 0.0, err / (bnd.p + cost))))


def worst_fractions(got: Step, case: Case):
    """{quantity: max over the elements of |got - ref| / bound} (0 / 0 counts as 0; an error over a zero bound as inf)."""
    ref = ref_step(case.p, case.g, case.m, case.v, total_norm=case.norm_override, **case.kw)
    bnd = bounds(case.p, case.g, case.m, case.v, total_norm=case.norm_override, **case.kw)
    out = {}
    for q in ("p", "g", "m", "v", "total_norm"):
        err = np.abs(np.asarray(getattr(got, q), dtype=np.float64) - getattr(ref, q))
        b = np.asarray(getattr(bnd, q), dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(err == 0, 0.0, err / b)
        out[q] = float(np.max(frac))
    return out
