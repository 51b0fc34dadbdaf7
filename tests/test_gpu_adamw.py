"""``cough_adamw_step`` (``grad_norm_kernel`` + ``adamw_kernel``) on its own, element by element, against the float64
restatement ``adamw_ref.ref_step`` under the float32 error budget ``adamw_ref.bounds``; then ``HipAdamW`` over 40 steps
with a scheduler and hyperparameters that change on the way.  No forward or backward pass is involved: the gradients
are synthetic, so nothing here depends on a pooling tie or a ReLU kink.

Every test prints its worst error as a fraction of its bound (``ADAMW_FRACTION <case> <quantity> <fraction>``);
``profiles/adamw_precision.txt`` is made from those lines."""
import copy

import numpy as np
import pytest
import torch

import adamw_ref as R
import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.training import HipAdamW

pytestmark = pytest.mark.gpu

GUARD = 256                   # floats on either side of every buffer
PATTERN = 0x7FA5A5A5          # a NaN bit pattern: a stray read would poison what it feeds, a stray write changes it


class Guarded:
    """n float32 on the device between two guard zones, placed so that the data is 4-byte aligned and no more."""

    def __init__(self, host: np.ndarray):
        n = host.size
        self.n = n
        self.raw = torch.full((1 + GUARD + n + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        self.data = self.raw[1 + GUARD:1 + GUARD + n].view(torch.float32)
        self.data.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))
        assert self.raw.data_ptr() % 256 == 0 and self.ptr % 8 == 4

    @property
    def ptr(self) -> int:
        return self.data.data_ptr()

    def host(self) -> np.ndarray:
        return self.data.cpu().numpy()

    def guards_intact(self) -> bool:
        lo, hi = self.raw[:1 + GUARD], self.raw[1 + GUARD + self.n:]
        return hi.numel() == GUARD and bool((lo == PATTERN).all()) and bool((hi == PATTERN).all())


def run_kernel(c: R.Case, stream=None) -> R.Step:
    """One ``cough_adamw_step`` on guarded copies of the case's buffers."""
    bufs = [Guarded(a) for a in (c.p, c.g, c.m, c.v)]
    norm = Guarded(np.full(1, -1.0, np.float32))
    kw = c.kw
    torch.cuda.synchronize()
    rc = _lib.load().cough_adamw_step(
        bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, c.p.size, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"],
        kw["weight_decay"], kw["max_norm"], kw["bc1"], kw["bc2"], norm.ptr, None if stream is None else stream.cuda_stream)
    _lib.check(rc, "cough_adamw_step")
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in bufs + [norm]), "a guard zone was written"
    p, g, m, v = (b.host() for b in bufs)
    return R.Step(p, g, m, v, norm.host()[0], None)


def report(case: str, frac: dict):
    for q, x in frac.items():
        print(f"ADAMW_FRACTION {case} {q} {x:.4f}")


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("spec", R.finite_cases(), ids=lambda s: s[0])
def test_every_element_within_the_float32_budget(spec):
    """Sizes (1 .. 3 * 4096 * 256 + 5: the last two take more than one pass of the grid-stride loop), hyperparameters x
    steps, clip regimes and norm stress: p, g, m, v and total_norm against the restatement, every element."""
    c = R.build(spec)
    got = run_kernel(c)
    frac = R.worst_fractions(got, c)
    report(spec[0], frac)
    assert all(np.all(np.isfinite(a)) for a in (got.p, got.g, got.m, got.v))
    assert all(x <= 1.0 for x in frac.values()), frac
    name = spec[0]
    if name in ("below", "max-norm-1e9", "far-below"):        # coef is exactly 1
        assert np.array_equal(bits(got.g), bits(c.g))
    if name.startswith("lr0"):
        assert np.array_equal(bits(got.p), bits(c.p))
        # the moments still move (an element whose v happens to round back onto itself is possible, hence not `all`)
        assert np.mean(got.m != c.m) > 0.99 and np.mean(got.v != c.v) > 0.99
    if name == "zero-grad":
        assert got.total_norm == 0 and not np.any(got.g)
        assert np.all(np.abs(got.m) <= np.abs(c.m)) and np.all(got.v <= c.v) and np.any(got.v < c.v)


def test_zero_gradient_on_zero_moments_only_decays_the_parameters():
    c = R.consistent_case("zero-state", R.N_GRID, "defaults", 1, grad="zero", seed=11)
    assert not np.any(c.m) and not np.any(c.v)
    got = run_kernel(c)
    frac = R.worst_fractions(got, c)
    report("zero-grad-zero-state", frac)
    assert all(x <= 1.0 for x in frac.values()), frac
    assert not np.any(got.m) and not np.any(got.v) and not np.any(got.g) and got.total_norm == 0
    assert np.all(np.isfinite(got.p)) and np.all(np.abs(got.p) <= np.abs(c.p)) and np.all(np.sign(got.p) == np.sign(c.p))


@pytest.mark.parametrize("kind", R.NONFINITE)
def test_nonfinite_gradients_as_torch_float32(kind):
    """One NaN / +inf / -inf element, or finite gradients whose squares overflow, at n = 1025: the NaN positions are
    those of torch's float32 clip_grad_norm_ + AdamW on the CPU (pinned in test_adamw_ref_host.py), the finite values
    are within the budget.  A NaN norm must give a NaN coefficient: every element NaN."""
    c = R.nonfinite_case(kind)
    want = R.torch_step(c.p, c.g, c.m, c.v, c.t, dtype=torch.float32, **R.abi_scalars(c.kw))
    got = run_kernel(c)
    ref = R.ref_step(c.p, c.g, c.m, c.v, total_norm=c.norm_override, **c.kw)
    bnd = R.bounds(c.p, c.g, c.m, c.v, total_norm=c.norm_override, **c.kw)
    for q in ("p", "g", "m", "v"):
        g_, w_, r_ = getattr(got, q), getattr(want, q), getattr(ref, q)
        print(f"ADAMW_NONFINITE {kind} {q}: NaN in {int(np.isnan(g_).sum())} elements, torch {int(np.isnan(w_).sum())}")
        assert np.array_equal(np.isnan(g_), np.isnan(w_)), f"{q}: NaN positions differ from torch's"
        assert not np.any(np.isinf(g_))
        ok = ~np.isnan(w_)
        err = np.abs(g_[ok].astype(np.float64) - r_[ok])
        assert np.all(err <= getattr(bnd, q)[ok]), q
    assert np.isnan(got.total_norm) if kind == "nan" else got.total_norm == np.inf
    assert np.isnan(want.total_norm) if kind == "nan" else want.total_norm == np.inf


@pytest.mark.parametrize("n", [R.N_STRESS, R.GRID_CAP_ELEMENTS + 77])
def test_repeated_calls_and_another_stream_give_the_same_bits(n):
    c = R.consistent_case("det", n, "defaults", 3, seed=n)
    a = run_kernel(c)
    b = run_kernel(c)
    s = torch.cuda.Stream()
    d = run_kernel(c, stream=s)
    for other in (b, d):
        for q in ("p", "g", "m", "v"):
            assert np.array_equal(bits(getattr(a, q)), bits(getattr(other, q))), q
        assert bits(np.float32(a.total_norm)) == bits(np.float32(other.total_norm))


# ------------------------------------------------------------------ HipAdamW over 40 steps
def _shapes():
    return R.ODD_SHAPES + [tuple(p.shape) for p in cda.create_model("standard", n_mels=90).parameters()]


def _optimizer(flat: torch.Tensor, grads: torch.Tensor, **kw):
    params, off = [], 0
    for s in _shapes():
        k = int(np.prod(s))
        params.append(torch.nn.Parameter(flat[off:off + k].view(s)))
        off += k
    assert off == flat.numel()
    return HipAdamW(params, flat, grads, **kw)


def _scheduler(opt):
    return torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=7, T_mult=2, eta_min=1e-6)


def _drive(opt, sched, grads, k_from, k_to):
    """Steps k_from .. k_to - 1 (0-based) of the run; one Record per step."""
    records = []
    n = grads.numel()
    for k in range(k_from, k_to):
        if k == R.RUN_SWITCH:
            opt.param_groups[0]["betas"] = R.RUN_SWITCHED["betas"]
            opt.param_groups[0]["weight_decay"] = R.RUN_SWITCHED["weight_decay"]
            opt.max_norm = R.RUN_SWITCHED["max_norm"]
        grads.copy_(torch.from_numpy(R.run_gradient(k, n)))
        g = opt.param_groups[0]
        kw = dict(lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]),
                  weight_decay=float(g["weight_decay"]), max_norm=float(opt.max_norm))
        pre = [t.detach().cpu().numpy().copy() for t in (opt._flat, grads, opt._exp_avg, opt._exp_avg_sq)]
        opt.step()
        torch.cuda.synchronize()
        post = R.Step(*[t.detach().cpu().numpy().copy() for t in (opt._flat, grads, opt._exp_avg, opt._exp_avg_sq)],
                      float(opt.total_norm.item()), None)
        records.append(R.Record(*pre, post, kw, k + 1))
        sched.step()
    return records


def _fresh(n):
    flat = torch.from_numpy(R.run_initial_params(n)).cuda()
    grads = torch.zeros(n, device="cuda")
    start = dict(R.RUN_START)
    opt = _optimizer(flat, grads, lr=start["lr"], betas=start["betas"], eps=start["eps"],
                     weight_decay=start["weight_decay"], max_norm=start["max_norm"])
    return opt, _scheduler(opt), flat, grads


@pytest.fixture(scope="module")
def run40():
    """The uninterrupted run, and the optimizer / scheduler state after RUN_SWITCH steps of a second, identical run."""
    n = sum(int(np.prod(s)) for s in _shapes())
    assert n == _lib.TRAIN_STD_NUM_PARAMS + sum(int(np.prod(s)) for s in R.ODD_SHAPES)
    opt, sched, _, grads = _fresh(n)
    records = _drive(opt, sched, grads, 0, R.RUN_STEPS)
    opt2, sched2, flat2, grads2 = _fresh(n)
    head = _drive(opt2, sched2, grads2, 0, R.RUN_SWITCH)
    saved = dict(opt=copy.deepcopy(opt2.state_dict()), sched=copy.deepcopy(sched2.state_dict()),
                 flat=flat2.detach().clone(), max_norm=opt2.max_norm)
    return dict(n=n, records=records, head=head, saved=saved)


def test_run_uses_what_it_claims(run40):
    recs = run40["records"]
    assert len(recs) == R.RUN_STEPS and [r.t for r in recs] == list(range(1, R.RUN_STEPS + 1))
    lrs = [r.kw["lr"] for r in recs]
    assert all(abs(lrs[k] - 1e-3) < 1e-12 for k in (0, 7, 21)) and min(lrs) < 1e-4 and len(set(lrs)) > 20   # restarts
    assert recs[R.RUN_SWITCH - 1].kw["beta1"] == 0.9 and recs[R.RUN_SWITCH].kw["beta1"] == 0.8
    assert recs[R.RUN_SWITCH].kw["weight_decay"] == 0.05 and recs[R.RUN_SWITCH].kw["max_norm"] == 0.5
    clipped = [r.post.total_norm > r.kw["max_norm"] for r in recs]
    assert any(clipped) and not all(clipped)


def test_each_step_is_the_adamw_of_the_betas_the_kernel_holds(run40):
    """Every step against the restatement started from the optimizer's own state, bias corrections from the
    float32-rounded betas (a self-consistent AdamW), under the float32 budget; total_norm holds the pre-clip norm.
    This is the test that sees bias corrections formed from the Python (double) betas while the kernel forms 1 - beta
    from the float ones: on an MI355X p was then at 2.13 times its bound at step 1 and 4.47 times at step 5; with
    ``HipAdamW.step`` forming them from the float-rounded betas it is at most 0.24."""
    worst, at = {}, {}
    for rec in run40["records"]:
        c = R.record_case(rec)
        for q, x in R.worst_fractions(rec.post, c).items():
            if x >= worst.get(q, 0.0):
                worst[q], at[q] = x, rec.t
        pre_clip = float(np.sqrt(np.sum(rec.g.astype(np.float64) ** 2)))
        assert abs(rec.post.total_norm - pre_clip) <= R.norm_rel_bound(rec.g.size) * pre_clip, rec.t
    report("hipadamw-40-steps", worst)
    assert all(x <= 1.0 for x in worst.values()), (worst, at)


def test_each_step_against_torch_adamw_with_the_double_betas(run40):
    worst = 0.0
    for rec in run40["records"]:
        x = R.beta_cast_fraction(rec)
        worst = max(worst, x)
        assert x <= 1.0, (rec.t, x)
    report("hipadamw-vs-torch-double-betas", {"p": worst})


def test_resume_is_bit_identical_and_the_state_hands_off_to_torch(run40):
    n, saved, recs = run40["n"], run40["saved"], run40["records"]
    for a, b in zip(run40["head"], recs):                   # two runs from the same start are the same run
        assert np.array_equal(bits(a.post.p), bits(b.post.p))
    flat = saved["flat"].clone()
    grads = torch.zeros(n, device="cuda")
    opt = _optimizer(flat, grads)                          # constructor defaults: everything comes from the state
    sched = _scheduler(opt)                                # (a new scheduler sets lr, so the states are loaded after it)
    opt.load_state_dict(copy.deepcopy(saved["opt"]))
    opt.max_norm = saved["max_norm"]
    sched.load_state_dict(copy.deepcopy(saved["sched"]))
    tail = _drive(opt, sched, grads, R.RUN_SWITCH, R.RUN_STEPS)
    for a, b in zip(tail, recs[R.RUN_SWITCH:]):
        assert a.kw == b.kw and a.t == b.t
        for q in ("p", "g", "m", "v"):
            assert np.array_equal(bits(getattr(a.post, q)), bits(getattr(b.post, q))), (a.t, q)
        assert a.post.total_norm == b.post.total_norm

    # the same state in torch.optim.AdamW over float64 copies: its first step against ours
    rec = recs[R.RUN_SWITCH]
    shapes = _shapes()
    tparams, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        tparams.append(torch.nn.Parameter(torch.from_numpy(rec.p[off:off + k].astype(np.float64)).view(s)))
        off += k
    topt = torch.optim.AdamW(tparams, lr=1.0)
    sd = copy.deepcopy(saved["opt"])
    for st in sd["state"].values():
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu()
    topt.load_state_dict(sd)
    tg = topt.param_groups[0]
    assert float(topt.state[tparams[0]]["step"]) == R.RUN_SWITCH and topt.state[tparams[3]]["exp_avg"].dtype == torch.float64
    # the switch of step RUN_SWITCH, and every scalar but the betas as the ABI carries it
    tg["betas"] = R.RUN_SWITCHED["betas"]
    tg["weight_decay"] = R.f32(R.RUN_SWITCHED["weight_decay"])
    assert tg["lr"] == rec.kw["lr"]
    tg["lr"], tg["eps"] = R.f32(tg["lr"]), R.f32(tg["eps"])
    off = 0
    for p in tparams:
        p.grad = torch.from_numpy(rec.g[off:off + p.numel()].astype(np.float64)).view(p.shape)
        off += p.numel()
    torch.nn.utils.clip_grad_norm_(tparams, max_norm=R.f32(R.RUN_SWITCHED["max_norm"]))
    topt.step()
    tp = np.concatenate([p.detach().numpy().reshape(-1) for p in tparams])
    one_tensor = R.torch_step(rec.p, rec.g, rec.m, rec.v, rec.t, dtype=torch.float64,
                              **dict(R.abi_scalars(rec.kw), beta1=rec.kw["beta1"], beta2=rec.kw["beta2"]))
    assert np.max(np.abs(tp - one_tensor.p)) <= 1e-12     # 27 tensors or one flat tensor: the same torch step
    x = R.beta_cast_fraction(rec, got_p=tail[0].post.p)
    report("handoff-to-torch", {"p": x})
    assert x <= 1.0, x
