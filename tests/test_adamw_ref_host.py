"""The optimizer tests' reference side, checked on the CPU: ``adamw_ref.ref_step`` against torch itself, the error
budget ``adamw_ref.bounds`` against a plain float32 evaluation, and torch's own float32 answer to non-finite gradients
(what ``tests/test_gpu_adamw.py`` holds ``cough_adamw_step`` to)."""
import numpy as np
import pytest
import torch

import adamw_ref as R


def _close(got, want, scale, what, rel=1e-12):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    worst = float(np.max(err / np.maximum(scale, 1e-300)))
    assert worst <= rel, f"{what}: {worst:.3e} relative"


@pytest.mark.parametrize("hyper", list(R.HYPERS))
@pytest.mark.parametrize("t", R.STEPS)
def test_ref_step_is_clip_grad_norm_plus_torch_adamw_in_float64(hyper, t):
    """Four consecutive steps from the consistent state of step t: both sides run on from their own results.  torch gets
    the same float32-rounded scalars and forms the bias corrections itself.  1e-12 relative -- of max(|m_old|, |g|)
    for the first moment, whose lerp torch evaluates in another form."""
    c = R.consistent_case("c", R.N_GRID, hyper, t, seed=7)
    sc = R.abi_scalars(c.kw)
    rng = np.random.default_rng(t)
    rp, rm, rv = (a.astype(np.float64) for a in (c.p, c.m, c.v))
    tp, tm, tv = rp, rm, rv
    g = c.g.astype(np.float64)
    for k in range(t, t + 4):
        bc1, bc2 = R.bias_corrections(c.kw["beta1"], c.kw["beta2"], k)
        r = R.ref_step(rp, g, rm, rv, bc1=bc1, bc2=bc2, **sc)
        ts = R.torch_step(tp, g, tm, tv, k, dtype=torch.float64, **sc)
        _close(ts.total_norm, r.total_norm, r.total_norm, "norm")
        _close(ts.g, r.g, np.abs(r.g), "g")
        _close(ts.m, r.m, np.maximum(np.abs(rm), np.abs(r.g)), "m")
        _close(ts.v, r.v, r.v, "v")
        _close(ts.p, r.p, np.abs(r.p), "p")
        rp, rm, rv = r.p, r.m, r.v
        tp, tm, tv = ts.p, ts.m, ts.v
        g = g * rng.uniform(0.5, 2.0) + 0.1 * rng.standard_normal(g.size)


@pytest.mark.parametrize("spec", R.finite_cases(), ids=lambda s: s[0])
def test_float32_transcription_stays_within_half_of_every_bound(spec):
    """The bounds are honest only if a plain float32 evaluation of the header's formula, with the norm summed in the
    kernel's 1024-strided order, sits well inside them."""
    c = R.build(spec)
    frac = R.worst_fractions(R.f32_step(c.p, c.g, c.m, c.v, **c.kw), c)
    print(spec[0], {k: round(v, 3) for k, v in frac.items()})
    assert all(v <= 0.5 for v in frac.values()), frac


def test_bounds_are_zero_where_the_clip_is_off_and_tight_enough_to_see_a_wrong_formula():
    """Below max_norm the gradient comes back bit for bit, and the parameter bound is small against the effects the
    GPU tests are there to see: eps on the wrong side of the bias correction, and the bias corrections of the double
    betas instead of the float ones at step 1."""
    c = R.build(R.clip_cases()[0])
    b = R.bounds(c.p, c.g, c.m, c.v, **c.kw)
    assert np.all(b.g == 0)
    c = R.consistent_case("far", R.N_GRID, "defaults", 1, seed=3, norm_to=1e-5)
    b = R.bounds(c.p, c.g, c.m, c.v, **c.kw)
    r = R.ref_step(c.p, c.g, c.m, c.v, **c.kw)
    wrong = dict(c.kw, eps=c.kw["eps"] * np.sqrt(c.kw["bc2"]))            # eps inside the division by sqrt(bc2)
    w = R.ref_step(c.p, c.g, c.m, c.v, **wrong)
    assert np.mean(np.abs(w.p - r.p) > b.p) > 0.5
    c = R.consistent_case("t1", R.N_GRID, "defaults", 1, seed=3)
    b = R.bounds(c.p, c.g, c.m, c.v, **c.kw)
    r = R.ref_step(c.p, c.g, c.m, c.v, **c.kw)
    w = R.ref_step(c.p, c.g, c.m, c.v, **dict(c.kw, bc1=1.0 - 0.9, bc2=1.0 - 0.999))
    assert np.mean(np.abs(w.p - r.p) > b.p) > 0.1


@pytest.mark.parametrize("kind", R.NONFINITE)
def test_nonfinite_gradients_in_torch_float32(kind):
    """What clip_grad_norm_ + AdamW do in float32 on the CPU, pinned: a NaN gradient makes the norm, the coefficient and
    with them every gradient, moment and parameter NaN; an infinite element or squares that overflow make the norm inf
    and the coefficient 0, so every finite gradient becomes 0 and NaN appears only where inf * 0 does."""
    c = R.nonfinite_case(kind)
    ts = R.torch_step(c.p, c.g, c.m, c.v, c.t, dtype=torch.float32, **R.abi_scalars(c.kw))
    bad = ~np.isfinite(c.g)
    if kind == "nan":
        assert np.isnan(ts.total_norm)
        assert all(np.all(np.isnan(a)) for a in (ts.p, ts.g, ts.m, ts.v))
    else:
        assert ts.total_norm == np.inf
        for a in (ts.p, ts.g, ts.m, ts.v):
            assert np.array_equal(np.isnan(a), bad) and np.all(np.isfinite(a[~bad]))
        assert np.all(ts.g[~bad] == 0)
        assert bad.sum() == (0 if kind == "overflow" else 1)
    # the restatement and the float32 transcription give the same pattern, and the same finite values within bounds
    ref = R.ref_step(c.p, c.g, c.m, c.v, total_norm=c.norm_override, **c.kw)
    bnd = R.bounds(c.p, c.g, c.m, c.v, total_norm=c.norm_override, **c.kw)
    f = R.f32_step(c.p, c.g, c.m, c.v, **c.kw)
    for q in ("p", "g", "m", "v"):
        want = getattr(ref, q)
        for got in (getattr(ts, q), getattr(f, q)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), q
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok].astype(np.float64) - want[ok]) <= getattr(bnd, q)[ok]), q
    assert np.isnan(f.total_norm) if kind == "nan" else f.total_norm == np.inf
    assert np.isnan(ref.total_norm) if kind == "nan" else ref.total_norm == np.inf
