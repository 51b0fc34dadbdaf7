"""The tie-aware parts of the Small / Standard restatements without a GPU (tests/pool_ties_ref.py): the custom 2x2
max-pool against F.max_pool2d bit for bit, and the resolver on the one draw of test_gpu_train_small.py where torch's own
float32 step and the float64 restatement take a pool window differently."""
import pytest
import torch
import torch.nn.functional as F

import pool_ties_ref
import train_small_ref
import train_std_ref
from pool_ties_ref import MaxPool2, choices_that_differ, first_largest, near_ties, tie_census, windows
from test_train_small_host import small_sd
from test_train_std_host import std_sd

GRID = 2.0 ** -6


def _no_pick(v):
    return torch.full((v.shape[0], v.shape[1], v.shape[2] // 2, v.shape[3] // 2), -1, dtype=torch.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 3), (4, 6), (5, 8), (7, 5), (12, 13), (45, 50)])
def test_the_pool_is_max_pool2d_bit_for_bit_with_and_without_exact_ties(h, w, dtype):
    g = torch.Generator().manual_seed(h * 100 + w)
    for levels in (0, 3):                                   # continuous values; three levels: ties in most windows
        v = torch.randn(3, 4, h, w, generator=g, dtype=dtype)
        if levels:
            v = torch.round(v).clamp(-1, 1)
        up = torch.randn(3, 4, h // 2, w // 2, generator=g, dtype=dtype)
        a = v.clone().requires_grad_(True)
        b = v.clone().requires_grad_(True)
        ya, yb = MaxPool2.apply(a, _no_pick(v)), F.max_pool2d(b, 2)
        assert torch.equal(ya, yb)
        ya.backward(up)
        yb.backward(up)
        assert torch.equal(a.grad, b.grad)
        if levels:
            c = tie_census(v)
            assert c["exact"] > 0 or c["positive"] == 0


def test_an_override_routes_the_window_and_is_read_at_backward_time():
    v = torch.tensor([[[[1.0, 3.0, 0.0], [3.0, 2.0, 0.0], [9.0, 9.0, 9.0]]]], requires_grad=True)   # 3 x 3: one window
    pick = _no_pick(v)
    y = MaxPool2.apply(v, pick)
    assert y.item() == 3.0
    y.backward(torch.ones_like(y), retain_graph=True)
    assert v.grad.flatten().tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]         # the first of the two 3s, in scan order
    v.grad = None
    pick[0, 0, 0, 0] = 2
    y.backward(torch.ones_like(y))
    assert v.grad.flatten().tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]


def test_near_ties_excludes_exact_ties_and_non_positive_windows():
    eps = 2.0 ** -30
    v = torch.tensor([[[[1.0, 1.0, 1.0, 1.0 - eps, 0.0, 0.0, -1.0, -1.0 - eps, 2.0, 1.0],
                        [0.5, 0.0, 0.0, 0.0, 0.0, 0.0, -2.0, -2.0, 0.0, 0.0]]]], dtype=torch.float64)
    got = near_ties(v)
    assert [(idx, runner) for _, idx, runner in got] == [((0, 0, 0, 1), 1)]
    assert abs(got[0][0] - eps) < 1e-15
    assert tie_census(v) == {"positive": 3, "exact": 1, "rounding": 0, "near": 1, "grey": 0}
    assert first_largest(windows(v))[0, 0, 0].tolist() == [0, 0, 0, 0, 0]


def _small_qsd():
    sd = dict(small_sd())
    for k in ("features.0.weight", "features.0.bias"):
        sd[k] = torch.round(sd[k] / GRID) * GRID
    sd["classifier.4.weight"] = sd["classifier.4.weight"] / 100
    sd["classifier.4.bias"] = sd["classifier.4.bias"] / 100
    return sd


def _small_batch(b, h, w, seed):
    """test_gpu_train_small._batch"""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(b, 1, h, w, generator=g).clamp(-8, 8) * 1024) / 1024
    y = torch.randint(0, 2, (b,), generator=g)
    mask = (torch.rand(b, 64, generator=g) >= 0.3).float()
    return x, y, mask


def test_the_pool_leaves_the_small_nets_gradients_bit_for_bit(monkeypatch):
    sd = _small_qsd()
    x, y, mask = _small_batch(5, 37, 29, seed=1)
    _, logits, g = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5]).grads(x, y, mask, 0.3)
    monkeypatch.setattr(pool_ties_ref, "pool", lambda ref, v, name, relu=None: F.max_pool2d(v, 2))
    _, tlogits, tg = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5]).grads(x, y, mask, 0.3)
    assert torch.equal(logits, tlogits)
    for n in train_small_ref.PARAM_NAMES:
        assert torch.equal(g[n], tg[n]), n


def test_the_resolver_keeps_exactly_the_choices_torchs_float32_step_takes_differently():
    """(64, 103, 101) at seed 652, the draw test_gpu_train_small.py used to step over: torch's float32 step and the
    float64 restatement differ in one window of the pool after features.11 (relative gap 3.6e-7) and in no ReLU sign.
    Fed the float32 gradients, the resolver must keep that window and nothing else.  What remains between the two is
    torch's own float32 accuracy at this size (1.8e-4 of a tensor's scale here, printed): not this project's to
    bound."""
    sd = _small_qsd()
    x, y, mask = _small_batch(64, 103, 101, seed=64 * 7 + 103 + 101)
    r32 = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5], dtype=torch.float32)
    _, _, g32 = r32.grads(x, y, mask, 0.3)
    g32 = {n: v.double() for n, v in g32.items()}
    r64 = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5])
    _, logits, rg = r64.grads(x, y, mask, 0.3)
    differ = choices_that_differ(r32, r64)
    print("choices torch's float32 step takes differently:", differ)
    assert len(differ) == 1 and next(iter(differ))[0] == "p2"
    before = train_small_ref._worst(g32, rg)
    pre = {k: v.clone() for k, v in r64.pre.items()}
    out, kept = train_small_ref.resolve_kinks(g32, r64, rg, ties=True)
    after = train_small_ref._worst(g32, out)
    print(f"worst gradient difference {before:.2e} -> {after:.2e} of scale; kept {kept}")
    assert {(name, idx) for name, idx, _ in kept} == differ
    assert 0 < kept[0][2] < 1e-6
    assert after < before
    # the forward pass is not the resolver's to touch
    assert all(torch.equal(pre[k], r64.pre[k]) for k in pre)
    # without ties the window is out of reach: whatever the ReLU flips do, the set is not the one that differs
    r64b = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5])
    _, _, rgb = r64b.grads(x, y, mask, 0.3)
    _, kept_b = train_small_ref.resolve_kinks(g32, r64b, rgb)
    assert all(name != "p2" for name, _, _ in kept_b)


def test_a_relu_input_taken_as_positive_brings_its_all_zero_window_with_it():
    """(8, 103, 101), the second batch of seed 1: the stem ReLU input at (4, 12, 85, 55) is -9.5e-9 in float64 and was
    +1.5e-8 in torch's float32 step, in a pool window whose other three outputs are 0.  Float32 gives the window to that
    pixel; float64 gives it to the window's first pixel, where a flipped derivative would never be read.  Flip and
    window are one choice.  The float32 side is built here (the same restatement with that pixel taken as positive), so
    that the test does not hang on one machine's float32 rounding: it moves features.1.bias by 1e-3 of its scale, and
    the resolver finds exactly it."""
    sd = _small_qsd()
    x, y, _ = _small_batch(20, 103, 101, seed=1)
    x, y = x[8:16], y[8:16]
    mask = (torch.rand(8, 64, generator=torch.Generator().manual_seed(1)) >= 0.3).float()
    idx = (4, 12, 85, 55)
    other = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5])
    other.grads(x, y, mask, 0.3)
    assert -1e-7 < other.pre["stem"][idx] < 0 and windows(other.pool_in["p0"])[4, 12, 42, 27].max() == 0
    other.flip["stem"][idx] = True
    other.pick["p0"][4, 12, 42, 27] = 3
    g = other.regrad()
    ref = train_small_ref.RefStep(sd, class_weights=[1.0, 2.5])
    _, _, rg = ref.grads(x, y, mask, 0.3)
    before = train_small_ref._worst(g, rg)
    out, kept = train_small_ref.resolve_kinks(g, ref, rg, ties=True)
    after = train_small_ref._worst(g, out)
    print(f"worst gradient difference {before:.2e} -> {after:.2e} of scale; kept {kept}")
    assert before > 5e-4 and after < 1e-12
    assert [(name, i) for name, i, _ in kept] == [("stem", idx)]
    assert ref.pick["p0"][4, 12, 42, 27] == 3 and (ref.pick["p0"] >= 0).sum() == 1
    # the flip alone changes nothing: the window's gradient goes to its first pixel
    ref.pick["p0"][4, 12, 42, 27] = -1
    assert train_small_ref._worst(g, ref.regrad()) == before


def test_the_resolver_takes_a_head_relu_input_which_has_no_pool_behind_it():
    """the fc ReLU's inputs are (B, hidden): no window goes with them"""
    class Ref:
        pre = {"fc": torch.tensor([[0.5, -3e-7], [2e-7, -1.0]], dtype=torch.float64)}
        flip = {"fc": torch.zeros(2, 2, dtype=torch.bool)}
        pool_in, pick, pool_of = {}, {}, {}

        def regrad(self):
            return {"w": ((self.pre["fc"] > 0) ^ self.flip["fc"]).double()}

    ref = Ref()
    g = {"w": torch.tensor([[1.0, 1.0], [1.0, 0.0]], dtype=torch.float64)}          # the other side of -3e-7 only
    worst = lambda a, b: (a["w"] - b["w"]).abs().max().item()
    out, kept = pool_ties_ref.resolve(g, ref, ref.regrad(), worst, ties=True)
    assert kept == [("fc", (0, 1), -3e-7)] and worst(g, out) == 0
    assert ref.flip["fc"].tolist() == [[False, True], [False, False]]


@pytest.mark.parametrize("kind", ["small", "standard"])
def test_a_case_within_rtol_comes_back_as_the_same_object(kind):
    if kind == "small":
        sd, mod = _small_qsd(), train_small_ref
        x, y, mask = _small_batch(3, 17, 16, seed=2)
        args = (0.3,)
    else:
        sd, mod = dict(std_sd()), train_std_ref
        x, y, _ = _small_batch(2, 16, 19, seed=2)
        mask = torch.ones(2, train_std_ref.MASK_WIDTH)
        args = (0.1, 0.5)
    ref = mod.RefStep(sd)
    _, _, rg = ref.grads(x, y, mask, *args)
    g = {n: v.clone() for n, v in rg.items()}
    out, kept = mod.resolve_kinks(g, ref, rg, ties=True)
    assert out is rg and kept == []
    assert all(not f.any() for f in ref.flip.values()) and all((p < 0).all() for p in ref.pick.values())
