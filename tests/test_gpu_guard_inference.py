"""The inference entry points of the C ABI between guard zones, on poisoned workspaces (``tests/guarded.py``).

Every output buffer is a guarded region at the smallest alignment ``include/cough_amd.h`` documents for it (4 bytes where it
documents none: a float32 / int32 array), every float input is held flush against a trailing guard at its documented
alignment (16 bytes for waveforms at the shipped STFT geometry, 4 otherwise), and every workspace is a guarded region of
exactly ``*_workspace_bytes`` bytes, 256-byte aligned, run once per fill: zeros, all-ones bits, and what a call of another
batch size with a NaN clip left.  The outputs must be bit-equal across the fills and bit-equal to the normal Python path,
which the parity suites hold to their references.  Batch sizes are 1 and 3 (and 5 for the pipeline)."""
import warnings

import pytest
import torch

import cough_detector_amd as cda
import guarded as G
from cough_detector_amd import _lib, synth
from guarded import Guarded
from parity import SHIPPED

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _other(b: int) -> int:
    return 1 if b == 3 else 3


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _with_nan(t: torch.Tensor) -> torch.Tensor:
    """A copy whose last item holds one NaN, a third of the way in."""
    t = t.clone()
    t[-1].view(-1)[t[-1].numel() // 3] = float("nan")
    return t


def _batch(*shape, seed=0, scale=1.0):
    """The input of a call under test: random, and from 3 items on the middle one (item 1) holds a NaN, so that whatever a
    NaN clip skips is read from the workspace as the fill left it, next to clean clips in the same workgroup."""
    t = _rand(*shape, seed=seed, scale=scale)
    if shape[0] >= 3:
        t[1].view(-1)[t[1].numel() // 2] = float("nan")
    return t


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


# ------------------------------------------------------------------ the featuriser's four paths
def _featurize_call(entry, lib, h, wav: Guarded, n_samples, feat_ptr, b, ws_ptr, ws_bytes):
    if entry == "cough_featurize":
        rc = lib.cough_featurize(h, wav.ptr, n_samples, feat_ptr, b, _lib.FEAT_NORMALIZE, _stream())
    elif entry == "cough_featurize_ws":
        rc = lib.cough_featurize_ws(h, wav.ptr, n_samples, feat_ptr, b, _lib.FEAT_NORMALIZE, ws_ptr, ws_bytes, _stream())
    else:
        rc = lib.cough_featurize_any(h, wav.ptr, n_samples, n_samples, feat_ptr, b, _lib.FEAT_NORMALIZE, ws_ptr, ws_bytes,
                                     _stream())
    _lib.check(rc, entry)


def _featurize_guarded(pre, entry, n_samples, path, wav_align, needs_ws):
    lib, h = _lib.load(), pre._native()
    assert pre.kernel_path() == path
    for b in (1, 3):
        w = _batch(b, n_samples, seed=b, scale=0.3)
        want = {"feat": pre.featurize_batch(w.cuda(), normalize=True)}
        assert torch.isfinite(want["feat"][::2]).all() and (b == 1 or torch.isnan(want["feat"][1]).any())
        need = lib.cough_featurizer_workspace_bytes_for(h, n_samples, b)
        assert need > 0 or not needs_ws          # a path without scratch takes NULL, 0 and runs once

        def run(ws_ptr, ws_bytes, more):
            wav = Guarded.holding(w.cuda(), wav_align, name="d_wav")
            feat = G.output(want["feat"].shape, name="d_feat")
            _featurize_call(entry, lib, h, wav, n_samples, feat.ptr, b, ws_ptr, ws_bytes)
            torch.cuda.synchronize()
            return [wav, feat] + more, {"feat": feat.float32.view(want["feat"].shape)}

        if not need:
            guards, got = run(None, 0, [])
            G.check(guards, got, want, f"{entry} b={b}")
            continue
        nb = _other(b)
        other_need = lib.cough_featurizer_workspace_bytes_for(h, n_samples, nb)
        other_wav = Guarded.holding(_with_nan(_rand(nb, n_samples, seed=7, scale=0.3)).cuda(), wav_align)
        other_feat = torch.empty((nb,) + tuple(want["feat"].shape[1:]), device="cuda")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, n: _featurize_call(entry, lib, h, other_wav, n_samples,
                                                                            other_feat.data_ptr(), nb, p, n))
        for fill, ws, more in G.workspaces(need, stale):
            guards, got = run(ws.ptr, need, [ws] + more)
            G.check(guards, got, want, f"{entry} b={b} workspace {fill}")


@pytest.mark.parametrize("flags,rows", [(SHIPPED, 90), ({**SHIPPED, "use_pre_emphasis": True, "use_delta_delta": True}, 103)],
                         ids=["shipped", "preemph_dd"])
def test_featurize_tuned(flags, rows):
    pre = cda.AudioPreprocessor(device="cuda", **flags)
    assert pre.get_num_features() == rows
    _featurize_guarded(pre, "cough_featurize", 16000, "tuned", 16, False)


@pytest.mark.parametrize("kw,path,n_samples,wav_align,needs_ws", [
    (dict(f_max=8000.0), "tuned_fullband", 16000, 16, False),
    (dict(hop_length=200, n_mels=40), "tuned_geometry", 16000, 4, False),
    (dict(hop_length=3, win_length=64, n_mels=32, segment_duration=0.02), "tuned_geometry", 320, 4, False),
    (dict(use_spectral_contrast=True, n_contrast_bands=4), "tuned", 16000, 16, True),
    (dict(n_fft=400), "generic", 16000, 4, True)],
    ids=["fullband", "hop200_mels40", "hop3_win64_mels32_20ms", "contrast4", "n_fft400"])
def test_featurize_ws(kw, path, n_samples, wav_align, needs_ws):
    pre = cda.AudioPreprocessor(device="cuda", **{**SHIPPED, **kw})
    assert pre.segment_samples == n_samples
    _featurize_guarded(pre, "cough_featurize_ws", n_samples, path, wav_align, needs_ws)


@pytest.mark.parametrize("n_samples,needs_ws", [(16300, False), (40000, True)])
def test_featurize_any_other_length(n_samples, needs_ws):
    """Other lengths through the shipped handle: 16300 samples (102 frames) still fit the one-launch run-time-geometry
    kernel and take no scratch; 40000 samples (251 frames) run on the generic chain, with a workspace."""
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    _featurize_guarded(pre, "cough_featurize_any", n_samples, "tuned", 4, needs_ws)


# ------------------------------------------------------------------ the residual net and its taps
def _act_shapes(channels, b, hgt, wid):
    oh, ow = ((hgt - 1) // 2 + 1) // 2, ((wid - 1) // 2 + 1) // 2
    shapes = []
    for c in channels:
        shapes.append((b, c, oh, ow))
        oh, ow = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    return shapes


def _resnet_forward(lib, h, x_ptr, b, hgt, wid, logits, probs, preds, ws_ptr, ws_bytes):
    _lib.check(lib.cough_resnet_forward(h, x_ptr, b, hgt, wid, logits, probs, preds, ws_ptr, ws_bytes, _stream()),
               "cough_resnet_forward")


def _resnet_guarded(model, hgt, wid):
    lib, h = _lib.load(), model._native()
    for b in (1, 3):
        x = _batch(b, 1, hgt, wid, seed=hgt + b)
        logits, probs, preds = _quiet(model._run, x.cuda(), True)
        want = {"logits": logits, "probs": probs, "preds": preds}
        assert torch.isfinite(logits[::2]).all() and (b == 1 or torch.isnan(logits[1]).all())
        shapes = _act_shapes(model.channels, b, hgt, wid)
        for k in range(len(shapes)):
            want[f"a{k + 1}"] = model.read_activation(k + 1)
            assert tuple(want[f"a{k + 1}"].shape) == shapes[k]
        need = lib.cough_resnet_workspace_bytes(h, b, hgt, wid)
        nb = _other(b)
        other_need = lib.cough_resnet_workspace_bytes(h, nb, hgt, wid)
        assert need > 0 and other_need > 0
        other_x = Guarded.holding(_with_nan(_rand(nb, 1, hgt, wid, seed=3)).cuda(), 4)
        other_logits = torch.empty((nb, 2), device="cuda")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, n: _resnet_forward(lib, h, other_x.ptr, nb, hgt, wid,
                                                                            other_logits.data_ptr(), None, None, p, n))
        for fill, ws, more in G.workspaces(need, stale):
            xg = Guarded.holding(x.cuda(), 4, name="d_feat")
            outs = {"logits": G.output((b, 2), name="d_logits"), "probs": G.output((b, 2), name="d_probs"),
                    "preds": G.output((b,), I32, name="d_preds")}
            _resnet_forward(lib, h, xg.ptr, b, hgt, wid, outs["logits"].ptr, outs["probs"].ptr, outs["preds"].ptr, ws.ptr, need)
            for k, shape in enumerate(shapes):
                outs[f"a{k + 1}"] = G.output(shape, name=f"read_activation({k + 1})")
                _lib.check(lib.cough_resnet_read_activation(h, ws.ptr, b, hgt, wid, k + 1, outs[f"a{k + 1}"].ptr, _stream()),
                           "cough_resnet_read_activation")
            torch.cuda.synchronize()
            got = {k: g.view(want[k].dtype).view(want[k].shape) for k, g in outs.items()}
            G.check([xg, ws] + more + list(outs.values()), got, want, f"cough_resnet_forward b={b} workspace {fill}")


def _residual(sd, dtype, channels=(32, 64, 128)):
    m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, channels=channels, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.cuda().eval()


@pytest.mark.parametrize("dtype,shapes", [("bf16x3", [(90, 101), (103, 101), (68, 101), (40, 33)]),
                                          ("bf16_approx", [(90, 101), (110, 101)]), ("fp32", [(17, 33)])])
def test_resnet_forward_and_taps(resnet_golden, dtype, shapes):
    model = _residual(resnet_golden[0], dtype)
    for hgt, wid in shapes:
        _resnet_guarded(model, hgt, wid)


def test_resnet_forward_other_channels_padded_in_the_workspace():
    channels = (5, 7, 9)
    model = _residual(synth.random_state_dict(seed=21, channels=channels), "fp32", channels)
    _resnet_guarded(model, 40, 33)


@pytest.mark.parametrize("case", ["identity", "proj_s1", "proj_s2", "same_s2"])
def test_resblock_forward(resblock_golden, case):
    (cin, cout, stride), sd, x, _ = resblock_golden[case]
    blk = cda.model.ResidualBlock(cin, cout, stride=stride)
    blk.load_state_dict(sd)
    blk = blk.cuda().eval()
    lib, h = _lib.load(), blk._native()
    n, hgt, wid = 2, x.shape[2], x.shape[3]
    x = x[:n].contiguous()
    want = {"y": blk(x.cuda())}
    need = lib.cough_resblock_workspace_bytes(h, n, hgt, wid)
    other_need = lib.cough_resblock_workspace_bytes(h, 3, hgt, wid)
    other_x = Guarded.holding(_with_nan(_rand(3, cin, hgt, wid, seed=5)).cuda(), 4)
    other_y = torch.empty((3,) + tuple(want["y"].shape[1:]), device="cuda")

    def call(x_ptr, nn, y_ptr, p, nbytes):
        _lib.check(lib.cough_resblock_forward(h, x_ptr, nn, hgt, wid, y_ptr, p, nbytes, _stream()), "cough_resblock_forward")

    if need == 0:
        xg, y = Guarded.holding(x.cuda(), 4, name="d_x"), G.output(want["y"].shape, name="d_y")
        call(xg.ptr, n, y.ptr, None, 0)
        torch.cuda.synchronize()
        G.check([xg, y], {"y": y.float32.view(want["y"].shape)}, want, case)
        return
    for fill, ws, more in G.workspaces(need, lambda ws: G.run_other(
            ws, other_need, lambda p, nbytes: call(other_x.ptr, 3, other_y.data_ptr(), p, nbytes))):
        xg, y = Guarded.holding(x.cuda(), 4, name="d_x"), G.output(want["y"].shape, name="d_y")
        call(xg.ptr, n, y.ptr, ws.ptr, need)
        torch.cuda.synchronize()
        G.check([xg, y, ws] + more, {"y": y.float32.view(want["y"].shape)}, want, f"{case} workspace {fill}")


# ------------------------------------------------------------------ the conv-stack nets
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16_approx"])
@pytest.mark.parametrize("kind", ["standard", "small"])
def test_cnn_forward_and_conv_output(cnn_golden, kind, dtype):
    model = cda.create_model(kind, n_mels=90, compute_dtype=dtype)
    model.load_state_dict(cnn_golden[kind][0])
    model = model.cuda().eval()
    lib, h = _lib.load(), model._native()
    for hgt, wid in ((90, 101), (37, 29)):
        for b in (1, 3):
            x = _batch(b, 1, hgt, wid, seed=hgt + b)
            logits, probs, preds = model._run(x.cuda(), True)
            want = {"logits": logits, "probs": probs, "preds": preds}
            assert torch.isfinite(logits[::2]).all() and (b == 1 or torch.isnan(logits[1]).all())
            want_conv = {"conv": model.conv_output(x.cuda())}
            need = lib.cough_cnn_workspace_bytes(h, b, hgt, wid)
            nb = _other(b)
            other_need = lib.cough_cnn_workspace_bytes(h, nb, hgt, wid)
            assert need > 0 and other_need > 0
            other_x = Guarded.holding(_with_nan(_rand(nb, 1, hgt, wid, seed=9)).cuda(), 4)
            other_logits = torch.empty((nb, 2), device="cuda")

            def stale(ws):
                return G.run_other(ws, other_need, lambda p, n: _lib.check(lib.cough_cnn_forward(
                    h, other_x.ptr, nb, hgt, wid, other_logits.data_ptr(), None, None, p, n, _stream()), "cough_cnn_forward"))
            for fill, ws, more in G.workspaces(need, stale):
                xg = Guarded.holding(x.cuda(), 4, name="d_feat")
                outs = {"logits": G.output((b, 2), name="d_logits"), "probs": G.output((b, 2), name="d_probs"),
                        "preds": G.output((b,), I32, name="d_preds")}
                _lib.check(lib.cough_cnn_forward(h, xg.ptr, b, hgt, wid, outs["logits"].ptr, outs["probs"].ptr,
                                                 outs["preds"].ptr, ws.ptr, need, _stream()), "cough_cnn_forward")
                torch.cuda.synchronize()
                got = {k: g.view(want[k].dtype).view(want[k].shape) for k, g in outs.items()}
                G.check([xg, ws] + more + list(outs.values()), got, want,
                        f"cough_cnn_forward {hgt}x{wid} b={b} workspace {fill}")
            for fill, ws, more in G.workspaces(need, stale):
                xg = Guarded.holding(x.cuda(), 4, name="d_feat")
                conv = G.output(want_conv["conv"].shape, name="d_out")
                _lib.check(lib.cough_cnn_conv_output(h, xg.ptr, b, hgt, wid, conv.ptr, ws.ptr, need, _stream()),
                           "cough_cnn_conv_output")
                torch.cuda.synchronize()
                G.check([xg, ws, conv] + more, {"conv": conv.float32.view(want_conv["conv"].shape)}, want_conv,
                        f"cough_cnn_conv_output {hgt}x{wid} b={b} workspace {fill}")


# ------------------------------------------------------------------ the fused pipeline
@pytest.mark.parametrize("flags,rows,golden", [(SHIPPED, 90, None), ({**SHIPPED, "use_delta_delta": True}, 103, "h103"),
                                               ({**SHIPPED, "use_spectral_contrast": True, "n_contrast_bands": 4}, 95, "h95")],
                         ids=["fused_shipped", "delta_delta_two_halves", "contrast4_unfused"])
def test_pipeline_forward(resnet_golden, resnet_heights_golden, flags, rows, golden):
    sd = resnet_golden[0] if golden is None else resnet_heights_golden[golden][0]
    pre = cda.AudioPreprocessor(device="cuda", **flags)
    model = cda.create_model("residual", n_mels=rows, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    model = model.cuda().eval()
    assert pre.get_num_features() == rows and model.effective_dtype(rows, 101) == "bf16x3"
    pipe = cda.CoughPipeline(pre, model)
    lib, fh, mh = _lib.load(), pre._native(), model._native()
    n = 16000

    def call(wav, b, feat, logits, probs, preds, p, nbytes):
        _lib.check(lib.cough_pipeline_forward(fh, mh, wav.ptr, n, b, _lib.FEAT_NORMALIZE, feat, logits, probs, preds, p, nbytes,
                                              _stream(), None, None), "cough_pipeline_forward")

    for b in (1, 3, 5):
        w = _batch(b, n, seed=b, scale=0.3)
        logits, probs, preds, feats = pipe._run(w.cuda(), True, True, True)
        assert torch.isfinite(logits[::2]).all() and (b == 1 or torch.isnan(logits[1]).all())
        full = {"logits": logits, "probs": probs, "preds": preds, "feat": feats}
        assert torch.equal(pipe._run(w.cuda(), True, False, False)[0].view(I32), logits.view(I32))
        need = lib.cough_pipeline_workspace_bytes(fh, mh, b)
        nb = _other(b)
        other_need = lib.cough_pipeline_workspace_bytes(fh, mh, nb)
        assert need > 0 and other_need > 0
        other_wav = Guarded.holding(_with_nan(_rand(nb, n, seed=11, scale=0.3)).cuda(), 16)
        other_logits = torch.empty((nb, 2), device="cuda")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, nbytes: call(other_wav, nb, None, other_logits.data_ptr(), None,
                                                                      None, p, nbytes))
        for with_feat in (False, True):
            for with_probs in (False, True):
                names = ["logits"] + (["probs", "preds"] if with_probs else []) + (["feat"] if with_feat else [])
                want = {k: full[k] for k in names}
                for fill, ws, more in G.workspaces(need, stale):
                    wav = Guarded.holding(w.cuda(), 16, name="d_wav")
                    outs = {k: G.output(want[k].shape, want[k].dtype, name="d_" + k) for k in names}
                    ptr = {k: outs[k].ptr if k in outs else None for k in full}
                    call(wav, b, ptr["feat"], ptr["logits"], ptr["probs"], ptr["preds"], ws.ptr, need)
                    torch.cuda.synchronize()
                    got = {k: g.view(want[k].dtype).view(want[k].shape) for k, g in outs.items()}
                    G.check([wav, ws] + more + list(outs.values()), got, want,
                            f"cough_pipeline_forward b={b} d_feat={with_feat} probs={with_probs} workspace {fill}")
