"""S0/R0/K6: sliding-window engine and device ring buffers vs the CPU oracle."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib, synth
from oracle import engine as oengine, resnet as ores

pytestmark = pytest.mark.gpu

CONFIG = dict(model_type="residual", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400,
              f_min=100.0, f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, use_pcen=False,
              use_pre_emphasis=False, pre_emphasis_coef=0.97, use_delta_delta=False, use_spectral_contrast=False,
              n_contrast_bands=6)


def make_checkpoint(tmp_path, sd):
    path = str(tmp_path / "best_model.pt")
    torch.save({"epoch": 3, "model_state_dict": sd, "optimizer_state_dict": {}, "metrics": {"f1": 0.5},
                "config": CONFIG}, path)                     # schema of src/train.py:192-198
    return path


def test_engine_matches_oracle_stream(tmp_path):
    sd = synth.random_state_dict(seed=5)
    sd["fc.2.bias"] = sd["fc.2.bias"] + torch.tensor([0.0, 0.12])       # probabilities straddle the threshold
    path = make_checkpoint(tmp_path, sd)
    now = {"t": 0.0}
    eng = cda.CoughDetectorInference(path, device="auto", confidence_threshold=0.5, smoothing_window=3,
                                     debounce_seconds=0.5, verbose=False, clock=lambda: now["t"])
    ref = oengine.EngineOracle(sd, 0.5, 3, 0.5, clock=lambda: now["t"])
    stream = synth.make_stream(9, 6.0)
    events, ref_events = [], []
    for i in range(0, len(stream), 1600):                    # 0.1 s chunks, inference.py:259
        now["t"] = (i + 1600) / 16000.0
        a = eng.process_audio_chunk(stream[i:i + 1600])
        b = ref.process_audio_chunk(stream[i:i + 1600])
        events.append(None if a is None else round(a[1], 3))
        ref_events.append(None if b is None else round(b[1], 3))
    assert len(eng.window_probs) == len(ref.window_probs) == 21
    assert np.abs(np.array(eng.window_probs) - np.array(ref.window_probs)).max() < 1e-3
    assert [e is None for e in events] == [e is None for e in ref_events]
    assert any(e is not None for e in events) and any(e is None for e in events[10:])
    is_cough, p = eng.predict(torch.zeros(1, 90, 101))
    assert isinstance(is_cough, bool) and 0.0 <= p <= 1.0
    eng.reset()
    assert len(eng.prediction_history) == 0 and eng.preprocessor.buffer.shape == (1, 0)


def test_engine_rejects_unsupported_checkpoints(tmp_path):
    sd = synth.random_state_dict(seed=5)
    path = str(tmp_path / "m.pt")
    torch.save({"model_state_dict": sd, "config": {**CONFIG, "n_fft": 4096}}, path)
    with pytest.raises(ValueError, match="n_fft"):
        cda.CoughDetectorInference(path, verbose=False)
    torch.save({"model_state_dict": sd, "config": {**CONFIG, "model_type": "small"}}, path)
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):   # a residual state_dict is not a "small" one
        cda.CoughDetectorInference(path, verbose=False)


@pytest.mark.parametrize("kind", ["standard", "small"])
def test_engine_runs_the_other_model_types(tmp_path, cnn_golden, kind):
    """model_type "standard" / "small" checkpoints (src/inference.py:145-151) go through the same engine."""
    from oracle import cnn as ocnn, featurizer as ofeat
    sd, _ = cnn_golden[kind]
    path = str(tmp_path / "m.pt")
    torch.save({"model_state_dict": sd, "config": {**CONFIG, "model_type": kind}}, path)
    now = {"t": 0.0}
    eng = cda.CoughDetectorInference(path, verbose=False, clock=lambda: now["t"], confidence_threshold=2.0)
    stream = synth.make_stream(4, 3.0)
    for i in range(0, len(stream), 1600):
        now["t"] = (i + 1600) / 16000.0
        assert eng.process_audio_chunk(stream[i:i + 1600]) is None           # threshold 2.0 never fires
    win = ofeat.RealtimeWindowerOracle(window_duration=1.0, hop_duration=0.25)
    feats = torch.cat(win.add_audio(torch.from_numpy(stream)[None]))         # (9, 90, 101)
    _, probs = ocnn.predict(kind, feats[:, None], sd)
    assert len(eng.window_probs) == feats.shape[0] == 9
    assert np.abs(np.array(eng.window_probs) - probs[:, 1].numpy()).max() < 1e-3


def test_ring_write_and_window_gather():
    lib = _lib.load()
    S, R, CH, W = 5, 20000, 1600, 16000
    rng = np.random.default_rng(0)
    rings = torch.zeros(S, R, device="cuda")
    host = np.zeros((S, 0), dtype=np.float32)
    wpos = 0
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.arange(S, dtype=torch.int32, device="cuda")
    for step in range(30):                                  # 48000 samples: wraps the 20000-sample ring twice
        chunk = rng.standard_normal((S, CH)).astype(np.float32)
        host = np.concatenate([host, chunk], axis=1)
        pos = torch.full((S,), wpos, dtype=torch.int64, device="cuda")
        dchunk = torch.from_numpy(chunk).cuda()
        _lib.check(lib.cough_ring_write(rings.data_ptr(), R, dchunk.data_ptr(), CH,
                                        ids.data_ptr(), pos.data_ptr(), S, stream), "ring_write")
        wpos += CH
        if wpos >= W + 800 and step % 3 == 0:
            start = wpos - W - (step % 2) * 800
            win_ids = torch.tensor([4, 0, 2], dtype=torch.int32, device="cuda")
            starts = torch.full((3,), start, dtype=torch.int64, device="cuda")
            out = torch.empty(3, W, device="cuda")
            _lib.check(lib.cough_window_gather(rings.data_ptr(), R, win_ids.data_ptr(), starts.data_ptr(), 3, W,
                                               out.data_ptr(), stream), "window_gather")
            want = host[[4, 0, 2], start:start + W]
            assert np.array_equal(out.cpu().numpy(), want)


def test_multi_stream_detector_matches_per_stream_oracles():
    from cough_detector_amd.streaming import MultiStreamDetector
    sd = synth.random_state_dict(seed=5)
    sd["fc.2.bias"] = sd["fc.2.bias"] + torch.tensor([0.0, 0.12])
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1)
    model.load_state_dict(sd)
    S = 5
    now = {"t": 0.0}
    det = MultiStreamDetector(model, S, confidence_threshold=0.5, smoothing_window=3, debounce_seconds=0.5,
                              clock=lambda: now["t"])
    refs = [oengine.EngineOracle(sd, 0.5, 3, 0.5, clock=lambda: now["t"]) for _ in range(S)]
    streams = np.stack([synth.make_stream(20 + s, 3.0) for s in range(S)])
    got_events, ref_events = [], []
    for i in range(0, streams.shape[1], 1600):
        now["t"] = (i + 1600) / 16000.0
        got_events.append(sorted(d[0] for d in det.push(streams[:, i:i + 1600])))
        ref_events.append(sorted(s for s in range(S) if refs[s].process_audio_chunk(streams[s, i:i + 1600]) is not None))
    for s in range(S):
        assert len(det.window_probs[s]) == len(refs[s].window_probs) == 9
        assert np.abs(np.array(det.window_probs[s]) - np.array(refs[s].window_probs)).max() < 1e-3
    assert got_events == ref_events
    # a long chunk that completes several windows at once (ring wrap + multi-window tick)
    det.reset()
    refs = [oengine.EngineOracle(sd, 2.0, 3, 0.5, clock=lambda: now["t"]) for _ in range(S)]   # threshold 2: never fires
    det.threshold = 2.0
    for i in range(0, 48000 - 9600 + 1, 9600):
        det.push(streams[:, i:i + 9600])
        for s in range(S):
            refs[s].process_audio_chunk(streams[s, i:i + 9600])
    for s in range(S):
        assert len(refs[s].window_probs) > 5
        tail = det.window_probs[s][-len(refs[s].window_probs):]
        assert np.abs(np.array(tail) - np.array(refs[s].window_probs)).max() < 1e-3


def test_graph_replay_equals_eager_launches():
    """The captured steady state (two HIP graphs) must give the probabilities of the eager launch chain bit for bit,
    including ticks that fall back to eager (a subset of streams, a longer chunk) in between.  The graphs are captured on
    the warm-up stream, so the pipeline keeps scratch for two streams only: the eager one and the warm-up one."""
    from cough_detector_amd.streaming import MultiStreamDetector
    sd = synth.random_state_dict(seed=5)
    S = 6
    streams = np.stack([synth.make_stream(40 + s, 4.0) for s in range(S)])
    runs = []
    for use_graphs in (True, False):
        model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16_approx")
        model.load_state_dict(sd)
        now = {"t": 0.0}
        det = MultiStreamDetector(model, S, confidence_threshold=0.5, clock=lambda: now["t"], use_graphs=use_graphs)
        events = []
        pos = 0
        for k in range(30):
            now["t"] = (pos + 1600) / 16000.0
            if k == 17:                                   # one tick feeds only three of the streams (eager path) ...
                events.append(det.push(streams[:3, pos:pos + 1600], stream_ids=[0, 1, 2]))
                events.append(det.push(streams[3:, pos:pos + 1600], stream_ids=[3, 4, 5]))   # ... then the rest
            else:
                events.append(det.push(streams[:, pos:pos + 1600]))
            pos += 1600
        runs.append(([list(p) for p in det.window_probs], events, det._g is not None))
        if use_graphs:
            assert len(det.pipe._ws) == 2 and det.pipe._ws.lookup(det.dev) is not None
            assert det._g["workspaces"][0] is not None        # the warm-up stream's, held by the graphs
    (pg, eg, used), (pe, ee, unused) = runs
    assert used and not unused                            # the graph path really ran
    assert all(len(p) == 9 for p in pg)
    assert pg == pe and eg == ee


def test_64_streams_config4_against_per_stream_oracles():
    """BASELINE.json configs[4]: 64 concurrent mic-like streams, 0.1 s chunks, 1 s window / 0.25 s hop, through the
    captured-graph steady state, split-bf16 classifier with a trained-scale head; every stream's window
    probabilities and detections against its own CPU oracle (R0 + M5 + S0 semantics)."""
    from cough_detector_amd.streaming import MultiStreamDetector
    from parity import realistic_state_dict
    sd = realistic_state_dict(5)
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    S, seconds = 64, 2.5
    now = {"t": 0.0}
    det = MultiStreamDetector(model, S, confidence_threshold=0.5, smoothing_window=3, debounce_seconds=0.5,
                              clock=lambda: now["t"])
    refs = [oengine.EngineOracle(sd, 0.5, 3, 0.5, clock=lambda: now["t"]) for _ in range(S)]
    streams = np.stack([synth.make_stream(500 + s, seconds) for s in range(S)])
    got_events, ref_events = [], []
    for i in range(0, streams.shape[1], 1600):
        now["t"] = (i + 1600) / 16000.0
        got_events.append(sorted(d[0] for d in det.push(streams[:, i:i + 1600])))
        ref_events.append(sorted(s for s in range(S) if refs[s].process_audio_chunk(streams[s, i:i + 1600]) is not None))
    assert det._g is not None                                 # the captured steady state really ran
    worst = 0.0
    for s in range(S):
        assert len(det.window_probs[s]) == len(refs[s].window_probs) == 7
        worst = max(worst, float(np.abs(np.array(det.window_probs[s]) - np.array(refs[s].window_probs)).max()))
    print(f"64 streams x 7 windows: max |prob - oracle| {worst:.2e}; detections {sum(map(len, got_events))}")
    assert worst < 1e-3
    assert got_events == ref_events and sum(map(len, got_events)) > 0
    # the bounded poll falls back to a blocking wait without changing results
    det2 = MultiStreamDetector(model, S, confidence_threshold=2.0, clock=lambda: 0.0)
    det2.SPIN_QUERIES = 0
    for i in range(0, 24000, 1600):
        det2.push(streams[:, i:i + 1600])
    assert [p[:3] for p in det2.window_probs] == [p[:3] for p in det.window_probs]


def test_multi_stream_probability_logs_stay_bounded():
    """a 64-stream detector running for days must not keep one float per window forever; the logs keep the
    most recent `prob_history` values (at most twice that between trims), `windows_seen` keeps counting."""
    from cough_detector_amd.streaming import MultiStreamDetector
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1)
    model.load_state_dict(synth.random_state_dict(seed=5))
    S = 3
    det = MultiStreamDetector(model, S, confidence_threshold=2.0, clock=lambda: 0.0, prob_history=6)
    streams = np.stack([synth.make_stream(40 + s, 12.0) for s in range(S)])
    tail = [[] for _ in range(S)]
    for i in range(0, streams.shape[1], 1600):
        before = [len(p) for p in det.window_probs]
        det.push(streams[:, i:i + 1600])
        for s in range(S):
            assert len(det.window_probs[s]) <= 2 * 6 + 1
            if len(det.window_probs[s]) != before[s]:
                tail[s].append(det.window_probs[s][-1])
    assert det.windows_seen == S * 45 and all(len(t) == 45 for t in tail)          # (12 s - 1 s) / 0.25 s + 1 windows per stream
    for s in range(S):
        n = len(det.window_probs[s])
        assert 6 <= n <= 12 and list(det.window_probs[s]) == tail[s][-n:]
    with pytest.raises(ValueError, match="prob_history"):
        MultiStreamDetector(model, S, prob_history=0)
    with pytest.raises(ValueError, match="hop_duration"):
        MultiStreamDetector(model, S, hop_duration=0.0)
