"""GPU: long-form transcription (runtime.transcribe_long: the seek loop batched over recordings, ragged prompts, the windowed front-end)
against tests/longform_ref.py -- the same loop one recording and one window at a time through the calls that existed before (front-end
on a host-made slice, encoder, generate_with_fallback(prompt_ids=...) at batch 1).  Per file: the same windows, the same segments (ids
and times exact), the same temperatures, at max_rows 2 and 3.

Model: toy-ts (window 192 frames = 1.92 s, max_target_positions 64) with the weights of the committed timestamp goldens (seed 32) and
the EOS remap of ts-toy_b3, so that rows do stop.  Audio: three recordings of 1.0 s, 3.1 s and 6.5 s, noise plus modulated tones from
AUDIO_SEED.  The seeds were picked on the batch-1 run alone, for two properties the test asserts: the run takes every branch (a cut at
consecutive timestamps, a full-window advance, and at max_rows 2 a call with an empty prompt beside a non-empty one), and none of its
decisions is a near-tie -- the smallest top-2 gap of the processed scores and the smallest gap of the timestamp rule's comparison stay
above 1e-3 (the criterion of tests/golden/find_healthy_seeds.py; the batched run's logits differ from batch 1 only by summation order,
~1e-5), and with a log-probability threshold no try's avg_logprob lies within 1e-2 of it (5 x the committed log-probability bound)."""
import functools
import json

import numpy as np
import pytest
import torch

from conftest import load_case
import longform_ref

pytestmark = pytest.mark.gpu
WEIGHT_SEED, AUDIO_SEED = 32, 1
SECONDS = (1.0, 3.1, 6.5)
OFF = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None, no_speech_token_id=None)
# avg_logprob of this model's greedy windows lies between -2.16 and -2.49: the threshold sends the lowest of them (the nearest on either
# side are -2.397 and -2.450) to the second temperature, which is above 0.5, so their text leaves the prompt (prompt_reset_since) and the rows sample
HOT = dict(temperatures=(0.0, 0.6), compression_ratio_threshold=None, logprob_threshold=-2.42, no_speech_threshold=None, no_speech_token_id=None)


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _audio(seed, seconds):
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * 16000)
    t = torch.arange(n) / 16000.0
    x = torch.randn(n, generator=g) * 0.05
    for _ in range(4):
        f, a, m = torch.rand(3, generator=g).tolist()
        x += 0.2 * a * torch.sin(2 * np.pi * (200 + 3000 * f) * t) * (0.5 + 0.5 * torch.sin(2 * np.pi * (0.3 + 2 * m) * t))
    return x.float().cuda()


@functools.lru_cache(maxsize=None)
def _setup():
    import whisper_trtllm_amd as w
    z, cfg, _weights, _mel = load_case("ts-toy_b3")           # toy-ts with eos = pad = 81
    assert int(z["seed"]) == WEIGHT_SEED and cfg["eos_token_id"] == 81
    weights = w.synthetic.make_weights(cfg, WEIGHT_SEED)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    fe = w.audio.LogMelFrontend(n_frames=2 * cfg["max_source_positions"])
    prev = int(load_case("pr-ts-toy_b3")[0]["prompt"][0][0])   # the <|startofprev|> of the committed prompt golden
    audios = [_audio(AUDIO_SEED * 10 + k, s) for k, s in enumerate(SECONDS)]
    return cfg, enc, dec, fe, prev, audios


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The batch-1 run of one option set: computed once, shared by the max_rows cases."""
    cfg, enc, dec, fe, prev, audios = _setup()
    opts = dict(OFF if name == "off" else HOT)
    return longform_ref.transcribe_sequential(enc, dec, fe, audios, startofprev=prev, margins=True, seed=5, **opts)


@pytest.mark.parametrize("max_rows", [2, 3])
@pytest.mark.parametrize("name", ["off", "hot"])
def test_batched_loop_equals_the_sequential_restatement(wt, name, max_rows):
    cfg, enc, dec, fe, prev, audios = _setup()
    want_segments, want_windows, gaps = _reference(name)
    opts = dict(OFF if name == "off" else HOT)
    calls = []
    inner = dec.generate_with_fallback

    def recording(hidden, **kw):
        calls.append([len(p) for p in kw["prompts"]])
        return inner(hidden, **kw)

    dec.generate_with_fallback = recording
    try:
        files, trace = wt.runtime.transcribe_long(enc, dec, fe, audios, startofprev_token_id=prev, max_rows=max_rows, seed=5, trace=True, **opts)
    finally:
        del dec.generate_with_fallback
    print(f"\n{name} max_rows {max_rows}: {len(trace)} windows in {len(calls)} calls, batch-1 gaps {json.dumps({k: round(float(v), 5) for k, v in gaps.items()})}")
    # the batch-1 run's own decisions are no near-ties (see the module docstring)
    assert gaps["top2"] >= 1e-3 and gaps["rule5"] >= 1e-3, gaps
    if opts["logprob_threshold"] is not None:
        assert gaps["avg_gap"] >= 1e-2, gaps
    for f in range(len(audios)):
        got_w = [(seek, plen, kind, temp) for file, seek, plen, kind, temp in trace if file == f]
        assert got_w == [w[:4] for w in want_windows[f]], f
        got_s = [(s["start"], s["end"], s["ids"], s["temperature"], s["seek"]) for s in files[f]]
        assert got_s == want_segments[f], f                   # ids and times exact
    # coverage, from the run itself: a missed branch is a failure
    kinds = [w[3] for w in trace]
    assert "cut" in kinds and "full" in kinds, kinds
    assert max(len(c) for c in calls) == max_rows
    if name == "off" and max_rows == 2:      # (at 3 rows all files start together; here the third enters beside a prompted row)
        assert any(0 in c and max(c) > 0 for c in calls), calls
    if name == "hot":
        temps = [w[4] for w in trace]
        assert 0.0 in temps and any(t > 0.5 for t in temps), temps
        hot = [(w[0], w[1]) for w in trace if w[4] > 0.5]
        after = [w for w in trace if any(w[0] == f and w[1] > s for f, s in hot)]
        assert any(w[2] == 0 for w in after if w[1] > 0), "no window behind a hot one started without prompt"


def test_whole_recordings_shorter_than_a_hop_and_wrong_front_end(wt):
    cfg, enc, dec, fe, prev, audios = _setup()
    files = wt.runtime.transcribe_long(enc, dec, fe, [audios[0][:100], audios[0]], startofprev_token_id=prev, **OFF)
    assert files[0] == [] and files[1]
    alone = wt.runtime.transcribe_long(enc, dec, fe, [audios[0]], startofprev_token_id=prev, **OFF)
    assert alone[0] == files[1]
    assert wt.runtime.transcribe_long(enc, dec, fe, []) == []
    with pytest.raises(ValueError):
        wt.runtime.transcribe_long(enc, dec, wt.audio.LogMelFrontend(n_frames=64), audios, startofprev_token_id=prev, **OFF)


def test_run_py_long_form(wt, tmp_path):
    """run.py --long_form: synthetic recordings through runtime.transcribe_long, printed as [start --> end] segments per file."""
    import os
    import pickle
    import subprocess
    import sys
    cfg, enc, dec, fe, prev, audios = _setup()
    import whisper_trtllm_amd as w
    weights = w.synthetic.make_weights(cfg, WEIGHT_SEED)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    eng = tmp_path / "engine"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(w.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(w.convert.build_decoder_engine(cfg, weights))
    with open(eng / "config.pkl", "wb") as f:
        pickle.dump(cfg, f)
    run = [sys.executable, os.path.join(root, "examples", "whisper", "run.py"), "--engine_dir", str(eng)]
    out = subprocess.run(run + ["--long_form", "--synthetic", "3", "--max_rows", "2", "--dump_ids", str(tmp_path / "segments.json")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = json.load(open(tmp_path / "segments.json"))
    assert len(files) == 3 and all(files)
    assert "long form" in out.stdout and out.stdout.count(" --> ") == sum(len(f) for f in files)
    # 2.5 windows of 1.92 s each: the segments come in window order, past the first window, none before its window's offset (what the
    # timestamps inside a window say is the random model's business)
    for segs in files:
        assert all(s["start"] >= s["seek"] * 0.01 - 1e-9 and s["start"] != s["end"] for s in segs)
        assert [s["seek"] for s in segs] == sorted(s["seek"] for s in segs) and segs[-1]["seek"] > 0
    plain = subprocess.run(run + ["--long_form", "--synthetic", "3", "--no_condition_on_previous_text", "--max_rows", "3"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    bad = subprocess.run(run + ["--long_form", "--num_beams", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--long_form" in bad.stderr
