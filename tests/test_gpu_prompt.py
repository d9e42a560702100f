"""GPU: decoder prompts (wt_decoder_set_prompt, generate(prompt_ids=...)) through the device prefill.

Prefill alone: after `begin` with a prompt, every layer's self K and V at rows 0..len-1 against an fp64 forward of the decoder over the
prompt (tests/prompt_ref.py, fed with the engine's own encoder output, so only the decoder is measured).  Bound: 8 x |fp32 torch forward -
fp64|_inf, measured here -- a margin of 8 over the float32 reference's own error for the engine's other summation orders (MFMA GEMMs, the
folded cross query, tiled attention); printed with the error, and the forced-stepping path's own error beside it.
Decode: the ids of every pr-* golden (tests/golden/make_golden_prompt.py: the reference's greedy_search over [prompt..., start]), the forced
path's ids on a shared prompt, log-probabilities, no_speech_prob, sampling at the absolute positions, mode switching and the refusals.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_case
import prompt_ref
import sampling_ref

pytestmark = pytest.mark.gpu
PR_CASES = ["pr-toy-short_b3", "pr-tiny_b2", "pr-ts-toy_b3", "pr-toy-long_b2"]


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


@functools.lru_cache(maxsize=None)
def _case(case):
    """(golden, cfg, weights, encoder engine, decoder engine, encoder output on the GPU): built once per case, never modified."""
    import whisper_trtllm_amd as w
    z, cfg, weights, mel = load_case(case)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    return z, cfg, weights, enc, dec, enc(torch.from_numpy(mel).cuda())


@pytest.fixture
def whole_prompts(monkeypatch):
    """pr-toy-long_b2 carries 130 prompt tokens at max_target_positions 160 (it is there for the attention's second query block): more than
    openai-whisper's max_target_positions // 2 - 1 that `generate` cuts a prompt to.  The engine behind the C-ABI has no such rule, so the
    tests hand it whole prompts."""
    import whisper_trtllm_amd.runtime as rt
    cut = rt.prompt_rows
    monkeypatch.setattr(rt, "prompt_rows", lambda prompt_ids, batch, max_target_positions: cut(prompt_ids, batch, 1 << 20))


def _forced_cfg(cfg, prompt):
    """The same decode by teacher forcing: the sequence starts at prompt[0], the rest of the prompt and the start token are forced."""
    n = len(prompt)
    forced = [[i, int(prompt[i])] for i in range(1, n)] + [[n, cfg["decoder_start_token_id"]]]
    forced += [[pos + n, tok] for pos, tok in cfg["forced_decoder_ids"]]
    return dict(cfg, decoder_start_token_id=int(prompt[0]), forced_decoder_ids=forced)


def _self_kv(dec, L, H, n):
    """[2][L][B][H][n][64] of the decode in flight."""
    return np.stack([np.stack([np.stack([dec.self_kv_head(l, h, w)[:, :n] for h in range(H)], 1) for l in range(L)]) for w in (0, 1)])


# ---- prefill alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pr-toy-short_b3", "pr-toy-long_b2"])
def test_prefill_leaves_the_prompts_keys_and_values(wt, whole_prompts, case):
    z, cfg, weights, enc, dec, hidden = _case(case)
    prompt = z["prompt"]
    B, n = prompt.shape
    L, H, T = cfg["decoder_layers"], cfg["decoder_attention_heads"], cfg["max_target_positions"]
    # a plain decode first: it fills the caches to max_length, so "rows >= len are untouched" below compares against known contents
    dec.generate(hidden)
    dec.begin(hidden)
    before = np.stack([dec.self_kv_head(l, h, w) for w in (0, 1) for l in range(L) for h in range(H)])
    dec.begin(hidden, prompt_ids=prompt)
    cur, nu, done = dec.poll()
    assert (cur, nu, done) == (n + 1, B, False)
    after = np.stack([dec.self_kv_head(l, h, w) for w in (0, 1) for l in range(L) for h in range(H)])
    assert after.shape[2] == T and np.array_equal(after[:, :, n:], before[:, :, n:], equal_nan=True)
    got = _self_kv(dec, L, H, n)
    enc_cpu = hidden.cpu()
    k64, v64 = prompt_ref.prompt_self_kv(weights, cfg, prompt, enc_cpu, torch.float64)
    k32, v32 = prompt_ref.prompt_self_kv(weights, cfg, prompt, enc_cpu, torch.float32)
    ref = np.stack([k64.numpy(), v64.numpy()])
    bound = 8.0 * max((k32.double() - k64).abs().max().item(), (v32.double() - v64).abs().max().item())
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    per_layer = [float(np.abs(got[:, l] - ref[:, l]).max()) for l in range(L)]
    print(f"\n{case}: prefill K/V err {err:.2e} bound {bound:.2e} ratio {err / bound:.3f} per layer {['%.1e' % e for e in per_layer]}")
    assert err < bound
    # rows carry different prompts: their keys differ from position 1 on (position 0 is <|startofprev|> in every row)
    assert np.abs(got[0, 0, 0, :, 1:] - got[0, 0, 1, :, 1:]).max() > 1e-2
    assert np.array_equal(got[0, 0, 0, :, 0], got[0, 0, 1, :, 0])

    # shared prompt (row 0 for every utterance): the prefill again, and the forced-stepping path's own error beside it
    shared = np.repeat(prompt[:1], B, 0)
    k64, v64 = prompt_ref.prompt_self_kv(weights, cfg, shared, enc_cpu, torch.float64)
    ref = np.stack([k64.numpy(), v64.numpy()])
    dec.begin(hidden, prompt_ids=prompt[0])
    e_pre = np.abs(_self_kv(dec, L, H, n) - ref).max()
    stepped = wt.WhisperDecoderEngine(None, _forced_cfg(cfg, prompt[0]), _session=dec.session.clone())
    stepped.begin(hidden)
    stepped.steps(n)
    e_step = np.abs(_self_kv(stepped, L, H, n) - ref).max()
    print(f"{case}: shared prompt, prefill err {e_pre:.2e}, forced stepping err {e_step:.2e}, bound {bound:.2e}")
    assert e_pre < bound


# ---- decode -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PR_CASES)
def test_ids_equal_the_reference_goldens(wt, whole_prompts, case):
    z, cfg, weights, enc, dec, hidden = _case(case)
    prompt = z["prompt"]
    ids = dec.generate(hidden, prompt_ids=prompt if prompt.shape[0] > 1 else prompt[0], return_timestamps=bool(int(z["timestamp_mode"])))
    np.testing.assert_array_equal(ids.cpu().numpy(), z["ids"])
    n = prompt.shape[1]
    assert (z["ids"][:, :n] == prompt).all() and (z["ids"][:, n] == cfg["decoder_start_token_id"]).all()


@pytest.mark.parametrize("case", ["pr-tiny_b2", "pr-toy-short_b3"])
def test_ids_and_no_speech_equal_the_forced_path_on_a_shared_prompt(wt, case):
    z, cfg, weights, enc, dec, hidden = _case(case)
    prompt = z["prompt"][0]
    n, B, ns = len(prompt), hidden.shape[0], 7
    ids, sc = dec.generate(hidden, prompt_ids=prompt, return_logprobs=True, no_speech_token_id=ns)
    stepped = wt.WhisperDecoderEngine(None, _forced_cfg(cfg, prompt), _session=dec.session.clone())
    trace = torch.full((B, cfg["max_length"] - 1, cfg["vocab_size"]), float("nan"), device="cuda")
    ids_f = stepped.generate(hidden, logits_trace=trace)
    np.testing.assert_array_equal(ids.cpu().numpy(), ids_f.cpu().numpy())
    # the forced path's no_speech_prob at the start token: softmax of the raw logits of its step n
    raw = trace[:, n].double().cpu()
    p = torch.softmax(raw, -1)[:, ns].numpy()
    got = sc.no_speech_prob.cpu().numpy().astype(np.float64)
    print(f"\n{case}: no_speech_prob {got} forced path {p} max diff {np.abs(got - p).max():.2e}")
    assert np.abs(got - p).max() <= 1e-5


def test_logprobs_match_the_golden_and_are_zero_over_the_prompt(wt):
    z, cfg, weights, enc, dec, hidden = _case("pr-toy-short_b3")
    prompt = z["prompt"]
    n = prompt.shape[1]
    ids, sc = dec.generate(hidden, prompt_ids=prompt, return_logprobs=True, no_speech_token_id=int(z["no_speech_token_id"]))
    ids = ids.cpu().numpy()
    np.testing.assert_array_equal(ids, z["ids"])
    got, want = sc.token_logprobs.cpu().numpy(), z["token_logprobs"]   # want: one entry per generated position n + 1 ..
    assert got.shape == ids.shape and want.shape[1] == ids.shape[1] - n - 1
    assert sc.prompt_len == n
    eos = cfg["eos_token_id"]
    worst = 0.0
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, n + 1:] == eos)[0]
        scored = int(hit[0]) + 1 if hit.size else ids.shape[1] - n - 1
        assert (got[b, :n + 1] == 0.0).all()
        err = np.abs(got[b, n + 1:n + 1 + scored] - want[b, :scored]).max()
        worst = max(worst, float(err))
        assert err <= 2e-3, (b, err)
        assert got[b, n + 1] == 0.0 and want[b, 0] == 0.0           # the forced <|notimestamps|> behind the start token
        assert (got[b, n + 1 + scored:] == 0.0).all()
        assert int(sc.n_scored[b]) == scored
        assert sc.avg_logprob[b].item() == np.float32(sc.sum_logprob[b].item()) / np.float32(scored)
    p = z["no_speech_prob"]
    rel = np.abs(sc.no_speech_prob.cpu().numpy().astype(np.float64) - p) / p
    print(f"\npr-toy-short_b3: max |token_logprob - reference| {worst:.3e}, no_speech_prob relative error {rel.max():.3e}")
    assert rel.max() <= 2e-3


def test_sampling_behind_a_prompt_draws_at_the_absolute_positions(wt):
    """Bitwise repeatable, and every token is the argmax of sampling_ref's key at the ABSOLUTE sequence position over the step's own
    (traced) logits after the processors -- a draw at the position without the prompt would pick other tokens."""
    z, cfg, weights, enc, dec, hidden = _case("pr-toy-short_b3")
    prompt, T, seeds = z["prompt"], 0.7, [11, 5, 123456789012]
    n, B, V, ml = prompt.shape[1], hidden.shape[0], cfg["vocab_size"], cfg["max_length"]
    trace = torch.full((B, ml - 1, V), float("nan"), device="cuda")
    ids, sc = dec.generate(hidden, prompt_ids=prompt, temperature=T, seeds=seeds, return_logprobs=True, logits_trace=trace)
    ids2, sc2 = dec.generate(hidden, prompt_ids=prompt, temperature=T, seeds=seeds, return_logprobs=True)
    assert torch.equal(ids, ids2) and torch.equal(sc.token_logprobs, sc2.token_logprobs)
    ids, raw = ids.cpu().numpy(), trace.cpu().numpy()
    eos, checked, other = cfg["eos_token_id"], 0, 0
    for b in range(B):
        for step in range(ids.shape[1] - n - 1):
            t = n + 1 + step                     # the position this step writes
            if (ids[b, n + 1:t] == eos).any():
                break
            if t == n + cfg["forced_decoder_ids"][-1][0]:   # forced <|notimestamps|>, right behind the start token
                assert ids[b, t] == cfg["forced_decoder_ids"][-1][1]
                continue
            s = raw[b, step].astype(np.float32).copy()
            s[cfg["suppress_tokens"]] = -np.inf
            if t == n + 1 + cfg["forced_decoder_ids"][-1][0]:   # begin_index, moved behind the prompt
                s[cfg["begin_suppress_tokens"]] = -np.inf
            k = sampling_ref.keys(s, T, seeds[b], t, np.float32)
            top = np.sort(k[np.isfinite(k)])[-2:]
            if top[1] - top[0] < 1e-4:           # a near-tie of the keys: the device's fp32 logf may order it the other way
                continue
            assert ids[b, t] == sampling_ref.nan_argmax(k), (b, t)
            other += int(sampling_ref.nan_argmax(sampling_ref.keys(s, T, seeds[b], t - n, np.float32)) != ids[b, t])
            checked += 1
    assert checked >= 8 and other > 0, (checked, other)


def test_a_decode_without_prompt_follows_on_the_same_handle(wt):
    z, cfg, weights, enc, dec, hidden = _case("pr-toy-short_b3")
    dec.generate(hidden, prompt_ids=z["prompt"])
    z0, cfg0, _w, _m = load_case("toy-short_b3")      # the same weights and mels, the config without the EOS remapping
    plain = wt.WhisperDecoderEngine(None, cfg0, _session=dec.session)
    np.testing.assert_array_equal(plain.generate(hidden).cpu().numpy(), z0["ids"])
    np.testing.assert_array_equal(dec.generate(hidden, prompt_ids=z["prompt"]).cpu().numpy(), z["ids"])


def test_refusals_leave_the_handle_usable(wt):
    z, cfg, weights, enc, dec, hidden = _case("pr-toy-short_b3")
    lib, h, L = dec.session._lib, dec.session.handle, wt._lib
    prompt = z["prompt"]
    B, n = prompt.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def set_prompt(rows):
        flat = [int(t) for r in rows for t in r]
        arr = (ctypes.c_int32 * len(flat))(*flat)
        return lib.wt_decoder_set_prompt(h, ctypes.byref(L.PromptParams(ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), len(rows), len(rows[0]))))

    def begin(max_length=None):
        p = dec._params(max_length, None, None, prompt_len=n)
        return lib.wt_decoder_begin(h, hidden.data_ptr(), B, ctypes.byref(p), stream)

    assert set_prompt([[cfg["vocab_size"]] + [3] * (n - 1)]) == -22 and "vocabulary" in L.last_error()
    assert set_prompt([[3, -1]]) == -22
    assert set_prompt(prompt[:2]) == 0 and begin() == -22 and "prompt rows" in L.last_error()       # 2 rows for a batch of 3
    assert set_prompt(prompt) == 0 and begin(max_length=n + 1) == -22 and "max_length" in L.last_error()
    assert begin(max_length=n + 2) == 0
    dec._set_beam_search(2)
    assert begin() == -38 and "beam" in L.last_error()
    dec._set_beam_search(1)
    dec._set_token_timestamps([(0, 0)])
    assert begin() == -38 and "token-level timestamps" in L.last_error()
    dec._set_token_timestamps(())
    p = dec._params(None, None, None)
    assert lib.wt_decoder_stream_begin(h, 2, 0, ctypes.byref(p), stream) == -38 and "prompt" in L.last_error()
    half = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights, precision="float16"), cfg)
    hp = (ctypes.c_int32 * n)(*[int(t) for t in prompt[0]])
    assert half.session._lib.wt_decoder_set_prompt(half.session.handle, ctypes.byref(L.PromptParams(ctypes.cast(hp, ctypes.POINTER(ctypes.c_int32)), 1, n))) == 0
    p = half._params(None, None, None, prompt_len=n)
    assert lib.wt_decoder_begin(half.session.handle, hidden.data_ptr(), B, ctypes.byref(p), stream) == -38 and "fp32" in L.last_error()
    with pytest.raises(ValueError):
        half.generate(hidden, prompt_ids=prompt)
    assert lib.wt_decoder_set_prompt(h, None) == 0
    np.testing.assert_array_equal(dec.generate(hidden, prompt_ids=prompt).cpu().numpy(), z["ids"])


def test_a_continuous_decode_follows_a_prompt_decode(wt):
    """dec.stream() clears the prompt a batch decode left on the handle, as it clears the other modes: the caller of stream() asked for none."""
    z, cfg, weights, enc, dec, hidden = _case("pr-toy-short_b3")
    dec.generate(hidden, prompt_ids=z["prompt"])
    st = dec.stream(slots=2)
    handles = st.submit(hidden)
    rows = {}
    while len(rows) < len(handles):
        st.run()
        rows.update(dict(st.collect()))
    plain = dec.generate(hidden).cpu().numpy()
    eos = cfg["eos_token_id"]
    for b, h in enumerate(handles):
        got = np.asarray(rows[h])
        want = plain[b]
        hit = np.nonzero(want[1:] == eos)[0]
        want = want[:hit[0] + 2] if hit.size else want
        np.testing.assert_array_equal(got[:len(want)], want)
    np.testing.assert_array_equal(dec.generate(hidden, prompt_ids=z["prompt"]).cpu().numpy(), z["ids"])


def test_run_py_prompt_ids(wt, tmp_path):
    """run.py --prompt_ids N N ...: one prompt for every utterance, through the pipeline into generate(prompt_ids=...)."""
    import json
    import os
    import pickle
    import subprocess
    import sys
    z, cfg, weights, enc, dec, hidden = _case("pr-tiny_b2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    eng = tmp_path / "engine"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(wt.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(wt.convert.build_decoder_engine(cfg, weights))
    with open(eng / "config.pkl", "wb") as f:
        pickle.dump(cfg, f)
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "2",
                          "--synthetic_start", str(int(z["mel_index"])), "--batching", "dataset", "--workers", "1", "--dump_ids",
                          str(tmp_path / "ids.json"), "--prompt_ids"] + [str(int(t)) for t in z["prompt"][0]],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    np.testing.assert_array_equal(np.array(json.load(open(tmp_path / "ids.json"))), z["ids"])
    bad = subprocess.run([sys.executable, os.path.join(root, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--num_beams", "2",
                          "--prompt_ids", "1", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--prompt_ids" in bad.stderr
