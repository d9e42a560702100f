"""GPU: fp16 decoder engines -- `build_decoder.py --engine_precision float16` (reference: TL/examples/whisper/build_decoder.py:25,62,
TL/tensorrt_llm/builder.py:55; fp32 scores kept, TL/tensorrt_llm/models/whisper/model.py:292-295; f32 cache I/O, :464-468).

The reference holds no fp16 fixture (README.md:82-88 publishes fp32+fp32 only) and its fp16 TensorRT engines cannot be built here, so
the fp16 NUMBERS are parity-unpinned by nature.  What is pinned is the arithmetic: the oracle's `fp16_engine` mode (oracle/cpu_ref.py)
evaluates the fp32 model on the fp16-ROUNDED weights with fp16-rounded K/V rows -- exactly what this engine stores -- in fp32 torch,
so logits compare at a few 1e-3 (the engine additionally rounds the folded cross-query matrix once more as a matrix) and ids compare
exactly wherever the oracle's own top-2 margin is healthy (asserted; a thin margin FAILS the test instead of skipping the check)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGITS_TOL = 2e-3   # |engine - fp16 oracle| on logits of scale 6..11: measured 2.0e-4 .. 7.3e-4 (tools/fp16_decoder_error.py; fp32 engines are held to 1e-3 against the fp32 oracle)


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _margin(cpu_ref, cfg, logits):
    """Minimum top-2 margin of the oracle's processed scores over every (row, step)."""
    m = float("inf")
    for t in range(logits.shape[1]):
        sc = cpu_ref.apply_logits_processors(cfg, t + 1, 1, logits[:, t])
        top = torch.topk(sc, 2, -1).values
        mm = top[:, 0] - top[:, 1]
        mm = mm[torch.isfinite(mm)]
        if len(mm):
            m = min(m, float(mm.min()))
    return m


@pytest.mark.parametrize("case,check_ids", [("toy-short_b3", True), ("toy-short-eos1_b3", True), ("toy_b1", True), ("tiny_b2", True),
                                            ("toy-wide_b2", False)])   # toy-wide: the fp16 oracle's margin is 4e-3, too thin for ids
def test_fast_path_matches_the_fp16_oracle(wt, case, check_ids):
    import cpu_ref
    z, cfg, weights, mel = load_case(case)
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    blob = wt.convert.build_decoder_engine(cfg, weights, precision="float16")
    assert len(blob) < 0.62 * len(wt.convert.build_decoder_engine(cfg, weights))     # the weight matrices really are half the bytes
    dec = wt.WhisperDecoderEngine(blob, cfg)
    assert dec.session.info.precision == 1
    hidden = enc(torch.from_numpy(mel).cuda())
    B, V, ml = mel.shape[0], cfg["vocab_size"], cfg["max_length"]
    trace = torch.zeros(B, ml - 1, V, dtype=torch.float32, device="cuda")
    ids = dec.generate(hidden, logits_trace=trace).cpu()
    W16 = cpu_ref.to_torch(cpu_ref.fp16_engine_weights(weights, decoder=True))
    with torch.no_grad():
        ids_ref, logits_ref = cpu_ref.greedy_search(W16, cfg, hidden.cpu(), return_logits=True, fp16_engine=True)
    steps = logits_ref.shape[1]
    err = float((trace[:, :steps].cpu() - logits_ref).abs().max())
    assert err < LOGITS_TOL, err
    if check_ids:
        margin = _margin(cpu_ref, cfg, logits_ref)
        assert margin > 4 * LOGITS_TOL, f"oracle margin {margin} too thin for an id comparison on this case"
        assert ids.shape == ids_ref.shape and torch.equal(ids, ids_ref.to(ids.dtype))
    # and the fp16 engine stays close to the fp32 model it approximates (not a parity claim: a sanity bound on the rounding)
    with torch.no_grad():
        _, logits32 = cpu_ref.greedy_search(cpu_ref.to_torch(weights), cfg, hidden.cpu(), return_logits=True)
    n = min(steps, logits32.shape[1])
    if torch.equal(ids_ref[:, :n + 1], cpu_ref.greedy_search(cpu_ref.to_torch(weights), cfg, hidden.cpu())[:, :n + 1]):
        assert float((trace[:, :n].cpu() - logits32[:, :n]).abs().max()) < 3e-2


@pytest.mark.parametrize("case", ["toy-short_b3", "toy-wide_b2"])
def test_session_protocol_of_an_fp16_decoder_engine(wt, case):
    """By-value Session steps (run.py:103-148): the caches in and out are f32 in fp16 builds too (model.py:464-468)."""
    import cpu_ref
    from test_gpu_session import _dec_inputs
    z, cfg, weights, mel = load_case(case)
    W16 = cpu_ref.to_torch(cpu_ref.fp16_engine_weights(weights, decoder=True))
    L, H, S, V = cfg["decoder_layers"], cfg["decoder_attention_heads"], cfg["max_source_positions"], cfg["vocab_size"]
    sess = wt.Session.from_serialized_engine(wt.convert.build_decoder_engine(cfg, weights, precision="float16"))
    ids = z["ids"]
    with torch.no_grad():
        enc = cpu_ref.encoder_forward(cpu_ref.to_torch(weights), cfg, torch.from_numpy(mel))[:1]
    g = torch.Generator().manual_seed(3)
    sk, sv = torch.rand(L, H, 1, 64, generator=g), torch.rand(L, H, 1, 64, generator=g)
    ck, cv = torch.rand(L, H, S, 64, generator=g), torch.rand(L, H, S, 64, generator=g)
    m_s, m_c = 1, 1
    names = ["hidden_states", "next_self_keys", "next_self_values", "next_cross_keys", "next_cross_values"]
    for t in range(5):
        tok = int(ids[0, t])
        with torch.no_grad():
            want = cpu_ref.engine_decoder_step(W16, cfg, torch.tensor([[tok]], dtype=torch.int32), enc, sk, sv, ck, cv, m_s, m_c, fp16_engine=True)
        out = sess._debug_run(_dec_inputs(wt, cfg, tok, enc, sk, sv, ck, cv, m_s, m_c))
        for n, w_ in zip(names, want):
            assert out[n].dtype == torch.float32
            err = (out[n].cpu() - w_.reshape(out[n].shape)).abs().max().item()
            assert err < (LOGITS_TOL if n == "hidden_states" else 1e-3), (t, n, err)
        sk, sv, ck, cv = (out[n].cpu() for n in names[1:])
        m_s, m_c = 1 + sk.shape[2], S + 1
    # partial cross cache (engine-only quirk, model.py:264-272): the fp16 GEMM writes rows [c, S) of the caller's f32 cache
    sk, sv = torch.randn(L, H, 3, 64, generator=g), torch.randn(L, H, 3, 64, generator=g)
    ck, cv = torch.randn(L, H, S, 64, generator=g), torch.randn(L, H, S, 64, generator=g)
    with torch.no_grad():
        want = cpu_ref.engine_decoder_step(W16, cfg, torch.tensor([[9]], dtype=torch.int32), enc, sk, sv, ck, cv, 3, 11, fp16_engine=True)
    out = sess._debug_run(_dec_inputs(wt, cfg, 9, enc, sk, sv, ck, cv, 3, 11))
    for n, w_ in zip(names, want):
        assert (out[n].cpu() - w_.reshape(out[n].shape)).abs().max().item() < (LOGITS_TOL if n == "hidden_states" else 1e-3), n


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 9, 16])
def test_every_batch_width_is_row_independent(wt, B):
    """NB = 2 / 4 / 8 / 16 instantiations of the half-weight GEMVs and the half-cache attention: row b equals the utterance decoded alone."""
    cfg = wt.synthetic.get_config("toy-short")
    weights = wt.synthetic.make_weights(cfg, 55)
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights, precision="float16"), cfg)
    mel = torch.from_numpy(wt.synthetic.make_mel(cfg, index=500, batch=16)).cuda()
    singles = getattr(test_every_batch_width_is_row_independent, "_singles", None)
    if singles is None:
        singles = [dec.generate(enc(mel[b:b + 1])).cpu().numpy()[0] for b in range(16)]
        test_every_batch_width_is_row_independent._singles = singles
    ids = dec.generate(enc(mel[:B])).cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(ids[b], singles[b])


def test_logprob_and_sampling_forms_at_batch_9(wt):
    """Half weights at batch 9, the smallest batch of the 16-row shapes (more than 48 KiB of dynamic LDS per workgroup): the vocabulary GEMV
    in its log-probability forms (one pair; two pairs with no_speech_token_id) and its sampling form (four waves).  The log-probability forms
    score the ids the plain form picks -- the running argmax is the same code over the same scores -- and each row's log-probabilities are
    those of the row decoded alone within 4 x LOGITS_TOL: either decode is within LOGITS_TOL of the fp16 oracle on every logit, and
    x_tok - lse moves by at most |dx_tok| + max |dx|.  Sampling: finite log-probabilities <= 0 through each row's EOS, bitwise repeatable."""
    cfg = wt.synthetic.get_config("toy-short")
    weights = wt.synthetic.make_weights(cfg, 55)
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights, precision="float16"), cfg)
    hidden = enc(torch.from_numpy(wt.synthetic.make_mel(cfg, index=500, batch=9)).cuda())
    greedy = dec.generate(hidden)
    for ns in (None, 5):
        ids, sc = dec.generate(hidden, return_logprobs=True, no_speech_token_id=ns)
        assert torch.equal(ids, greedy)
        assert torch.isfinite(sc.token_logprobs).all() and (sc.token_logprobs <= 0).all()
        for b in (0, 8):
            alone, s1 = dec.generate(hidden[b:b + 1], return_logprobs=True, no_speech_token_id=ns)
            n = alone.shape[1]
            assert torch.equal(ids[b, :n], alone[0])
            err = (sc.token_logprobs[b, :n] - s1.token_logprobs[0]).abs().max().item()
            assert err <= 4 * LOGITS_TOL, (ns, b, err)
            if ns is not None:
                p, p1 = sc.no_speech_prob[b].item(), s1.no_speech_prob[0].item()
                assert 0.0 < p < 1.0 and abs(p - p1) <= np.expm1(4 * LOGITS_TOL) * p1, (b, p, p1)
    seeds = list(range(70, 79))
    runs = [dec.generate(hidden, return_logprobs=True, temperature=0.8, seeds=seeds) for _ in range(2)]
    (ids, sc), (ids2, sc2) = runs
    assert torch.equal(ids, ids2) and torch.equal(sc.token_logprobs.view(torch.int32), sc2.token_logprobs.view(torch.int32))
    assert torch.isfinite(sc.token_logprobs).all() and (sc.token_logprobs <= 0).all()
    assert ((ids >= 0) & (ids < cfg["vocab_size"])).all()
    assert torch.equal(dec.generate(hidden), greedy)   # and the plain form again, on the same handle


def test_bitwise_reproducible_and_long_decode(wt):
    """tiny.en-shaped model, all 447 steps twice: bitwise equal ids and logits (no atomics on data), self-cache rows up to 447 in fp16."""
    cfg = wt.synthetic.get_config("whisper-tiny.en")
    weights = wt.synthetic.make_weights(cfg, 5)
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights, precision="float16"), cfg)
    hidden = enc(torch.from_numpy(wt.synthetic.make_mel(cfg, index=40, batch=2)).cuda())
    V, ml = cfg["vocab_size"], cfg["max_length"]
    runs = []
    for _ in range(2):
        trace = torch.zeros(2, ml - 1, V, dtype=torch.float32, device="cuda")
        ids = dec.generate(hidden, logits_trace=trace)
        runs.append((ids.cpu(), trace.cpu()))
    assert runs[0][0].shape == (2, ml)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][1]).all()


def test_reference_cli_builds_and_runs_an_fp16_decoder(wt, tmp_path):
    """The reference's own command line: build_encoder.py / build_decoder.py --engine_precision float16 (build_decoder.py:25,62), then
    run.py on the engine directory.  Checkpoint = a local HF-format directory this test writes (no hub access)."""
    from safetensors.numpy import save_file
    import json
    cfg = wt.synthetic.get_config("toy-short")
    weights = wt.synthetic.make_weights(cfg, 3)
    ck = tmp_path / "whisper-toy.en"
    ck.mkdir()
    save_file({k: np.ascontiguousarray(v) for k, v in weights.items() if k != "proj_out.weight"}, str(ck / "model.safetensors"))
    json.dump({k: v for k, v in cfg.items() if k != "name"}, open(ck / "config.json", "w"))
    eng = tmp_path / "engines"
    for script in ("build_encoder.py", "build_decoder.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "whisper", script), "--whisper", str(ck), "--engine_precision", "float16",
                            "--engine_dir", str(eng)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    info, _ = wt.engine_pack.unpack((eng / "WhisperDecoder.engine").read_bytes())
    assert info["precision"] == 1 and info["kind"] == 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "3",
                        "--synthetic_start", "5", "--dump_ids", str(tmp_path / "ids.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = np.array(json.load(open(tmp_path / "ids.json")))
    # the same engines in-process
    enc = wt.WhisperEncoderEngine((eng / "WhisperEncoder.engine").read_bytes())
    dec = wt.WhisperDecoderEngine((eng / "WhisperDecoder.engine").read_bytes(), pickle.load(open(eng / "config.pkl", "rb")))
    mel = torch.from_numpy(wt.synthetic.make_mel(cfg, index=5, batch=3)).cuda()
    want = dec.generate(enc(mel)).cpu().numpy()
    np.testing.assert_array_equal(got[:, :want.shape[1]], want)
