"""GPU: one decoder handle through a sequence of decode configurations (csrc/host_logic.h: DecodeRequest -> DecodeConfig).

The captured step graphs are keyed on the StepKey of the decode in flight: a decode whose key equals the one the graphs were captured
under replays them, any other key drops them.  So, on the whisper-tiny.en synthetic model at batch 2 with max_length 24:
  * whatever ran before on the handle, every decode gives what a fresh handle given only that configuration gives (a stale graph would
    replay the previous decode's temperature, beam table or query-history buffer);
  * the number of step-graph captures (wt_dbg_step_graph_captures) follows from the key rule: a repeated configuration, other seeds or
    other prompt ids of the same length capture nothing; every other switch captures at least once, and its immediate repeat nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ML = 24
HEADS = [(2, 1), (3, 0), (3, 3)]
PROMPT_A = [50360, 1000, 2000, 3000, 4000]
PROMPT_B = [50360, 1111, 2222, 3333, 4444]

# (name, generate() arguments | "stream", batch rows, a capture is due)
SEQUENCE = [
    ("plain", {}, 2, True),
    ("plain again", {}, 2, False),
    ("timestamps", {"return_timestamps": True}, 2, True),
    ("4 beams", {"num_beams": 4, "return_scores": True}, 2, True),
    ("token timestamps", {"return_token_timestamps": True, "alignment_heads": HEADS}, 2, True),
    ("log-probabilities", {"return_logprobs": True, "no_speech_token_id": 50361}, 2, True),
    ("sampling 0.7 seed 11", {"temperature": 0.7, "seed": 11}, 2, True),
    ("sampling 0.7 seed 12345", {"temperature": 0.7, "seed": 12345}, 2, False),
    ("sampling 0.9", {"temperature": 0.9, "seed": 11}, 2, True),
    ("shared prompt", {"prompt_ids": PROMPT_A}, 2, True),
    ("other prompt ids", {"prompt_ids": PROMPT_B}, 2, False),
    ("stream", "stream", 4, True),
    ("plain, batch 1", {}, 1, True),
    ("plain, batch 2", {}, 2, True),
]


def _decode(wt, enc, dec, hidden, mel, kw, rows):
    """-> (ids, {name: float output})"""
    if kw == "stream":   # 2 slots over 4 utterances
        got = wt.transcribe_continuous(enc, dec, torch.from_numpy(mel[:rows]).cuda(), slots=2, chunk=4, max_length=ML)
        return [np.asarray(g) for g in got], {}
    out = dec.generate(hidden[:rows], max_length=ML, **kw)
    if kw.get("return_scores"):
        return out[0].cpu().numpy(), {"beam scores": out[1].cpu().numpy()}
    if kw.get("return_token_timestamps"):
        return out[0].cpu().numpy(), {"token times": out[1].cpu().numpy()}
    if kw.get("return_logprobs"):
        sc = out[1]
        return out[0].cpu().numpy(), {"token_logprobs": sc.token_logprobs.cpu().numpy(), "sum_logprob": sc.sum_logprob.cpu().numpy(),
                                      "no_speech_prob": sc.no_speech_prob.cpu().numpy()}
    return out.cpu().numpy(), {}


@pytest.fixture(scope="module")
def sequence():
    """The sequence once on ONE handle (every configuration twice in a row, the captures counted after each decode), and every
    configuration on a fresh handle of its own."""
    import whisper_trtllm_amd as wt
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    lib = wt._lib.load()
    cfg = wt.synthetic.get_config("whisper-tiny.en")
    cfg["max_length"] = ML
    weights = wt.synthetic.make_weights(cfg, 77)
    mel = wt.synthetic.make_mel(cfg, index=300, batch=4)
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights), cfg)
    hidden = enc(torch.from_numpy(mel[:2]).cuda())
    captures = lambda: int(lib.wt_dbg_step_graph_captures(dec.session.handle))   # noqa: E731
    assert captures() == 0
    steps = []
    for name, kw, rows, _due in SEQUENCE:
        first = _decode(wt, enc, dec, hidden, mel, kw, rows)
        c_first = captures()
        again = _decode(wt, enc, dec, hidden, mel, kw, rows)
        c_again = captures()
        fresh = _decode(wt, enc, dec.clone(), hidden, mel, kw, rows)
        steps.append(dict(name=name, first=first, again=again, fresh=fresh, c_first=c_first, c_again=c_again))
    return steps


# the tolerance each feature's own test file uses against its golden
TOL = {"beam scores": dict(rtol=1e-5, atol=1e-5),          # test_gpu_beam.py
       "token times": dict(rtol=0, atol=0),                # test_gpu_token_timestamps.py: exact
       "token_logprobs": dict(rtol=0, atol=2e-3), "sum_logprob": dict(rtol=0, atol=2e-3 * (ML - 1)),   # test_gpu_logprobs.py: 2e-3 per token
       "no_speech_prob": dict(rtol=2e-3, atol=0)}


def test_every_configuration_decodes_like_a_fresh_handle(sequence):
    for st in sequence:
        ids_fresh, floats_fresh = st["fresh"]
        for which in ("first", "again"):
            ids, floats = st[which]
            assert len(ids) == len(ids_fresh)
            for b in range(len(ids_fresh)):
                np.testing.assert_array_equal(ids[b], ids_fresh[b], err_msg=f"{st['name']} ({which}), row {b}")
            assert floats.keys() == floats_fresh.keys()
            for k, want in floats_fresh.items():
                np.testing.assert_allclose(floats[k], want, err_msg=f"{st['name']} ({which}): {k}", **TOL[k])
    by = {st["name"]: st for st in sequence}
    # the configurations differ where they should: other seeds and another temperature draw other tokens, the prompt ids are in the output
    assert not np.array_equal(by["sampling 0.7 seed 11"]["first"][0], by["sampling 0.7 seed 12345"]["first"][0])
    assert not np.array_equal(by["sampling 0.7 seed 11"]["first"][0], by["sampling 0.9"]["first"][0])
    assert by["shared prompt"]["first"][0][:, :len(PROMPT_A)].tolist() == [PROMPT_A] * 2
    assert by["other prompt ids"]["first"][0][:, :len(PROMPT_B)].tolist() == [PROMPT_B] * 2


def test_captures_follow_the_step_key(sequence):
    before = 0
    for (name, _kw, _rows, due), st in zip(SEQUENCE, sequence):
        added = st["c_first"] - before
        print(f"{name}: {added} capture(s), {st['c_again'] - st['c_first']} on the repeat")
        if due:
            assert added >= 1, f"{name}: a new step key replayed the previous configuration's graphs"
        else:
            assert added == 0, f"{name}: {added} capture(s) although nothing a step graph carries changed"
        assert st["c_again"] == st["c_first"], f"{name}: the immediate repeat captured again"
        before = st["c_again"]
