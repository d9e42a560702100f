"""Host side of the decoder prompts (no GPU): the argument checks of generate(prompt_ids=...), the truncation rule, the position shifting
in WhisperDecoderEngine._params / _set_timestamp_rules, DecodeScores with a prompt, and the token decoder stripping a prompt."""
import ctypes
import json
import os
import types

import pytest
import torch

import whisper_trtllm_amd as wt
from whisper_trtllm_amd import runtime as rt
from whisper_trtllm_amd.text import WhisperTokenDecoder

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_prompt_rows_shapes_and_truncation():
    assert rt.prompt_rows([9, 1, 2], 4, 448) == [[9, 1, 2]]                      # one row shared by the batch
    assert rt.prompt_rows(torch.tensor([[9, 1], [9, 2]]), 2, 448) == [[9, 1], [9, 2]]
    # openai-whisper's _get_initial_tokens: <|startofprev|> + the LAST n_ctx // 2 - 1 prompt tokens
    long = [9] + list(range(100, 400))
    cut = rt.prompt_rows(long, 1, 448)[0]
    assert cut == [9] + list(range(400 - 223, 400)) and len(cut) == 448 // 2
    assert rt.prompt_rows([9] + list(range(223)), 1, 448)[0] == [9] + list(range(223))   # exactly the limit: kept whole
    assert rt.prompt_rows([[9, 1, 2, 3, 4, 5], [8, 6, 7, 8, 9, 10]], 2, 8) == [[9, 3, 4, 5], [8, 8, 9, 10]]
    for bad in ([], [[1, 2], [3]], [[1], [2], [3]]):
        with pytest.raises(ValueError):
            rt.prompt_rows(bad, 2, 448)


def test_prompt_argument_checks():
    ok = [[9, 1, 2]]
    rt._check_prompt_args(ok, 512, 20, 1, False, False)
    for kw in (dict(vocab_size=9), dict(max_length=4), dict(num_beams=2), dict(return_token_timestamps=True), dict(half_engine=True)):
        args = dict(vocab_size=512, max_length=20, num_beams=1, return_token_timestamps=False, half_engine=False)
        args.update(kw)
        with pytest.raises(ValueError):
            rt._check_prompt_args(ok, **args)
    rt._check_prompt_args(ok, 512, 5, 1, False, False)    # 3 prompt tokens + start + one generated token fit max_length 5
    with pytest.raises(ValueError):
        rt._check_prompt_args([[9, -1, 2]], 512, 20, 1, False, False)


def _engine(cfg):
    dec = object.__new__(wt.WhisperDecoderEngine)
    dec.config = cfg
    return dec


def _pairs(p):
    return [(p.forced_decoder_ids[2 * i], p.forced_decoder_ids[2 * i + 1]) for i in range(p.n_forced)]


def test_params_shift_every_position_behind_the_prompt():
    cfg = wt.synthetic.get_config("whisper-tiny.en")
    dec = _engine(cfg)
    p0 = dec._params(None, None, None)
    assert p0.begin_index == 2 and _pairs(p0) == [(1, 50362)]
    p = dec._params(None, None, None, prompt_len=12)
    assert p.begin_index == 14 and _pairs(p) == [(13, 50362)] and p.max_length == p0.max_length
    assert p.decoder_start_token_id == p0.decoder_start_token_id
    multi = _engine(dict(cfg, forced_decoder_ids=[[1, 50259], [2, 50359], [3, 50363]]))
    p = multi._params(None, None, None, prompt_len=5)
    assert p.begin_index == 9 and _pairs(p) == [(6, 50259), (7, 50359), (8, 50363)]
    # timestamp mode: <|notimestamps|> leaves the forced list, the rule's begin_index moves with the prompt
    p = dec._params(None, None, None, return_timestamps=True, prompt_len=12)
    assert p.begin_index == 13 and p.n_forced == 0
    seen = []
    dec.session = types.SimpleNamespace(handle=None, _lib=types.SimpleNamespace(
        wt_decoder_set_timestamp_rules=lambda h, t: seen.append(t._obj if t is not None else None) or 0))
    dec._set_timestamp_rules(True, 12)
    dec._set_timestamp_rules(True)
    dec._set_timestamp_rules(False, 12)
    assert (seen[0].begin_index, seen[1].begin_index, seen[2]) == (14, 2, None)
    assert seen[0].timestamp_begin == seen[1].timestamp_begin == 50363


def test_decode_scores_count_generated_positions_only():
    eos = 7
    #               prompt (3)   start  generated ...
    ids = torch.tensor([[9, 7, 2, 50, 11, 12, 7, 7],      # an EOS id inside the prompt is text there; the row's EOS is its 3rd generated token
                        [9, 1, 2, 50, 11, 12, 13, 14]])   # no EOS: all 4 generated positions
    lp = torch.zeros(2, 8)
    lp[:, 4:] = -0.5
    total = torch.tensor([-1.5, -2.0])
    sc = rt.DecodeScores(ids, lp, total, None, eos, prompt_len=3)
    assert sc.n_scored.tolist() == [3, 4] and sc.prompt_len == 3
    assert torch.allclose(sc.avg_logprob, torch.tensor([-0.5, -0.5]))
    plain = rt.DecodeScores(ids[:, 3:], lp[:, 3:], total, None, eos)
    assert plain.n_scored.tolist() == [3, 4] and plain.prompt_len == 0


@pytest.fixture(scope="module")
def text_golden():
    return json.load(open(os.path.join(GOLDEN_DIR, "text.json"), encoding="utf-8"))


def test_decode_strips_a_leading_prompt(text_golden):
    tok = WhisperTokenDecoder(text_golden["vocab"], text_golden["added_tokens"])
    prev, sot = text_golden["added_tokens"]["<|startofprev|>"], text_golden["added_tokens"]["<|startoftranscript|>"]
    for case in text_golden["cases"]:
        ids = case["ids"]
        # ids without a prompt decode as they always did (the committed reference strings)
        assert tok.decode(ids, skip_special_tokens=True) == case["skip"]
        assert tok.decode(ids, skip_special_tokens=False) == case["keep"]
        if not ids or ids[0] != sot:
            continue
        text_part = [i for i in ids if i not in tok.special_ids and i < tok.timestamp_begin][:5] or [258]
        with_prompt = [prev] + text_part + ids
        assert tok.decode(with_prompt, skip_special_tokens=True) == case["skip"]           # the reference's _strip_prompt
        assert tok.decode(with_prompt, skip_special_tokens=False).startswith("<|startofprev|>")
    assert tok.decode([prev, 258, 264], skip_special_tokens=True) == ""                      # a prompt without a start token: nothing left
    assert tok._strip_prompt([sot, prev, 258]) == [sot, prev, 258]                           # <|startofprev|> not in front: untouched


def test_a_stream_clears_the_prompt_of_an_earlier_decode(monkeypatch):
    """DecodeStream resets every mode a batch decode may have left on the handle before wt_decoder_stream_begin -- the prompt among them,
    which the engine would otherwise refuse the stream for."""
    calls = []

    class Lib:
        def __getattr__(self, name):
            def f(*args):
                calls.append((name, args))
                return 0
            return f

    dec = _engine(wt.synthetic.get_config("toy-short"))
    dec.session = types.SimpleNamespace(handle=None, _lib=Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))   # no GPU here
    rt.DecodeStream(dec, 2)
    names = [n for n, _ in calls]
    assert names[-1] == "wt_decoder_stream_begin" and "wt_decoder_set_prompt" in names[:-1]
    assert dict(calls)["wt_decoder_set_prompt"][1] is None and dec._prompt_len == 0
