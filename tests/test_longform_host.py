"""Host side of long-form transcription (no GPU): the segment cutting and seek advance of one window on literal token lists (expected
values derived by hand from openai-whisper's transcribe(), as restated in DESIGN.md "Long-form transcription"), the seek loop over a
scripted decode_fn (windows visited, prompts, prompt reset, no-speech skip, seeds, independence of max_rows), and the argument checks of
generate(prompts=...)."""
import os
import re
import types

import pytest
import torch

import whisper_trtllm_amd as wt
from whisper_trtllm_amd import longform as lf
from whisper_trtllm_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0, EOS, PREV = 1000, 999, 998      # timestamp_begin, EOS, <|startofprev|> of the literal cases
TP, STRIDE, N = 0.02, 2, 3000


def _split(tokens, seek=0, size=N):
    segs, advance, kind = lf.split_window(tokens, T0, EOS, seek, size, TP, STRIDE)
    return [(round(s, 9), round(e, 9)) for s, e, _ in segs], [t for _, _, ids in segs for t in ids], advance, kind


# ---- (a) one window ------------------------------------------------------------------------------------------------------------------
def test_case_a_cut_at_the_last_consecutive_timestamps():
    toks = [T0, 5, 6, T0 + 50, T0 + 50, 7, T0 + 120, T0 + 120, 8, 9]
    times, kept, advance, kind = _split(toks)
    assert times == [(0.00, 1.00), (1.00, 2.40)]
    assert kept == toks[:7]            # the tokens behind the last cut are dropped: the next window decodes them again
    assert (advance, kind) == (240, "cut")


def test_case_b_a_single_closing_timestamp_takes_the_whole_window():
    toks = [T0, 5, 6, T0 + 200]
    assert _split(toks) == ([(0.00, 4.00)], toks, 3000, "full")


def test_case_c_consecutive_timestamps_and_a_single_end():
    toks = [T0, 5, T0 + 100, T0 + 100, 6, T0 + 300]
    assert _split(toks) == ([(0.00, 2.00), (2.00, 6.00)], toks, 3000, "full")


def test_case_d_no_timestamps_at_all():
    assert _split([5, 6, 7]) == ([(0.00, 30.00)], [5, 6, 7], 3000, "full")
    # 1234 frames of content left: the segment ends with the content, and so does the advance
    assert _split([5, 6, 7], seek=0, size=1234) == ([(0.00, 12.34)], [5, 6, 7], 1234, "full")
    times, kept, advance, _ = _split([5, 6, 7], seek=500, size=1234)
    assert times == [(5.00, 17.34)] and advance == 1234


def test_case_e_an_empty_cut_is_dropped_and_the_guard_advances():
    assert _split([T0, T0]) == ([], [], 3000, "guard")     # start == end: no segment; an advance of 0 frames becomes the window


def test_segments_without_text_are_dropped_and_times_carry_the_offset():
    times, kept, advance, kind = _split([T0, T0 + 40, T0 + 40, 5, T0 + 90, T0 + 90], seek=1000)
    assert times == [(10.80, 11.80)] and kept == [T0 + 40, 5, T0 + 90] and (advance, kind) == (180, "cut")
    assert _split([]) == ([], [], 3000, "full")             # EOS at once


# ---- (b) the loop --------------------------------------------------------------------------------------------------------------------
class Script:
    """decode_fn returning scripted token lists per (file, seek) and recording every call."""

    def __init__(self, table, default=None):
        self.table, self.default, self.calls = table, default, []

    def __call__(self, requests):
        self.calls.append([dict(r) for r in requests])
        out = []
        for r in requests:
            e = self.table.get((r["file"], r["seek"]), self.default)
            assert e is not None, ("unscripted window", r["file"], r["seek"])
            e = e if isinstance(e, dict) else dict(tokens=e)
            out.append(dict(dict(tokens=[], temperature=0.0, avg_logprob=-0.3, no_speech_prob=0.1, compression_ratio=1.0), **e))
        return out


def _run(script, frames, **kw):
    args = dict(n_ctx=448, max_source_positions=1500, timestamp_begin=T0, eos_token_id=EOS, startofprev_token_id=PREV, trace=True)
    args.update(kw)
    return lf.transcribe(script, frames, **args)


def _windows_of(trace, f):
    return [w for w in trace if w[0] == f]


A_TOKS = [T0, 5, 6, T0 + 50, T0 + 50, 7, T0 + 120, T0 + 120, 8, 9]


def test_loop_seeks_prompts_and_seeds():
    script = Script({(0, 0): A_TOKS, (0, 240): [T0, 8, 9, T0 + 200], (0, 3240): [T0, 10, T0 + 30]})
    segs, trace = _run(script, [3300], seed=7)
    assert [w[1] for w in trace] == [0, 240, 3240]                       # cut at 2.40 s, then a whole window, then the 60-frame tail
    assert [w[3] for w in trace] == ["cut", "full", "full"]
    prompts = [c[0]["prompt"] for c in script.calls]
    assert prompts[0] == []
    assert prompts[1] == [PREV] + A_TOKS[:7]                             # timestamp tokens stay in the prompt
    assert prompts[2] == [PREV] + A_TOKS[:7] + [T0, 8, 9, T0 + 200]
    assert [c[0]["segment_size"] for c in script.calls] == [3000, 3000, 60]
    assert [c[0]["seed"] for c in script.calls] == [7, 7 + 240, 7 + 3240]
    assert [(round(s["start"], 9), round(s["end"], 9), s["seek"]) for s in segs[0]] == [(0.0, 1.0, 0), (1.0, 2.4, 0), (2.4, 6.4, 240), (32.4, 33.0, 3240)]
    assert segs[0][2]["ids"] == [T0, 8, 9, T0 + 200] and segs[0][0]["temperature"] == 0.0
    assert [w[2] for w in trace] == [0, 8, 12]


def test_prompt_is_cut_to_half_the_context_and_seeded_by_initial_prompt_ids():
    long = [T0] + list(range(1, 301)) + [T0 + 100]                        # 302 tokens in one segment
    script = Script({(0, 0): long, (0, 3000): [T0, 5, T0 + 10]})
    _segs, trace = _run(script, [3100], initial_prompt_ids=[400, 401])
    assert script.calls[0][0]["prompt"] == [PREV, 400, 401]
    p = script.calls[1][0]["prompt"]
    assert len(p) == 448 // 2 and p == [PREV] + ([400, 401] + long)[-223:]
    # a small context: n_ctx 64 keeps 31
    script = Script({(0, 0): long, (0, 3000): [T0, 5, T0 + 10]})
    _run(script, [3100], n_ctx=64)
    assert script.calls[1][0]["prompt"] == [PREV] + long[-31:]


def test_prompt_reset_behind_a_hot_window_and_not_behind_a_warm_one():
    w = lambda t: dict(tokens=[T0, 5, T0 + 1500], temperature=t)
    script = Script({(0, 0): w(0.0), (0, 3000): w(0.6), (0, 6000): w(0.4), (0, 9000): w(0.0)})
    _segs, trace = _run(script, [12000])
    p = [c[0]["prompt"] for c in script.calls]
    assert p[1] == [PREV, T0, 5, T0 + 1500]
    assert p[2] == []                                                   # the window at 0.6 > 0.5 reset the prompt behind itself
    assert p[3] == [PREV, T0, 5, T0 + 1500]                             # the one at 0.4 did not: its own tokens are the next prompt
    assert [w_[4] for w_ in trace] == [0.0, 0.6, 0.4, 0.0]
    script = Script({}, default=[T0, 5, T0 + 1500])
    _run(script, [9000], condition_on_previous_text=False)
    assert [c[0]["prompt"] for c in script.calls] == [[], [], []]


def test_no_speech_skip_and_its_logprob_override():
    quiet = dict(tokens=[T0, 5, T0 + 100], no_speech_prob=0.9, avg_logprob=-2.0)
    sure = dict(tokens=[T0, 6, T0 + 100], no_speech_prob=0.9, avg_logprob=-0.5)     # confident text wins over the no-speech probability
    script = Script({(0, 0): quiet, (0, 3000): sure, (0, 6000): [T0, 7, T0 + 100]})
    segs, trace = _run(script, [9000])
    assert [w[3] for w in trace] == ["skip", "full", "full"] and [w[1] for w in trace] == [0, 3000, 6000]
    assert [s["ids"] for s in segs[0]] == [[T0, 6, T0 + 100], [T0, 7, T0 + 100]]
    assert script.calls[1][0]["prompt"] == []                           # nothing of a skipped window is recorded
    script = Script({(0, 0): quiet, (0, 3000): sure, (0, 6000): [T0, 7, T0 + 100]})
    segs, trace = _run(script, [9000], logprob_threshold=None)          # no override: both quiet windows are skipped
    assert [w[3] for w in trace] == ["skip", "skip", "full"]
    script = Script({(0, 0): quiet, (0, 3000): sure, (0, 6000): [T0, 7, T0 + 100]})
    segs, trace = _run(script, [9000], no_speech_threshold=None)
    assert [w[3] for w in trace] == ["full", "full", "full"]


def _three_files():
    table = {(0, 0): A_TOKS, (0, 240): [T0, 8, 9, T0 + 200],
             (1, 0): [T0, 20, T0 + 400, T0 + 400, 21, T0 + 900], (1, 3000): [T0, 22, T0 + 700, T0 + 700], (1, 4400): [T0, 23, T0 + 80],
             (2, 0): [T0, 30, 31, T0 + 50]}
    return table, [3240, 4500, 100, 0]


def test_results_do_not_depend_on_max_rows_and_a_new_file_enters_without_prompt():
    table, frames = _three_files()
    runs = {}
    for rows in (1, 2, 3):
        script = Script(table)
        segs, trace = _run(script, frames, max_rows=rows, seed=3)
        runs[rows] = (segs, [sorted(_windows_of(trace, f)) for f in range(4)], script.calls)
        assert max(len(c) for c in script.calls) == min(rows, 3)
        assert segs[3] == [] and not _windows_of(trace, 3)              # content_frames == 0: no segments, never decoded
    assert runs[1][0] == runs[2][0] == runs[3][0] and runs[1][1] == runs[2][1] == runs[3][1]
    assert [w[1] for w in runs[1][1][1]] == [0, 3000, 4400]
    # max_rows 2: file 0 ends after two windows and file 2 takes its row, without prompt, beside file 1's third window
    third = runs[2][2][2]
    assert [(r["file"], r["seek"]) for r in third] == [(1, 4400), (2, 0)]
    assert third[1]["prompt"] == [] and third[0]["prompt"][0] == PREV and len(third[0]["prompt"]) > 1
    assert third[1]["seed"] == 3 + (2 << 32) and third[0]["seed"] == 3 + (1 << 32) + 4400
    with pytest.raises(ValueError):
        _run(Script(table), frames, max_rows=17)
    assert _run(Script({}), []) == ([], [])


def test_generation_budget_fits_behind_the_longest_prompt():
    assert lf.generation_budget(448, 0) == 223 and lf.generation_budget(64, 0) == 31 and lf.generation_budget(448, 2) == 221
    for n_ctx, forced in ((448, 0), (64, 0), (65, 1)):
        assert n_ctx // 2 + 1 + forced + lf.generation_budget(n_ctx, forced) <= n_ctx


# ---- (c) prompts= ----------------------------------------------------------------------------------------------------------------------
def test_ragged_prompt_rows_and_strip():
    assert rt.ragged_prompt_rows([[9, 1, 2], [], [9, 5]], 3, 448) == [[9, 1, 2], [], [9, 5]]
    assert rt.ragged_prompt_rows([[9, 1, 2, 3, 4, 5], [8, 6]], 2, 8) == [[9, 3, 4, 5], [8, 6]]      # the text part cut to 8 // 2 - 1
    with pytest.raises(ValueError):
        rt.ragged_prompt_rows([[9, 1], []], 3, 448)                      # wrong row count
    ids = torch.tensor([[7, 7, 9, 1, 50, 11, 7, 7], [9, 1, 2, 3, 50, 12, 13, 14]])
    assert rt.strip_prompts(ids, 4, eos_token_id=7) == [[50, 11, 7], [50, 12, 13, 14]]
    assert rt.strip_prompts(ids, 4) == [[50, 11, 7, 7], [50, 12, 13, 14]]


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _engine(monkeypatch, precision=0):
    dec = object.__new__(wt.WhisperDecoderEngine)
    dec.config = wt.synthetic.get_config("toy-short")
    info = types.SimpleNamespace(max_target_positions=40, vocab_size=512, precision=precision, max_source_positions=96, d_model=128)
    dec.session = types.SimpleNamespace(handle=None, _lib=_Lib(), info=info)
    dec.max_batch = 16
    begun = []
    monkeypatch.setattr(wt.WhisperDecoderEngine, "begin", lambda self, *a, **k: begun.append(k))
    monkeypatch.setattr(wt.WhisperDecoderEngine, "run", lambda self, lookahead=0: (3, 0))
    monkeypatch.setattr(wt.WhisperDecoderEngine, "read_ids", lambda self, cur: torch.zeros(2, cur, dtype=torch.int32))
    return dec, begun


def test_prompts_argument_checks(monkeypatch):
    dec, begun = _engine(monkeypatch)
    hidden = torch.zeros(2, 96, 128)
    for bad in (dict(prompts=[[9, 1]]),                                   # one row for a batch of two
                dict(prompts=[[9, 1], [9, 512]]),                         # an id outside the vocabulary
                dict(prompts=[[9, 1], [9, -1]]),
                dict(prompts=[[9, 1], []], prompt_ids=[9, 1]),            # both kinds of prompt
                dict(prompts=[[9, 1, 2, 3], [9]], max_length=5),          # Lmax + 2 > max_length
                dict(prompts=[[9, 1], []], num_beams=2),
                dict(prompts=[[9, 1], []], return_token_timestamps=True, alignment_heads=[(0, 0)])):
        with pytest.raises(ValueError):
            dec.generate(hidden, **bad)
    assert not begun
    dec.generate(hidden, prompts=[[9, 1, 2, 3], [9]], max_length=6)       # Lmax + 2 == max_length
    assert begun[-1]["prompts"] == [[9, 1, 2, 3], [9]]
    dec.generate(hidden, prompts=[[], []])                                 # all rows empty: the decode without prompt
    assert "prompts" not in begun[-1] and "prompt_ids" not in begun[-1]
    half, _ = _engine(monkeypatch, precision=1)
    with pytest.raises(ValueError):
        half.generate(hidden, prompts=[[9, 1], []])
    with pytest.raises(ValueError):
        dec.generate_with_fallback(hidden, prompts=[[9, 1], []], prompt_ids=[9, 1])


def test_set_prompt_hands_the_engine_rows_and_lengths(monkeypatch):
    dec = object.__new__(wt.WhisperDecoderEngine)
    dec.session = types.SimpleNamespace(handle=None, _lib=_Lib())
    dec._set_prompt([[9, 1, 2], [], [9, 5]], ragged=True)
    name, (_h, ids, n_rows, ld, lens) = dec.session._lib.calls[-1]
    assert name == "wt_decoder_set_prompt_rows" and (n_rows, ld) == (3, 3) and dec._prompt_len == 3
    assert [lens[i] for i in range(3)] == [3, 0, 2] and [ids[i] for i in range(9)] == [9, 1, 2, 0, 0, 0, 9, 5, 0]
    dec._set_prompt(None)
    assert dec.session._lib.calls[-1][0] == "wt_decoder_set_prompt" and dec._prompt_len == 0


def test_header_declares_the_new_calls_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "whisper_trtllm_amd.h"), encoding="utf-8").read()
    assert re.search(r"int\s+wt_decoder_set_prompt_rows\(wt_engine\*\s*dec,\s*const int32_t\*\s*ids,\s*int n_rows,\s*int ld,\s*const int32_t\*\s*lens\);", header)
    assert re.search(r"int\s+wt_logmel_forward_windows\(wt_logmel\*\s*h,\s*const float\*\s*audio,\s*const int64_t\*\s*offsets,\s*const int32_t\*\s*n_valid,"
                     r"\s*int batch,\s*float\*\s*mel_out,\s*void\*\s*stream\);", header)
    lib = wt._lib.load()
    assert lib.wt_abi_version() == 3 and wt._lib.ABI_VERSION == 3
    assert hasattr(lib, "wt_decoder_set_prompt_rows") and hasattr(lib, "wt_logmel_forward_windows")


def test_more_than_sixteen_rows_are_sliced_and_shifted_to_the_longest_prompt(monkeypatch):
    """Engine batches of a larger batch are left-padded to their OWN longest prompt and get max_length lowered by the difference; the
    parts come back shifted to the whole batch's, the start token of every row in one column."""
    dec, _ = _engine(monkeypatch)
    state, seen = {}, []
    pad, start = dec.config["pad_token_id"], dec.config["decoder_start_token_id"]

    def begin(self, enc, max_length=None, *a, **k):
        rows = k.get("prompts")
        state.update(B=enc.shape[0], L=max(len(r) for r in rows) if rows else 0, ml=max_length)
        seen.append((enc.shape[0], state["L"], max_length))
        self._prompt_len = state["L"]

    def read_ids(self, cur):
        t = torch.full((state["B"], cur), 7, dtype=torch.int32)
        t[:, state["L"]] = start
        return t

    monkeypatch.setattr(wt.WhisperDecoderEngine, "begin", begin)
    monkeypatch.setattr(wt.WhisperDecoderEngine, "run", lambda self, lookahead=0: (state["ml"], 0))
    monkeypatch.setattr(wt.WhisperDecoderEngine, "read_ids", read_ids)
    monkeypatch.setattr(wt.WhisperDecoderEngine, "read_logprobs",
                        lambda self, ids: rt.DecodeScores(ids, torch.ones(ids.shape), torch.zeros(ids.shape[0]), None, 432, state["L"]))
    hidden = torch.zeros(18, 96, 128)
    prompts = [[9, 1, 2, 3]] + [[9, 1]] * 15 + [[], [9]]
    ids, sc = dec.generate(hidden, prompts=prompts, max_length=12, return_logprobs=True)
    assert seen == [(16, 4, 12), (2, 1, 9)]                      # the second engine batch: longest prompt 1, the same 7 generated tokens
    assert ids.shape == (18, 12) and (ids[:, 4] == start).all() and sc.prompt_len == 4
    assert ids[16].tolist()[:4] == [pad, pad, pad, 7] and (sc.token_logprobs[16:, :3] == 0).all() and (sc.token_logprobs[16:, 3:] == 1).all()
    assert dec.generate(hidden, prompts=prompts, max_length=12).shape == (18, 12)
