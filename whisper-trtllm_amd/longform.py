"""Long-form transcription: openai-whisper's `transcribe()` seek loop, batched over recordings.

Audio longer than one window is decoded window by window; every window is decoded in timestamp mode and the next one starts at the
last complete timestamp, so no word is cut at a window edge.  Under `condition_on_previous_text` the text decoded so far is the next
window's prompt.  Up to `max_rows` recordings advance side by side: every iteration gathers their current windows into ONE call of the
front-end (`LogMelFrontend.windows`), the encoder and `generate_with_fallback(prompts=...)` -- the rows carry prompts of unequal lengths
(include/whisper_trtllm_amd.h (9h)), a recording that ends hands its row to the next one, which arrives with no prompt.

The host logic is written against an injectable `decode_fn` and needs no GPU:

    decode_fn(requests) -> results
    requests[k] = dict(file, seek, segment_size, prompt, seed)     prompt: [] or [<|startofprev|>, previous tokens ...]
    results[k]  = dict(tokens, temperature, avg_logprob, no_speech_prob, compression_ratio)
                  tokens: the generated ids behind the start and forced tokens, up to but excluding the EOS
    with `languages`: requests[k] also holds language (the recording's language token id, or -1: detect it in this window) and
                  results[k] language, language_prob (the row's language token and its probability among the language ids)

`engine_decode_fn` is the adapter onto the engines.  Stated differences from openai-whisper: every window is normalised on its own (the
reference's WhisperFeatureExtractor per 30 s chunk; openai-whisper takes the whole file's maximum); an advance of 0 frames becomes a
whole window, so the loop always terminates; a window generates at most n_ctx // 2 - 1 - forced tokens (openai-whisper: n_ctx // 2), the
budget that fits behind the longest possible prompt, so that the budget of a row never depends on the prompts decoding beside it.
Languages (multilingual checkpoints): a recording's language is detected in the decode of its FIRST window and kept for every later
one, as openai-whisper does; rows on their first window and rows further along share one decode call (per-row language tokens,
include/whisper_trtllm_amd.h (9i)).  Stated difference: the detection sees the initial prompt when there is one.
Not built: word timestamps across windows, best_of, the hallucination-silence heuristics, beams; text -> ids stays the caller's."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

from .audio import HOP, SAMPLING_RATE

def split_window(tokens: Sequence[int], tb: int, eos: int, seek: int, segment_size: int, tp: float, stride: int):
    """One decoded window -> (segments, advance in frames, advance kind).  `tokens`: the window's generated ids without EOS; `tb`:
    timestamp_begin; `tp`: seconds per timestamp unit; `stride`: frames per timestamp unit.  A segment is (start s, end s, ids); the
    kinds are "cut" (the window is cut at its last pair of consecutive timestamps and the rest is decoded again), "full" (the whole
    window is consumed) and "guard" (a cut that would not advance: the whole window instead).  Segments with start == end or without a
    text token are dropped."""
    tokens = [int(t) for t in tokens]
    time_offset = seek * HOP / SAMPLING_RATE
    ts = [t >= tb for t in tokens]
    single_end = ts[-2:] == [False, True]
    cons = [i for i in range(1, len(tokens)) if ts[i - 1] and ts[i]]
    segments = []
    if cons:
        slices = cons + ([len(tokens)] if single_end else [])
        last = 0
        for cur in slices:
            sl = tokens[last:cur]
            segments.append((time_offset + (sl[0] - tb) * tp, time_offset + (sl[-1] - tb) * tp, sl))
            last = cur
        if single_end:
            advance, kind = segment_size, "full"
        else:   # the tokens behind the last cut are dropped: the next window decodes them again
            advance, kind = (tokens[last - 1] - tb) * stride, "cut"
    else:
        duration = segment_size * HOP / SAMPLING_RATE
        stamps = [t for t in tokens if t >= tb]
        if stamps and stamps[-1] != tb:
            duration = (stamps[-1] - tb) * tp
        segments.append((time_offset, time_offset + duration, tokens))
        advance, kind = segment_size, "full"
    if advance <= 0:
        advance, kind = segment_size, "guard"
    segments = [s for s in segments if s[0] != s[1] and any(t < tb and t != eos for t in s[2])]
    return segments, advance, kind


class _File:
    def __init__(self, index: int, content_frames: int, initial: Sequence[int]):
        self.index, self.content_frames = index, int(content_frames)
        self.seek, self.all_tokens, self.prompt_reset_since = 0, [int(t) for t in initial], 0
        self.segments: List[dict] = []
        self.language, self.language_prob = -1, None      # language token id (-1: not known yet) and its probability where it was detected


def transcribe(decode_fn: Callable, content_frames: Sequence[int], *, n_ctx: int, max_source_positions: int, timestamp_begin: int,
               eos_token_id: int, startofprev_token_id: int, initial_prompt_ids: Optional[Sequence[int]] = None,
               condition_on_previous_text: bool = True, no_speech_threshold: Optional[float] = 0.6,
               logprob_threshold: Optional[float] = -1.0, max_rows: int = 8, seed: int = 0, trace: bool = False,
               languages: Optional[Sequence[int]] = None):
    """The seek loop over recordings of `content_frames[f]` mel frames each.  Returns per recording the list of segments
    dict(start, end, ids, temperature, avg_logprob, no_speech_prob, compression_ratio, seek); with `trace` also the list of windows
    (file, seek, prompt_len, advance_kind, temperature) in the order they were decoded ("skip": a no-speech window).  The result of
    a recording does not depend on `max_rows` or on what decodes beside it.
    `languages`: per recording its language token id, or -1 to detect it on the recording's first window; the result then ends with the
    list of dict(language, language_prob) per recording (language_prob None where the caller chose the language; a recording without
    audio keeps language -1)."""
    if not isinstance(max_rows, int) or not 1 <= max_rows <= 16:
        raise ValueError(f"max_rows must be an integer in [1, 16], got {max_rows!r}")
    N = 2 * max_source_positions                                  # window, frames
    stride = N // max_source_positions                            # frames per timestamp unit
    tp = N * HOP / SAMPLING_RATE / max_source_positions           # seconds per timestamp unit
    tb, keep = int(timestamp_begin), n_ctx // 2 - 1
    files = [_File(f, n, initial_prompt_ids or ()) for f, n in enumerate(content_frames)]
    if languages is not None:
        if len(languages) != len(files):
            raise ValueError(f"languages has {len(languages)} entries for {len(files)} recordings")
        for f, lang in zip(files, languages):
            f.language = int(lang) if int(lang) >= 0 else -1
    waiting = [f for f in files if f.content_frames > 0]
    active: List[_File] = []
    windows = []
    while waiting or active:
        while waiting and len(active) < max_rows:                 # a row that fell free goes to the next recording
            active.append(waiting.pop(0))
        requests = []
        for f in active:
            prev = f.all_tokens[f.prompt_reset_since:][-keep:]
            requests.append(dict(file=f.index, seek=f.seek, segment_size=min(N, f.content_frames - f.seek),
                                 prompt=[int(startofprev_token_id)] + prev if prev else [], seed=int(seed) + (f.index << 32) + f.seek))
            if languages is not None:
                requests[-1]["language"] = f.language
        results = decode_fn(requests)
        if len(results) != len(requests):
            raise RuntimeError(f"decode_fn returned {len(results)} results for {len(requests)} windows")
        for f, rq, r in zip(list(active), requests, results):
            size, temperature = rq["segment_size"], float(r["temperature"])
            if languages is not None and f.language < 0:          # the recording's first window: its language, kept from here on
                f.language, f.language_prob = int(r["language"]), float(r["language_prob"])
            skip = False
            if no_speech_threshold is not None and r.get("no_speech_prob") is not None:
                skip = r["no_speech_prob"] > no_speech_threshold
                if logprob_threshold is not None and r["avg_logprob"] > logprob_threshold:
                    skip = False
            if skip:
                advance, kind = size, "skip"
            else:
                segments, advance, kind = split_window(r["tokens"], tb, eos_token_id, f.seek, size, tp, stride)
                for start, end, ids in segments:
                    f.segments.append(dict(start=start, end=end, ids=ids, temperature=temperature, avg_logprob=r["avg_logprob"],
                                           no_speech_prob=r.get("no_speech_prob"), compression_ratio=r.get("compression_ratio"), seek=f.seek))
                    f.all_tokens.extend(ids)
                if not condition_on_previous_text or temperature > 0.5:
                    f.prompt_reset_since = len(f.all_tokens)
            windows.append((f.index, f.seek, len(rq["prompt"]), kind, temperature))
            f.seek += advance
            if f.seek >= f.content_frames:
                active.remove(f)
    out = [f.segments for f in files]
    if languages is not None:
        langs = [dict(language=f.language, language_prob=f.language_prob) for f in files]
        return (out, windows, langs) if trace else (out, langs)
    return (out, windows) if trace else out


def generation_budget(n_ctx: int, n_forced: int) -> int:
    """Generated tokens per window (start and forced tokens not counted): what fits behind the longest prompt, n_ctx // 2 of
    <|startofprev|> + text, the start token and the forced tokens -- at most openai-whisper's n_ctx // 2."""
    return min(n_ctx // 2, n_ctx - n_ctx // 2 - 1 - n_forced)


def engine_decode_fn(enc, dec, frontend, audio_flat, file_offsets: Sequence[int], file_samples: Sequence[int], *,
                     temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold: Optional[float] = 2.4,
                     logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6, no_speech_token_id=None,
                     text_of=None, task=None):
    """`decode_fn` over the engines: recording f is samples [file_offsets[f], file_offsets[f] + file_samples[f]) of the flat GPU buffer;
    all windows of a call go through one front-end call, one encoder call and one generate_with_fallback(prompts=...).  Requests that
    carry `language` decode with per-row language tokens (-1: detected in that call); `task`: see `generate`."""
    from .runtime import _default_text_of, strip_prompts, timestamp_rules
    from .text import compression_ratio
    info = dec.session.info
    N = 2 * info.max_source_positions
    if getattr(frontend, "n_frames", None) != N:
        raise ValueError(f"the front-end handle must be created for the model's window: LogMelFrontend(n_frames={N}), got "
                         f"{getattr(frontend, 'n_frames', None)}")
    n_ctx, eos = info.max_target_positions, dec.config["eos_token_id"]
    n_forced = len(timestamp_rules(dec.config)[4])     # the forced list without <|notimestamps|>
    budget = generation_budget(n_ctx, n_forced)
    if budget < 1:
        raise ValueError(f"max_target_positions {n_ctx} leaves no room to generate behind a prompt and {n_forced} forced tokens")
    text_of = text_of or _default_text_of(dec.config)

    def decode(requests):
        offsets = [file_offsets[r["file"]] + r["seek"] * HOP for r in requests]
        n_valid = [min(N * HOP, file_samples[r["file"]] - r["seek"] * HOP) for r in requests]
        hidden = enc(frontend.windows(audio_flat, offsets, n_valid))
        prompts = [r["prompt"] for r in requests]
        lmax = max(len(p) for p in prompts)
        lk = {}
        if "language" in requests[0]:
            lk["language"] = [r["language"] if r["language"] >= 0 else "auto" for r in requests]
        if task is not None:
            lk["task"] = task
        ids, scores, temps, *langs = dec.generate_with_fallback(
            hidden, temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
            no_speech_threshold=no_speech_threshold, no_speech_token_id=no_speech_token_id, text_of=text_of,
            seeds=[r["seed"] for r in requests], return_timestamps=True, max_length=lmax + 1 + n_forced + budget, prompts=prompts, **lk)
        lang_ids = langs[0].ids.cpu().tolist() if langs else None
        lang_prob = langs[0].prob_of_ids().cpu().tolist() if langs else None
        avg = scores.avg_logprob.cpu().tolist()
        nsp = scores.no_speech_prob.cpu().tolist() if scores.no_speech_prob is not None else [None] * len(requests)
        temps = temps.cpu().tolist()
        out = []
        for k, row in enumerate(strip_prompts(ids.cpu(), lmax)):
            tokens = row[1 + n_forced:1 + n_forced + budget]
            if eos in tokens:
                tokens = tokens[:tokens.index(eos)]
            text = text_of(tokens)
            out.append(dict(tokens=tokens, temperature=temps[k], avg_logprob=avg[k], no_speech_prob=nsp[k],
                            compression_ratio=compression_ratio(text) if text else 0.0))
            if langs:
                out[-1].update(language=lang_ids[k], language_prob=lang_prob[k])
        return out

    return decode


def transcribe_long(enc, dec, frontend, audios, *, initial_prompt_ids=None, condition_on_previous_text: bool = True,
                    temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold: Optional[float] = 2.4,
                    logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6, no_speech_token_id=None,
                    startofprev_token_id=None, text_of=None, max_rows: int = 8, seed: int = 0, trace: bool = False, language=None, task=None):
    """Transcribe recordings of any length: `audios` is a list of 1-D float32 GPU tensors (16 kHz mono).  See `transcribe` for the
    result.  `language` (multilingual configs; see `generate`): "auto" detects every recording's language on its first window and keeps
    it; an id / code / token sets it; a list gives one of those per recording.  The result then ends with the recordings' dict(language,
    language_prob).  `task`: "transcribe" / "translate" or a token id.  `startofprev_token_id` defaults to the config's, or to where Whisper's vocabularies put it: <|startofprev|>,
    <|nospeech|>, <|notimestamps|> are consecutive ids, and <|notimestamps|> is the config's forced token.
    fp32 decoder engines."""
    import torch
    from .runtime import resolve_languages, resolve_task, timestamp_rules
    languages = None
    if language is not None:
        languages = resolve_languages(dec.config, language, len(audios))[1]
    if task is not None:
        resolve_task(dec.config, task)
    if not audios:
        empty = ([], []) if trace else []
        return (empty + ([],) if trace else ([], [])) if language is not None else empty
    for a in audios:
        if a.dim() != 1 or a.dtype != torch.float32 or not a.is_cuda:
            raise ValueError("audios must be 1-D float32 CUDA tensors")
    no_ts, tb = timestamp_rules(dec.config)[:2]
    if startofprev_token_id is None:
        startofprev_token_id = dec.config.get("startofprev_token_id", no_ts - 2)
    samples = [int(a.numel()) for a in audios]
    offsets = [sum(samples[:f]) for f in range(len(samples))]
    flat = audios[0] if len(audios) == 1 else torch.cat(list(audios))
    fn = engine_decode_fn(enc, dec, frontend, flat, offsets, samples, temperatures=temperatures,
                          compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
                          no_speech_threshold=no_speech_threshold, no_speech_token_id=no_speech_token_id, text_of=text_of, task=task)
    info = dec.session.info
    return transcribe(fn, [n // HOP for n in samples], n_ctx=info.max_target_positions, max_source_positions=info.max_source_positions,
                      timestamp_begin=tb, eos_token_id=dec.config["eos_token_id"], startofprev_token_id=startofprev_token_id,
                      initial_prompt_ids=initial_prompt_ids, condition_on_previous_text=condition_on_previous_text,
                      no_speech_threshold=no_speech_threshold, logprob_threshold=logprob_threshold, max_rows=max_rows, seed=seed, trace=trace,
                      languages=languages)
