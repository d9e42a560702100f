"""Sequential restatement of the long-form loop WITH languages (DESIGN.md "Language detection"), for tests/test_gpu_language.py, in the
manner of tests/longform_ref.py: one recording after the other, one window per call, at batch 1.  The language of a recording is
detected on its first window (`detect_language`: one decoder step from the start token) and every window is then decoded through the
path that existed before per-row languages: an engine view whose CONFIG carries that language at forced position 1
(generate_with_fallback(return_timestamps=True, prompt_ids=...)).  Own cutting code and bookkeeping; it shares only the stated constants.
The no-speech skip is not restated: the test runs without a no-speech token."""
import torch

HOP, SR = 160, 16000


def language_view(wt, dec, lang):
    """`dec`'s engine under a config whose forced list holds `lang` at position 1: the batch-wide forced id of the path before."""
    forced = [[1, int(lang)]] + [list(p) for p in dec.config["forced_decoder_ids"][1:]]
    return wt.WhisperDecoderEngine(None, dict(dec.config, forced_decoder_ids=forced), _session=dec.session)


def transcribe_sequential(wt, enc, dec, frontend, audios, *, startofprev, temperatures, compression_ratio_threshold, logprob_threshold,
                          no_speech_threshold, no_speech_token_id, seed=0):
    """Returns (segments per file [(start, end, ids, temperature, seek)], windows per file [(seek, prompt_len, kind, temperature)],
    languages per file [(language token, its probability)])."""
    from whisper_trtllm_amd.runtime import timestamp_rules
    cfg, info = dec.config, dec.session.info
    _no_ts, tb, _begin, _max_init, kept = timestamp_rules(cfg)
    n_forced, eos = len(kept), cfg["eos_token_id"]
    S, n_ctx = info.max_source_positions, info.max_target_positions
    N = 2 * S
    tp, stride = N * HOP / SR / S, N // S
    budget = min(n_ctx // 2, n_ctx - n_ctx // 2 - 1 - n_forced)
    all_segments, all_windows, languages = [], [], []
    for f, audio in enumerate(audios):
        host = audio.cpu()
        content = host.numel() // HOP
        seek, history, since = 0, [], 0
        segments, windows, lang, view = [], [], None, None
        while seek < content:
            size = min(N, content - seek)
            hidden = enc(frontend(host[seek * HOP:seek * HOP + N * HOP].clone().cuda()[None]))
            if lang is None:                                   # the first window names the recording's language
                toks, probs = dec.detect_language(hidden)
                lang = (int(toks[0]), float(probs[0].max()))
                view = language_view(wt, dec, lang[0])
            prev = history[since:][-(n_ctx // 2 - 1):]
            prompt = [startofprev] + prev if prev else None
            plen = len(prompt) if prompt else 0
            ids, _sc, used = view.generate_with_fallback(
                hidden, temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
                no_speech_threshold=no_speech_threshold, no_speech_token_id=no_speech_token_id, seeds=[seed + (f << 32) + seek],
                return_timestamps=True, max_length=plen + 1 + n_forced + budget, **({"prompt_ids": prompt} if prompt else {}))
            temp = float(used[0])
            row = [int(t) for t in ids[0].cpu().tolist()][plen:]
            assert row[1] == lang[0]
            toks = row[1 + n_forced:1 + n_forced + budget]
            if eos in toks:
                toks = toks[:toks.index(eos)]
            t0 = seek * HOP / SR
            stamp = [t >= tb for t in toks]
            doubles = [i for i in range(1, len(toks)) if stamp[i - 1] and stamp[i]]
            closed = len(toks) >= 2 and stamp[-1] and not stamp[-2]
            found = []
            if doubles:
                at = 0
                for c in doubles + ([len(toks)] if closed else []):
                    found.append((t0 + (toks[at] - tb) * tp, t0 + (toks[c - 1] - tb) * tp, toks[at:c]))
                    at = c
                step, kind = (size, "full") if closed else ((toks[at - 1] - tb) * stride, "cut")
            else:
                marks = [t for t in toks if t >= tb]
                span = (marks[-1] - tb) * tp if marks and marks[-1] != tb else size * HOP / SR
                found.append((t0, t0 + span, toks))
                step, kind = size, "full"
            if step <= 0:
                step, kind = size, "guard"
            for a, b, part in found:
                if a != b and any(t < tb and t != eos for t in part):
                    segments.append((a, b, part, temp, seek))
                    history += part
            if temp > 0.5:
                since = len(history)
            windows.append((seek, plen, kind, temp))
            seek += step
        all_segments.append(segments)
        all_windows.append(windows)
        languages.append(lang)
    return all_segments, all_windows, languages
