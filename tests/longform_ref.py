"""Sequential restatement of the long-form seek loop (openai-whisper's transcribe(), DESIGN.md "Long-form transcription") for
tests/test_gpu_longform.py: one recording after the other, one window per call, through calls that existed before the batched loop --
the front-end on a host-made slice, the encoder, generate_with_fallback(return_timestamps=True, prompt_ids=...) at batch 1.  Written
apart from whisper_trtllm_amd/longform.py on purpose (its own cutting code, its own bookkeeping); it shares only the stated constants.

It also measures how close the batch-1 run's own decisions were: per greedy step the top-2 gap of the processed scores and the gap of
the timestamp rule's comparison (logsumexp of the timestamps against the best text score), per fallback try the distance of
avg_logprob from its threshold.  A test that asserts ids across batch sizes is meaningful only where these are far from a tie."""
import numpy as np
import torch

HOP, SR = 160, 16000


def _margins(cfg, raw, row):
    """`raw` [steps, V]: the raw logits of a greedy decode's steps; `row`: its ids from the start token on.  Returns (smallest top-2 gap
    of the processed scores, smallest |logsumexp(timestamps) - max(text)| where the rule compares them)."""
    from whisper_trtllm_amd.runtime import timestamp_rules
    no_ts, tb, ts_begin, max_init, forced = timestamp_rules(cfg)
    assert not forced
    eos = cfg["eos_token_id"]
    top2, rule5 = np.inf, np.inf
    for step in range(len(row) - 1):
        cur = 1 + step                                    # tokens so far, the start token included
        if cur == ts_begin - 1:                           # the forced <|0.00|>
            continue
        s = torch.from_numpy(np.array(raw[step], dtype=np.float32)).double()
        s[cfg["suppress_tokens"]] = -np.inf
        if cur == 1:
            s[cfg["begin_suppress_tokens"]] = -np.inf
        s[no_ts] = -np.inf
        seq = row[ts_begin:cur]
        last = len(seq) >= 1 and seq[-1] >= tb
        penult = len(seq) < 2 or seq[-2] >= tb
        if last and penult:
            s[tb:] = -np.inf
        elif last:
            s[:eos] = -np.inf
        if cur == ts_begin and max_init >= 0:
            s[tb + max_init + 1:] = -np.inf
        lp = torch.log_softmax(s, -1)
        ts_mass, text_best = torch.logsumexp(lp[tb:], -1).item(), lp[:tb].max().item()
        if np.isfinite(ts_mass) and np.isfinite(text_best):
            rule5 = min(rule5, abs(ts_mass - text_best))
        if ts_mass > text_best:
            s[:tb] = -np.inf
        t2 = torch.topk(s, 2).values
        if torch.isfinite(t2[1]):
            top2 = min(top2, (t2[0] - t2[1]).item())
        assert int(torch.argmax(s)) == row[cur], (step, int(torch.argmax(s)), row[cur])   # the restated rules are the device's
        if row[cur] == eos:
            break
    return top2, rule5


def transcribe_sequential(enc, dec, frontend, audios, *, startofprev, temperatures, compression_ratio_threshold, logprob_threshold,
                          no_speech_threshold, no_speech_token_id, condition_on_previous_text=True, seed=0, margins=False):
    """Returns (segments per file [(start, end, ids, temperature, seek)], windows per file [(seek, prompt_len, kind, temperature, avg_logprob)],
    dict(top2, rule5, avg_gap) of the smallest decision gaps seen)."""
    cfg, info = dec.config, dec.session.info
    from whisper_trtllm_amd.runtime import timestamp_rules
    tb = timestamp_rules(cfg)[1]
    eos = cfg["eos_token_id"]
    S, n_ctx = info.max_source_positions, info.max_target_positions
    N = 2 * S
    tp = N * HOP / SR / S
    stride = N // S
    budget = min(n_ctx // 2, n_ctx - n_ctx // 2 - 1)
    gaps = dict(top2=np.inf, rule5=np.inf, avg_gap=np.inf)
    tries = []
    inner = dec.generate

    def recording_generate(*a, **k):          # every fallback try's avg_logprob, for the distance from the threshold
        out = inner(*a, **k)
        tries.append(float(out[1].avg_logprob[0]))
        return out

    all_segments, all_windows = [], []
    for f, audio in enumerate(audios):
        host = audio.cpu()
        content = host.numel() // HOP
        seek, tokens_all, reset_since = 0, [], 0
        segments, windows = [], []
        while seek < content:
            size = min(N, content - seek)
            t_off = seek * HOP / SR
            piece = host[seek * HOP:seek * HOP + N * HOP].clone().cuda()           # a slice made on the host
            hidden = enc(frontend(piece[None]))
            prev = tokens_all[reset_since:][-(n_ctx // 2 - 1):]
            prompt = [startofprev] + prev if prev else None
            plen = len(prompt) if prompt else 0
            ml = plen + 1 + budget
            trace = torch.full((1, ml - 1, info.vocab_size), float("nan"), device="cuda") if margins else None
            dec.generate = recording_generate
            try:
                ids, sc, used = dec.generate_with_fallback(
                    hidden, temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
                    no_speech_threshold=no_speech_threshold, no_speech_token_id=no_speech_token_id, seeds=[seed + (f << 32) + seek],
                    return_timestamps=True, max_length=ml, **({"prompt_ids": prompt} if prompt else {}),
                    **({"logits_trace": trace} if margins else {}))
            finally:
                del dec.generate
            if logprob_threshold is not None:
                gaps["avg_gap"] = min([gaps["avg_gap"]] + [abs(a - logprob_threshold) for a in tries])
            tries.clear()
            temp = float(used[0])
            row = [int(t) for t in ids[0].cpu().tolist()][plen:]
            toks = row[1:1 + budget]
            if eos in toks:
                toks = toks[:toks.index(eos)]
            if margins and temp == 0.0:
                t2, r5 = _margins(cfg, trace[0].cpu().numpy(), row[:1 + len(toks) + 1])
                gaps["top2"], gaps["rule5"] = min(gaps["top2"], t2), min(gaps["rule5"], r5)
            nsp = float(sc.no_speech_prob[0]) if sc.no_speech_prob is not None else None
            avg = float(sc.avg_logprob[0])
            skip = no_speech_threshold is not None and nsp is not None and nsp > no_speech_threshold
            if skip and logprob_threshold is not None and avg > logprob_threshold:
                skip = False
            if skip:
                windows.append((seek, plen, "skip", temp, avg))
                seek += size
                continue
            is_ts = [t >= tb for t in toks]
            pairs = [i for i in range(1, len(toks)) if is_ts[i - 1] and is_ts[i]]
            closes = len(toks) >= 2 and (not is_ts[-2]) and is_ts[-1]
            new = []
            if pairs:
                cuts = pairs + [len(toks)] if closes else pairs
                at = 0
                for c in cuts:
                    part = toks[at:c]
                    new.append((t_off + (part[0] - tb) * tp, t_off + (part[-1] - tb) * tp, part))
                    at = c
                step, kind = (size, "full") if closes else ((toks[at - 1] - tb) * stride, "cut")
            else:
                span = size * HOP / SR
                stamps = [t for t in toks if t >= tb]
                if stamps and stamps[-1] != tb:
                    span = (stamps[-1] - tb) * tp
                new.append((t_off, t_off + span, toks))
                step, kind = size, "full"
            if step <= 0:
                step, kind = size, "guard"
            for a, b, part in new:
                if a != b and any(t < tb and t != eos for t in part):
                    segments.append((a, b, part, temp, seek))
                    tokens_all += part
            if not condition_on_previous_text or temp > 0.5:
                reset_since = len(tokens_all)
            windows.append((seek, plen, kind, temp, avg))
            seek += step
        all_segments.append(segments)
        all_windows.append(windows)
    return all_segments, all_windows, gaps
