#!/usr/bin/env python3
"""Golden vectors of language detection and per-row language tokens from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_language.py [case ...]   (no case = all)
Every case is a synthetic config with a multilingual-shaped forced list [[1, L0], [2, task], [3, <|notimestamps|>]] and 5-9
`language_ids` scattered through the vocabulary (one of them a suppressed id where the config has one in reach: the suppress lists do
not apply to the detection).  Recorded per case (tests/golden/<case>.npz):
  * openai-whisper's detect_language restated on the reference model: the raw logits of the step whose input is the start token alone,
    at the language ids, in float64; their softmax; the argmax (a language id per row);
  * per row, the reference's `greedy_search` at BATCH 1 with that row's detected language in the forced list (the timestamp-mode list of
    make_golden_logprobs.py for the lg-ts case), and its transition scores taken as make_golden_logprobs.py takes them.
A seed is kept only if every language top-2 margin and every decode-step top-2 margin is >= 1e-3 (tests/golden/find_healthy_seeds.py's
criterion) and the rows of the batch do not all detect the same language; the script walks the seeds from the case's first one."""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import build_hf, import_reference_hf  # noqa: E402

CASES = [  # (case, config, first seed, batch, config overrides, timestamp mode)
    ("lg-tiny_b2", "whisper-tiny.en", 40, 2,
     {"max_length": 20, "forced_decoder_ids": [[1, 50259], [2, 50358], [3, 50362]],
      "language_ids": [50330, 311, 50259, 50357, 20000, 50263, 7203]}, False),
    ("lg-toy-short_b3", "toy-short", 40, 3,
     {"forced_decoder_ids": [[1, 130], [2, 505], [3, 510]], "language_ids": [402, 3, 130, 511, 0, 256, 77, 7, 311]}, False),
    ("lg-ts-toy_b3", "toy-ts", 40, 3,
     {"max_length": 32, "forced_decoder_ids": [[1, 130], [2, 498], [3, 502]], "language_ids": [402, 3, 130, 499, 256, 77]}, True),
]


def decode_row(model, cfg, enc_row, forced, max_length, BaseModelOutput, ts_mode):
    """greedy_search at batch 1 under `forced`: (ids [len], transition scores [len - 1], top-2 margins [len - 1])."""
    from transformers.generation.logits_process import (ForceTokensLogitsProcessor, LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    top2, scores_tuple = [], []

    class Top2:  # last in the list: the processed scores (greedy_search's output_scores tuple) and the margin of their argmax
        def __call__(self, input_ids, scores):
            scores_tuple.append(scores.detach().clone())
            t2 = torch.topk(scores.double(), 2, dim=-1).values
            top2.append(torch.where(torch.isinf(t2[:, 1]), torch.full_like(t2[:, 0], np.inf), t2[:, 0] - t2[:, 1]).numpy())
            return scores

    if ts_mode:   # <|notimestamps|> leaves the prompt; the language and the task stay forced in front of the forced <|0.00|>
        no_ts = forced[-1][1]
        kept = forced[:-1]
        gc = types.SimpleNamespace(eos_token_id=cfg["eos_token_id"], no_timestamps_token_id=no_ts, forced_decoder_ids=forced,
                                   max_initial_timestamp_index=1)
        procs = [SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1 + kept[-1][0]), ForceTokensLogitsProcessor(kept),
                 WhisperTimeStampLogitsProcessor(gc), Top2()]
    else:
        procs = [SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1 + forced[-1][0]), ForceTokensLogitsProcessor(forced), Top2()]
    ids = torch.full((1, 1), cfg["decoder_start_token_id"], dtype=torch.long)
    with contextlib.redirect_stdout(io.StringIO()):
        out = model.greedy_search(ids, logits_processor=LogitsProcessorList(procs),
                                  stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]),
                                  pad_token_id=cfg["pad_token_id"], eos_token_id=cfg["eos_token_id"],
                                  encoder_outputs=BaseModelOutput(last_hidden_state=enc_row), use_cache=True,
                                  output_scores=True, return_dict_in_generate=True)
        assert torch.is_tensor(out), "this greedy_search returns scores itself: use out.sequences / out.scores"
        trans = model.compute_transition_scores(out, tuple(scores_tuple), normalize_logits=True)
    return out[0].numpy().astype(np.int64), trans[0].numpy().astype(np.float32), np.stack(top2, 1)[0]


def record(model, cfg, enc_out, B, BaseModelOutput, ts_mode):
    """None for an unhealthy seed, else the arrays of the case."""
    lang_ids, forced, max_length, eos = cfg["language_ids"], cfg["forced_decoder_ids"], cfg["max_length"], cfg["eos_token_id"]
    start = torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)
    hidden = model.model.decoder(input_ids=start, encoder_hidden_states=enc_out).last_hidden_state
    logits = model.proj_out(hidden)[:, 0].double().numpy()[:, lang_ids]          # detect_language: the start token alone
    z = logits - logits.max(-1, keepdims=True)
    probs = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    order = np.sort(logits, -1)
    margin = order[:, -1] - order[:, -2]
    detected = np.asarray(lang_ids)[logits.argmax(-1)]
    if margin.min() < 1e-3 or len(set(detected.tolist())) < 2:
        return None
    rows = []
    for b in range(B):
        row_forced = [[1, int(detected[b])]] + [list(p) for p in forced[1:]]
        ids, trans, top2 = decode_row(model, cfg, enc_out[b:b + 1], row_forced, max_length, BaseModelOutput, ts_mode)
        hit = np.nonzero(ids[1:] == eos)[0]
        live = top2[:hit[0] + 1] if hit.size else top2      # a row's decisions count up to its EOS
        if live.min() < 1e-3:
            return None
        rows.append((ids, trans, top2))
    width = max(len(r[0]) for r in rows)
    ids = np.full((B, width), cfg["pad_token_id"], dtype=np.int64)
    trans = np.zeros((B, width - 1), dtype=np.float32)
    top2 = np.full((B, width - 1), np.inf)
    for b, (i, t, m) in enumerate(rows):
        ids[b, :len(i)], trans[b, :len(t)], top2[b, :len(m)] = i, t, m
    return {"lang_logits": logits, "lang_probs": probs, "lang_margin": margin, "lang_detected": detected.astype(np.int64), "ids": ids,
            "row_len": np.asarray([len(r[0]) for r in rows], dtype=np.int64), "token_logprobs": trans, "top2_margin": top2}


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    from whisper_trtllm_amd import synthetic
    WhisperConfig, Model, BaseModelOutput = import_reference_hf()
    only = set(sys.argv[1:])
    for case, cname, seed0, B, overrides, ts_mode in CASES:
        if only and case not in only:
            continue
        cfg = synthetic.get_config(cname)
        cfg.update(overrides)
        for seed in range(seed0, seed0 + 64):
            weights = synthetic.make_weights(cfg, seed)
            mel = synthetic.make_mel(cfg, index=7 * seed, batch=B)
            model = build_hf(cfg, weights, WhisperConfig, Model)
            with torch.no_grad():
                enc_out = model.model.encoder(torch.from_numpy(mel)).last_hidden_state
                got = record(model, cfg, enc_out, B, BaseModelOutput, ts_mode)
            if got is not None:
                break
            print(f"[{case}] seed {seed}: unhealthy (a margin under 1e-3, or one language for every row)")
        else:
            raise SystemExit(f"[{case}] no healthy seed in [{seed0}, {seed0 + 64})")
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed, "overrides_json": json.dumps(overrides),
               "timestamp_mode": int(ts_mode), "language_ids": np.asarray(cfg["language_ids"], dtype=np.int64), **got}
        print(f"[{case}] seed {seed} | detected {got['lang_detected'].tolist()} | min language margin {got['lang_margin'].min():.3e} | "
              f"min step margin {got['top2_margin'].min():.3e}")
        for r, p in zip(got["ids"], got["lang_probs"]):
            print("   ", r.tolist())
            print("   ", np.round(p, 4).tolist())
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
