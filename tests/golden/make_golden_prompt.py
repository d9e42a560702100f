#!/usr/bin/env python3
"""Golden vectors of decodes behind a decoder prompt, from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prompt.py [case ...]   (no case = all)
The reference's `greedy_search` is called with multi-token input_ids = [prompt..., start] per row and the prompt's keys and values as
`past_key_values`, which the reference's own model computes one position at a time.  The bundled model cannot take the prompt in one
forward: its WhisperDecoder builds the causal mask (_prepare_decoder_attention_mask) but hands `attention_mask=None` to every layer, and
its attention has no mask term, so a multi-token forward lets every prompt position see the later ones -- not what Whisper computes.  A
position fed alone sees exactly its past, which is the causal result.  (The one-pass causal forward the prefill is checked against is
tests/prompt_ref.py, in fp64.)  The processor list is the one
of make_golden_logprobs.py with every position moved behind the prompt: SuppressTokensAtBegin at len(input_ids) + the last forced
position, the forced pairs shifted by the prompt length, the timestamp rule's begin_index likewise.  Recorded per case
(tests/golden/pr-*.npz): the prompt, the ids (prompt included), the top-2 margin of the processed scores per step and -- for
pr-toy-short_b3 -- compute_transition_scores(normalize_logits=True) and softmax(raw logits of the first step)[no_speech id].  A seed is
kept only if no margin of a live decision is under 1e-3 (tests/golden/find_healthy_seeds.py's criterion).

Smallest kept margins: pr-toy-short_b3 4.9e-03, pr-tiny_b2 1.5e-02, pr-ts-toy_b3 1.9e-02, pr-toy-long_b2 1.4e-02."""
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

CASES = [  # (case, config, weight seed, batch, config overrides, prompt length, one prompt per row, timestamp mode, <|startofprev|>, no_speech id)
    # EOS (= pad) remapped onto a text token this decode emits (the remapping of lp-toy-short_b3): one row stops early, the others run to max_length
    ("pr-toy-short_b3", "toy-short", 11, 3, {"eos_token_id": 432, "pad_token_id": 432}, 7, True, False, 507, 7),
    ("pr-tiny_b2", "whisper-tiny.en", 14, 2, {"max_length": 36}, 12, False, False, 50360, None),
    ("pr-ts-toy_b3", "toy-ts", 32, 3, {}, 9, False, True, 499, None),
    # 130 prompt positions: two 128-query blocks and three 64-key tiles of the prefill attention
    ("pr-toy-long_b2", "toy-short", 11, 2, {"max_target_positions": 160, "max_length": 150}, 130, True, False, 507, None),
]


def make_prompt(cfg, seed, rows, n, sop):
    """<|startofprev|> and n - 1 text ids below the config's specials, one row per utterance (or one shared row)."""
    rng = np.random.default_rng(1000 + seed)
    hi = min(cfg["decoder_start_token_id"], cfg["eos_token_id"], sop) - 1
    banned = set(cfg["suppress_tokens"]) | set(cfg["begin_suppress_tokens"]) | {cfg["eos_token_id"], cfg["pad_token_id"]}
    ok = np.array([t for t in range(3, hi) if t not in banned])
    return np.stack([np.concatenate([[sop], rng.choice(ok, n - 1)]) for _ in range(rows)]).astype(np.int64)


def record(model, cfg, enc_out, prompt, max_length, BaseModelOutput, ts_mode):
    from transformers.generation.logits_process import (ForceTokensLogitsProcessor, LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    B, n = prompt.shape
    raw, top2, scores_tuple = [], [], []

    class Raw:
        def __call__(self, input_ids, scores):
            raw.append(scores.detach().clone().double().numpy())
            return scores

    class Top2:
        def __call__(self, input_ids, scores):
            scores_tuple.append(scores.detach().clone())
            t2 = torch.topk(scores.double(), 2, dim=-1).values
            top2.append(torch.where(torch.isinf(t2[:, 1]), torch.full_like(t2[:, 0], np.inf), t2[:, 0] - t2[:, 1]).numpy())
            return scores

    forced = cfg["forced_decoder_ids"]
    if ts_mode:
        no_ts = forced[-1][1]
        gc = types.SimpleNamespace(eos_token_id=cfg["eos_token_id"], no_timestamps_token_id=no_ts, forced_decoder_ids=[[1, no_ts]],
                                   max_initial_timestamp_index=1)
        ts = WhisperTimeStampLogitsProcessor(gc)
        ts.begin_index += n
        procs = [Raw(), SuppressTokensLogitsProcessor(cfg["suppress_tokens"]), SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], n + 1),
                 ts, Top2()]
    else:
        procs = [Raw(), SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], n + 1 + forced[-1][0]),
                 ForceTokensLogitsProcessor([[pos + n, tok] for pos, tok in forced]), Top2()]
    ids = torch.cat([torch.from_numpy(prompt), torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)], 1)
    eo, past = BaseModelOutput(last_hidden_state=enc_out), None
    for t in range(n):   # the prompt through the reference's model, one position at a time (see the module docstring)
        past = model(encoder_outputs=eo, decoder_input_ids=ids[:, t:t + 1], past_key_values=past, use_cache=True).past_key_values
    with contextlib.redirect_stdout(io.StringIO()):
        out = model.greedy_search(ids, logits_processor=LogitsProcessorList(procs),
                                  stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]),
                                  pad_token_id=cfg["pad_token_id"], eos_token_id=cfg["eos_token_id"],
                                  encoder_outputs=eo, past_key_values=past, use_cache=True,
                                  output_scores=True, return_dict_in_generate=True)
        assert torch.is_tensor(out), "this greedy_search returns scores itself: use out.sequences / out.scores"
        trans = model.compute_transition_scores(out, tuple(scores_tuple), normalize_logits=True)
    return out, trans, raw[0], np.stack(top2, 1)


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    from whisper_trtllm_amd import synthetic
    WhisperConfig, Model, BaseModelOutput = import_reference_hf()
    only = set(sys.argv[1:])
    for case, cname, seed, B, overrides, n, per_row, ts_mode, sop, ns in CASES:
        if only and case not in only:
            continue
        cfg = synthetic.get_config(cname)
        cfg.update(overrides)
        weights = synthetic.make_weights(cfg, seed)
        mel = synthetic.make_mel(cfg, index=7 * seed, batch=B)
        model = build_hf(cfg, weights, WhisperConfig, Model)
        prompt = make_prompt(cfg, seed, B if per_row else 1, n, sop)
        with torch.no_grad():
            enc_out = model.model.encoder(torch.from_numpy(mel)).last_hidden_state
            ids, trans, raw0, top2 = record(model, cfg, enc_out, np.repeat(prompt, B // prompt.shape[0], 0), cfg["max_length"], BaseModelOutput, ts_mode)
        ids = ids.numpy().astype(np.int64)
        eos = cfg["eos_token_id"]
        live = np.ones(top2.shape, dtype=bool)   # a row's decisions count up to its EOS
        for b in range(B):
            hit = np.nonzero(ids[b, n + 1:] == eos)[0]
            if hit.size:
                live[b, hit[0] + 1:] = False
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed, "overrides_json": json.dumps(overrides),
               "timestamp_mode": int(ts_mode), "prompt": prompt, "ids": ids, "top2_margin": top2}
        if ns is not None:
            z = raw0 - raw0.max(-1, keepdims=True)
            out.update(no_speech_token_id=ns, no_speech_prob=(np.exp(z[:, ns]) / np.exp(z).sum(-1)).astype(np.float64),
                       token_logprobs=trans.numpy().astype(np.float32))
        print(f"[{case}] prompt {prompt.shape} ids {ids.shape} eos rows {int((ids[:, n + 1:] == eos).any(1).sum())} | min top-2 {top2[live].min():.3e}")
        for r in ids:
            print("   ", r[n:].tolist())
        assert top2[live].min() >= 1e-3, "unhealthy seed: pick another"
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
