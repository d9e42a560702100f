#!/usr/bin/env python3
"""Golden vectors of the token log-probabilities from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_logprobs.py [case ...]   (no case = all)
The reference's `greedy_search` is called directly with the processor list generate() builds -- SuppressTokens,
SuppressTokensAtBegin, ForceTokens, and for the lp-ts case the timestamp-mode list of make_golden_timestamps.py.  The bundled
greedy_search is cut down to the id loop: it accepts output_scores / return_dict_in_generate and ignores them, returning ids
alone.  So the tuple it would have collected -- the processed scores of every step, `next_tokens_scores` -- is taken by a last
entry of the processor list, and handed to the reference's own compute_transition_scores.  Recorded per case (tests/golden/<case>.npz): ids, compute_transition_scores(sequences, scores,
normalize_logits=True) (the log-probability of every generated token under the processed scores of its step; what the reference
leaves at pad positions behind an EOS is recorded as it comes and not compared), softmax(raw logits of step 0)[no_speech id] in
float64, and the top-2 margin of the processed scores per step.  A seed is kept only if no margin is under 1e-3
(tests/golden/find_healthy_seeds.py's criterion).  lp-tiny_b2 shares weights and mels with tiny_b2."""
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

CASES = [  # (case, config, weight seed, batch, config overrides, timestamp mode, no_speech id)
    ("lp-tiny_b2", "whisper-tiny.en", 14, 2, {"max_length": 24}, False, 50361),
    # random weights never pick the one EOS id: EOS (= pad, as in the .en models) is remapped onto a text token the decode emits, so two
    # rows stop early and one runs to max_length
    ("lp-toy-short_b3", "toy-short", 11, 3, {"eos_token_id": 392, "pad_token_id": 392}, False, 7),
    ("lp-ts-toy_b3", "toy-ts", 32, 3, {"eos_token_id": 81, "pad_token_id": 81}, True, 7),
]


def record(model, cfg, enc_out, B, max_length, BaseModelOutput, ts_mode):
    from transformers.generation.logits_process import (ForceTokensLogitsProcessor, LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    raw, top2 = [], []

    class Raw:   # first in the list: the raw logits of the step
        def __call__(self, input_ids, scores):
            raw.append(scores.detach().clone().double().numpy())
            return scores

    scores_tuple = []

    class Top2:  # last in the list: the processed scores (greedy_search's output_scores tuple) and the margin of their argmax
        def __call__(self, input_ids, scores):
            scores_tuple.append(scores.detach().clone())
            t2 = torch.topk(scores.double(), 2, dim=-1).values
            top2.append(torch.where(torch.isinf(t2[:, 1]), torch.full_like(t2[:, 0], np.inf), t2[:, 0] - t2[:, 1]).numpy())
            return scores

    forced = cfg["forced_decoder_ids"]
    if ts_mode:   # make_golden_timestamps.py: <|notimestamps|> leaves the prompt, SuppressTokensAtBegin starts behind the start token
        no_ts = forced[-1][1]
        gc = types.SimpleNamespace(eos_token_id=cfg["eos_token_id"], no_timestamps_token_id=no_ts, forced_decoder_ids=[[1, no_ts]],
                                   max_initial_timestamp_index=1)
        procs = [Raw(), SuppressTokensLogitsProcessor(cfg["suppress_tokens"]), SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1),
                 WhisperTimeStampLogitsProcessor(gc), Top2()]
    else:         # generate()'s list: begin_index = prompt length + the last forced position (generation/utils.py:943)
        procs = [Raw(), SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1 + forced[-1][0]), ForceTokensLogitsProcessor(forced), Top2()]
    ids = torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)
    with contextlib.redirect_stdout(io.StringIO()):
        out = model.greedy_search(ids, logits_processor=LogitsProcessorList(procs),
                                  stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]),
                                  pad_token_id=cfg["pad_token_id"], eos_token_id=cfg["eos_token_id"],
                                  encoder_outputs=BaseModelOutput(last_hidden_state=enc_out), use_cache=True,
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
    for case, cname, seed, B, overrides, ts_mode, ns in CASES:
        if only and case not in only:
            continue
        cfg = synthetic.get_config(cname)
        cfg.update(overrides)
        max_length = cfg["max_length"]
        weights = synthetic.make_weights(cfg, seed)
        mel = synthetic.make_mel(cfg, index=7 * seed, batch=B)
        model = build_hf(cfg, weights, WhisperConfig, Model)
        with torch.no_grad():
            enc_out = model.model.encoder(torch.from_numpy(mel)).last_hidden_state
            ids, trans, raw0, top2 = record(model, cfg, enc_out, B, max_length, BaseModelOutput, ts_mode)
        ids = ids.numpy().astype(np.int64)
        z = raw0 - raw0.max(-1, keepdims=True)
        nsp = np.exp(z[:, ns]) / np.exp(z).sum(-1)
        # a row's decisions count up to its EOS: behind it the reference writes pad whatever the scores say
        eos = cfg["eos_token_id"]
        live = np.ones(top2.shape, dtype=bool)
        for b in range(B):
            hit = np.nonzero(ids[b, 1:] == eos)[0]
            if hit.size:
                live[b, hit[0] + 1:] = False
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed, "overrides_json": json.dumps(overrides),
               "timestamp_mode": int(ts_mode), "no_speech_token_id": ns, "ids": ids,
               "token_logprobs": trans.numpy().astype(np.float32), "no_speech_prob": nsp.astype(np.float64), "top2_margin": top2}
        print(f"[{case}] ids {ids.shape} eos rows {int((ids[:, 1:] == eos).any(1).sum())} | min top-2 {top2[live].min():.3e} | "
              f"no_speech_prob {nsp}")
        for r, t in zip(ids, trans.numpy()):
            print("   ", r.tolist())
            print("   ", np.round(t, 3).tolist())
        assert top2[live].min() >= 1e-3, "unhealthy seed: pick another"
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
