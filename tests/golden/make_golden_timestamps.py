#!/usr/bin/env python3
"""Golden vectors of Whisper's timestamp mode from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_timestamps.py [case ...]   (no case = all)
The reference's generate() hard-wires return_timestamps=False and ignores custom processors, so its `greedy_search` is called
directly with the processor list generate() would build in timestamp mode: SuppressTokens, SuppressTokensAtBegin(begin_index 1:
the prompt is the start token alone) and WhisperTimeStampLogitsProcessor (forced_decoder_ids [[1, <|notimestamps|>]] ->
begin_index 2, max_initial_timestamp_index 1).  Recorded per case (tests/golden/<case>.npz): ids, subsampled raw logits of every
step, and per step the rule-5 margin logsumexp(timestamps) - max(text) over the masked log-probabilities the reference compares
(NaN at the forced <|0.00|> step, which returns before the comparison).  A seed is kept only if no rule-5 comparison and no final
argmax is closer than 1e-3 (tests/golden/find_healthy_seeds.py's criterion).  ts-tiny_b2 shares weights and mels with tiny_b2."""
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

CASES = [  # (case, config, weight seed, batch, config overrides)
    ("ts-tiny_b2", "whisper-tiny.en", 14, 2, {"max_length": 64}),
    # random weights never pick the one EOS id of 500 text ids: EOS (= pad, as in the .en models) is remapped onto a text token the
    # decode emits, so two rows stop early and one runs to max_length (seed and id picked by a scan under the health criterion)
    ("ts-toy_b3", "toy-ts", 32, 3, {"eos_token_id": 81, "pad_token_id": 81}),
]


def record(model, cfg, enc_out, B, max_length, BaseModelOutput):
    from transformers.generation.logits_process import (LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    no_ts = cfg["forced_decoder_ids"][-1][1]
    gc = types.SimpleNamespace(eos_token_id=cfg["eos_token_id"], no_timestamps_token_id=no_ts, forced_decoder_ids=[[1, no_ts]],
                               max_initial_timestamp_index=1)
    ts_proc = WhisperTimeStampLogitsProcessor(gc)
    tb = ts_proc.timestamp_begin
    raw, margins, top2 = [], [], []

    class Raw:   # first in the list: the raw logits of the step
        def __call__(self, input_ids, scores):
            raw.append(scores.detach().clone().numpy())
            return scores

    class Ts:    # the reference processor; its log-softmax output is captured for the rule-5 margin
        def __call__(self, input_ids, scores):
            seen = []
            f = torch.nn.functional.log_softmax

            def spy(*a, **k):
                out = f(*a, **k)
                seen.append(out.detach().clone())
                return out
            torch.nn.functional.log_softmax = spy
            try:
                scores = ts_proc(input_ids, scores)
            finally:
                torch.nn.functional.log_softmax = f
            if seen:
                lp = seen[0].double()
                margins.append((torch.logsumexp(lp[:, tb:], -1) - lp[:, :tb].max(-1).values).numpy())
            else:
                margins.append(np.full(scores.shape[0], np.nan))
            t2 = torch.topk(scores.double(), 2, dim=-1).values
            top2.append(torch.where(torch.isinf(t2[:, 1]), torch.full_like(t2[:, 0], np.inf), t2[:, 0] - t2[:, 1]).numpy())
            return scores

    procs = LogitsProcessorList([Raw(), SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1), Ts()])
    ids = torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)
    with contextlib.redirect_stdout(io.StringIO()):
        ids = model.greedy_search(ids, logits_processor=procs, stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]),
                                  pad_token_id=cfg["pad_token_id"], eos_token_id=cfg["eos_token_id"],
                                  encoder_outputs=BaseModelOutput(last_hidden_state=enc_out), use_cache=True)
    return ids, np.stack(raw, 1), np.stack(margins, 1), np.stack(top2, 1), tb


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    from whisper_trtllm_amd import synthetic
    WhisperConfig, Model, BaseModelOutput = import_reference_hf()
    only = set(sys.argv[1:])
    for case, cname, seed, B, overrides in CASES:
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
            ids, L, margin, top2, tb = record(model, cfg, enc_out, B, max_length, BaseModelOutput)
        ids = ids.numpy().astype(np.int64)
        live = np.isfinite(margin)
        stride = max(1, L.shape[-1] // 256)
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed,
               "overrides_json": json.dumps(overrides), "timestamp_begin": tb, "ids": ids,
               "logits_sub": np.ascontiguousarray(L[:, :, ::stride]), "logits_stride": stride, "logits_max": L.max(-1),
               "ts_margin": margin, "top2_margin": top2}
        n_ts = int((ids >= tb).sum())
        print(f"[{case}] ids {ids.shape} timestamps {n_ts} eos rows {int((ids == cfg['eos_token_id']).any(1).sum())} | "
              f"min |rule-5 margin| {np.abs(margin[live]).min():.3e} | min top-2 {top2.min():.3e}")
        for r in ids:
            print("   ", r.tolist())
        assert np.abs(margin[live]).min() >= 1e-3 and top2.min() >= 1e-3, "unhealthy seed: pick another"
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
