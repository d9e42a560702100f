#!/usr/bin/env python3
"""Golden vectors of the temperature sampler from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling.py [case ...]   (no case = all)
The reference's `greedy_search` is called with the processor list of make_golden_logprobs.py, followed by the reference's own
TemperatureLogitsWarper(T) and a last entry that adds the sampler's Gumbel noise (tests/sampling_ref.py: Philox-4x32-10 on counter
(v >> 2, t, 0, 0) with t = input_ids.shape[1], keyed by the row's seed; fp32) -- so the argmax of the reference's loop IS the Gumbel-max
draw over the reference's warped scores.  Recorded per case (tests/golden/<case>.npz): ids, log_softmax of the processed scores BEFORE
the warper at the chosen ids (float64 arithmetic on the reference's fp32 scores; the sampler's log-probabilities are those of the
untempered scores), the top-2 margin of the key per step, the temperature and the row seeds.  A seed is kept only if no live margin is
under 1e-3 (tests/golden/find_healthy_seeds.py's criterion).  Every case shares weights and mels with the lp-* case of the same model and
must differ from its greedy ids in at least one row: otherwise the golden shows nothing."""
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
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import build_hf, import_reference_hf  # noqa: E402
import sampling_ref  # noqa: E402

CASES = [  # (case, greedy case of the same weights, config, weight seed, batch, config overrides, timestamp mode, temperature, sampler seed)
    ("sm-tiny_b2", "lp-tiny_b2", "whisper-tiny.en", 14, 2, {"max_length": 24}, False, 0.6, 1),
    ("sm-toy-short_b3", "lp-toy-short_b3", "toy-short", 11, 3, {"eos_token_id": 392, "pad_token_id": 392}, False, 1.0, 8),   # (seeds 1 .. 7: no row stops early)
    ("sm-ts-toy_b3", "lp-ts-toy_b3", "toy-ts", 32, 3, {"eos_token_id": 81, "pad_token_id": 81}, True, 0.8, 1),
]


def record(model, cfg, enc_out, B, max_length, BaseModelOutput, ts_mode, T, seeds):
    from transformers.generation.logits_process import (ForceTokensLogitsProcessor, LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, TemperatureLogitsWarper, WhisperTimeStampLogitsProcessor)
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    processed, top2 = [], []

    class Processed:   # the scores after every processor, before the warper
        def __call__(self, input_ids, scores):
            processed.append(scores.detach().clone().double().numpy())
            return scores

    class Noise:       # last: the Gumbel noise of position t = input_ids.shape[1], then the margin of the key's argmax
        def __call__(self, input_ids, scores):
            t = input_ids.shape[1]
            g = np.stack([sampling_ref.gumbel(seeds[b], t, scores.shape[1], np.float32) for b in range(scores.shape[0])])
            key = scores + torch.from_numpy(g)
            t2 = torch.topk(key.double(), 2, dim=-1).values
            top2.append(torch.where(torch.isinf(t2[:, 1]), torch.full_like(t2[:, 0], np.inf), t2[:, 0] - t2[:, 1]).numpy())
            return key

    forced = cfg["forced_decoder_ids"]
    if ts_mode:
        no_ts = forced[-1][1]
        gc = types.SimpleNamespace(eos_token_id=cfg["eos_token_id"], no_timestamps_token_id=no_ts, forced_decoder_ids=[[1, no_ts]],
                                   max_initial_timestamp_index=1)
        procs = [SuppressTokensLogitsProcessor(cfg["suppress_tokens"]), SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1),
                 WhisperTimeStampLogitsProcessor(gc)]
    else:
        procs = [SuppressTokensLogitsProcessor(cfg["suppress_tokens"]),
                 SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 1 + forced[-1][0]), ForceTokensLogitsProcessor(forced)]
    procs += [Processed(), TemperatureLogitsWarper(T), Noise()]
    ids = torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)
    with contextlib.redirect_stdout(io.StringIO()):
        out = model.greedy_search(ids, logits_processor=LogitsProcessorList(procs),
                                  stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]),
                                  pad_token_id=cfg["pad_token_id"], eos_token_id=cfg["eos_token_id"],
                                  encoder_outputs=BaseModelOutput(last_hidden_state=enc_out), use_cache=True)
    return out, processed, np.stack(top2, 1)


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    from whisper_trtllm_amd import synthetic
    WhisperConfig, Model, BaseModelOutput = import_reference_hf()
    only = set(sys.argv[1:])
    for case, greedy_case, cname, seed, B, overrides, ts_mode, T, sampler_seed in CASES:
        if only and case not in only:
            continue
        cfg = synthetic.get_config(cname)
        cfg.update(overrides)
        max_length = cfg["max_length"]
        weights = synthetic.make_weights(cfg, seed)
        mel = synthetic.make_mel(cfg, index=7 * seed, batch=B)
        model = build_hf(cfg, weights, WhisperConfig, Model)
        greedy = np.load(os.path.join(HERE, greedy_case + ".npz"))["ids"]
        eos = cfg["eos_token_id"]
        while True:
            seeds = [sampler_seed + b for b in range(B)]
            with torch.no_grad():
                enc_out = model.model.encoder(torch.from_numpy(mel)).last_hidden_state
                ids, processed, top2 = record(model, cfg, enc_out, B, max_length, BaseModelOutput, ts_mode, T, seeds)
            ids = ids.numpy().astype(np.int64)
            live = np.ones(top2.shape, dtype=bool)   # a row's decisions count up to its EOS
            for b in range(B):
                hit = np.nonzero(ids[b, 1:] == eos)[0]
                if hit.size:
                    live[b, hit[0] + 1:] = False
            stopped = (ids[:, 1:-1] == eos).any(1)
            # sm-toy-short_b3: like its greedy twin, some rows must stop early and some run on (the sampler seed is searched for that)
            wanted = case != "sm-toy-short_b3" or (stopped.any() and not stopped.all())
            if top2[live].min() >= 1e-3 and wanted:
                break
            print(f"[{case}] sampler seed {sampler_seed}: min live margin {top2[live].min():.3e}, rows stopped early {stopped.tolist()} -- next")
            sampler_seed += 1
        lp = np.zeros((B, ids.shape[1] - 1))
        for k, s in enumerate(processed):
            for b in range(B):
                fin = s[b][s[b] > -np.inf]
                lp[b, k] = s[b, ids[b, k + 1]] - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))
        width = max(ids.shape[1], greedy.shape[1])
        padto = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=cfg["pad_token_id"])
        differs = (padto(ids) != padto(greedy)).any(1)
        assert differs.any(), "the sampled ids equal the greedy golden: the golden would show nothing"
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed, "overrides_json": json.dumps(overrides),
               "timestamp_mode": int(ts_mode), "temperature": np.float32(T), "sampler_seeds": np.array(seeds, dtype=np.uint64), "ids": ids,
               "token_logprobs": lp.astype(np.float64), "top2_margin": top2}
        print(f"[{case}] T {T} sampler seeds {seeds} ids {ids.shape} eos rows {int((ids[:, 1:] == eos).any(1).sum())} | "
              f"min live key margin {top2[live].min():.3e} | rows that differ from {greedy_case}: {differs.tolist()}")
        for r, t in zip(ids, lp):
            print("   ", r.tolist())
            print("   ", np.round(t, 3).tolist())
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
