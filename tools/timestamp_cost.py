#!/usr/bin/env python3
"""Cost of the timestamp mode per decode step: whisper-medium.en fp32, batch 8, `--steps` steps, plain greedy vs timestamp mode on one
decoder handle (graph replay, host mailbox loop), alternated `--reps` times after one warm-up decode of each.  Time = host clock around
generate() ending in a device synchronise (each decode runs to max_length: random weights emit no EOS), divided by the steps taken.
Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import whisper_trtllm_amd as w  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
    ms = {False: [], True: []}
    for rep in range(a.reps + 1):
        for ts in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = dec.generate(hidden, max_length=a.steps + 1, return_timestamps=ts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                ms[ts].append(1e3 * dt / (ids.shape[1] - 1))
    plain, tsm = sorted(ms[False]), sorted(ms[True])
    med = lambda v: v[len(v) // 2]
    print(json.dumps({"config": a.config, "batch": a.batch, "steps": a.steps, "ms_per_step_plain": plain, "ms_per_step_timestamps": tsm,
                      "median_plain": med(plain), "median_timestamps": med(tsm), "ratio": med(tsm) / med(plain)}))


if __name__ == "__main__":
    main()
