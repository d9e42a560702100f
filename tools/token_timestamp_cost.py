#!/usr/bin/env python3
"""Cost of the token-level timestamps: whisper-medium.en fp32, batch 8, 447 steps (max_length 448) on one decoder handle.
  * ms per decode step with the mode off (baseline) and on (the query capture in the cross-attention launches; finished rows never
    occur here, random weights emit no EOS): host clock around begin + run ending in a device synchronise, alternated `--reps`
    times after one warm-up decode of each, the post-pass not included;
  * the post-pass at N = 447, split into the matrix launches (3 per utterance) and the DTW launch: device events around each half
    (wt_dbg_token_timestamp_postpass), `--reps` repeats after one warm-up, median;
  * the device memory the mode allocates.
Prints one JSON line.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import whisper_trtllm_amd as w  # noqa: E402

MEDIUM_EN_HEADS = [(l, h) for l in (10, 13, 16, 19, 21, 23) for h in (1, 7, 12)]   # 18 heads, the size of medium.en's own list


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=447)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    L, H = cfg["decoder_layers"], cfg["decoder_attention_heads"]
    heads = [(l, h) for l, h in MEDIUM_EN_HEADS if l < L and h < H] or [(L - 1, 0)]
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
    lib, handle = dec.session._lib, dec.session.handle
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = {False: [], True: []}
    for rep in range(a.reps + 1):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.begin(hidden, max_length=a.steps + 1, return_token_timestamps=on, alignment_heads=heads)
            cur, _nu = dec.run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                ms[on].append(1e3 * dt / (cur - 1))
    assert cur == a.steps + 1      # the mode is on and the decode ran to max_length: N = steps
    post = {1: [], 2: []}
    total = []
    for rep in range(a.reps + 1):
        for which in (1, 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w._lib.check(lib.wt_dbg_token_timestamp_postpass(handle, which, stream()), "wt_dbg_token_timestamp_postpass")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                post[which].append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.read_token_timestamps(cur)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            total.append(e0.elapsed_time(e1))
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(ms[False]), med(ms[True])
    print(json.dumps({"config": a.config, "batch": a.batch, "steps": a.steps, "heads": len(heads), "reps": a.reps,
                      "ms_per_step_off": sorted(ms[False]), "ms_per_step_capture": sorted(ms[True]), "median_off": off, "median_capture": on,
                      "capture_ratio": on / off, "decode_ms_off": off * a.steps,
                      "postpass_matrix_ms": sorted(post[1]), "postpass_dtw_ms": sorted(post[2]), "postpass_read_ms": sorted(total),
                      "median_matrix_ms": med(post[1]), "median_dtw_ms": med(post[2]), "median_read_ms": med(total),
                      "added_device_bytes": int(lib.wt_dbg_token_timestamp_bytes(handle))}))


if __name__ == "__main__":
    main()
