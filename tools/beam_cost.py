#!/usr/bin/env python3
"""Cost of beam search per decode step: whisper-medium.en fp32, `--steps` steps, 16 greedy rows against 4 utterances x 4 beams on ONE
decoder handle (graph replay, host mailbox loop), alternated `--reps` times after one warm-up decode of each.  Time = host clock around
generate() ending in a device synchronise, divided by the steps taken (random weights emit no EOS: every decode runs to max_length).
Then the per-layer launches of each mode, timed through wt_decoder_time_kernel on the same handle in the middle of a decode: the
cross-attention reading one cache row per row (greedy, 16 rows) against four shared utterance rows read once per beam ("rows") and once
per utterance by a block that carries its four beams ("grouped"), and the self-attention with and without the ancestry table.  Also the largest deviation of the sequence scores from the reference-recorded goldens
(tests/golden/beam-*.npz).  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

os.environ["WT_TUNING"] = "1"   # lets WT_BEAM_CROSS pick the cross-attention form per decode (rows | grouped), read at wt_decoder_begin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_trtllm_amd as w  # noqa: E402


def golden_score_deviation():
    out = {}
    for case in ("beam-toy_b3x2", "beam-toy_b2x4", "beam-tiny_b2x4"):
        z = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
        cfg = w.synthetic.get_config(str(z["config_name"]))
        cfg.update(json.loads(str(z["overrides_json"])))
        weights = w.synthetic.make_weights(cfg, int(z["seed"]))
        enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
        dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
        hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=int(z["mel_index"]), batch=int(z["batch"]))).cuda())
        ids, sc = dec.generate(hidden, num_beams=int(z["num_beams"]), length_penalty=float(z["length_penalty"]),
                               early_stopping=bool(z["early_stopping"]), return_scores=True)
        out[case] = {"ids_equal": bool(np.array_equal(ids.cpu().numpy(), z["ids"])),
                     "max_score_deviation": float(np.abs(sc.cpu().numpy().astype(np.float64) - z["scores"]).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=16)).cuda())
    modes = {"greedy16": (1, None), "beam4x4_grouped": (4, "grouped"), "beam4x4_rows": (4, "rows")}
    ms = {k: [] for k in modes}
    for rep in range(a.reps + 1):
        for name, (nb, form) in modes.items():
            os.environ["WT_BEAM_CROSS"] = form or "grouped"
            h = hidden if nb == 1 else hidden[:4]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.generate(h, max_length=a.steps + 1, num_beams=nb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                ms[name].append(1e3 * dt / a.steps)
    kernels = {}
    for name, (nb, form) in modes.items():   # per-layer launches, half way through a decode of each mode
        os.environ["WT_BEAM_CROSS"] = form or "grouped"
        dec.begin(hidden if nb == 1 else hidden[:4], max_length=a.steps + 1, num_beams=nb)
        dec.steps(a.steps // 2)
        dec.poll()
        kernels[name] = {k: dec.time_kernel(k, 50) for k in ("self_attn", "cross_attn", "qkv", "pair", "cross_out", "fc1", "fc2")}
    os.environ.pop("WT_BEAM_CROSS")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    out = {"config": a.config, "steps": a.steps, "ms_per_step": {k: sorted(v) for k, v in ms.items()}, "median_ms_per_step": {k: med(v) for k, v in ms.items()},
           "us_per_launch_at_half_length": kernels, "golden_score_deviation": golden_score_deviation()}
    out["ratio_beam_grouped_vs_greedy16"] = out["median_ms_per_step"]["beam4x4_grouped"] / out["median_ms_per_step"]["greedy16"]
    out["ratio_beam_rows_vs_greedy16"] = out["median_ms_per_step"]["beam4x4_rows"] / out["median_ms_per_step"]["greedy16"]
    L = cfg["decoder_layers"]
    for k in ("beam4x4_grouped", "beam4x4_rows"):   # what the per-layer launches explain of the step difference; the rest: select + finish + plain-logits GEMV
        out["us_per_step_layer_launches_minus_greedy_" + k] = L * (sum(kernels[k].values()) - sum(kernels["greedy16"].values()))
    print(json.dumps(out))

if __name__ == "__main__":
    main()
