#!/usr/bin/env python3
"""Golden vectors of the token-level timestamps from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_token_timestamps.py [case ...]   (no case = all)
The reference's generate() never reads return_token_timestamps, and its cut-down decoder drops output_attentions, so generate() is run
with the softmax output of every cross-attention forward recorded as it is computed, and the reference's own
WhisperForConditionalGeneration._extract_token_timestamps (with _median_filter and _dynamic_time_warping) is called on the result.
Recorded per case (tests/golden/<case>.npz): ids, the alignment heads, the fp32 `matrix` the reference hands to the DTW, the DTW path, token_timestamps, and matrix_f64_dist = max |matrix - the same formula in float64
on the same model| (the reference's own fp32 noise after the 1 / std amplification).

Health criterion (enforced here): a seed is kept only if token_timestamps are unchanged under 32 seeded perturbations of the reference
matrix with uniform noise of amplitude 10 x the matrix test's bar, bar = 8 x matrix_f64_dist x max(1, max |matrix|).  Random-init heads
attend diffusely, so seeds are scanned; `q_scale` (recorded as an override, applied by the tests too) multiplies the cross-attention
q_proj of the synthetic weights to sharpen the heads when no seed passes without it."""
import contextlib
import copy
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import build_hf, import_reference_hf  # noqa: E402

BAR_MULTIPLE = 8.0       # tests/test_gpu_token_timestamps.py: bar = BAR_MULTIPLE x matrix_f64_dist x max(1, max |matrix|)
NOISE_MULTIPLE = 10.0
CASES = [  # (case, config, first weight seed, batch, config overrides, alignment heads, median width, q_scale candidates)
    # "eos_from": EOS is remapped onto the text id row 0 emits at that position of the seed's plain decode (as toy-short-eos1_b3 does for
    # its seed), pad = 77: a row stops early and steps on pad input to the end, inside the alignment
    ("tt-toy-short_b3", "toy-short", 11, 3, {"eos_from": 7, "pad_token_id": 77}, [[1, 0], [1, 1], [0, 1]], 7, [1.0, 4.0, 8.0, 16.0]),
    ("tt-tiny_b2", "whisper-tiny.en", 14, 2, {"max_length": 24}, [[2, 1], [3, 0], [3, 3], [3, 5]], 7, [1.0, 4.0, 8.0, 16.0]),
]
SEEDS_PER_SCALE = 24


def record_cross_attentions(model, run):
    """Run `run()` and return (its result, cross_attentions[call][layer] = softmax weights [B, H, T, S] of that decoder forward).  The
    reference's decoder layers never return their attention weights (output_attentions is dropped on the way), so the softmax output
    inside every cross-attention forward -- the reference's own numbers -- is recorded as it is computed."""
    calls, state = [], {"layer": None}
    softmax = torch.nn.functional.softmax
    H = model.config.decoder_attention_heads

    def spy(x, *a, **k):
        out = softmax(x, *a, **k)
        if state["layer"] is not None:
            calls[-1][state["layer"]] = out.detach().clone().view(-1, H, out.shape[-2], out.shape[-1])
        return out

    def wrap(i, forward):
        def f(*a, **k):
            if i == 0:
                calls.append({})
            state["layer"] = i
            try:
                return forward(*a, **k)
            finally:
                state["layer"] = None
        return f
    attns = [l.encoder_attn for l in model.model.decoder.layers]
    for i, m in enumerate(attns):
        m.forward = wrap(i, m.forward)
    torch.nn.functional.softmax = spy
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            res = run()
    finally:
        torch.nn.functional.softmax = softmax
        for m in attns:
            del m.forward
    return res, tuple(tuple(c[i] for i in range(len(attns))) for c in calls)


def reference_run(model, model64, cfg, mel, heads, width, BaseModelOutput):
    from transformers.models.whisper.modeling_whisper import _dynamic_time_warping, _median_filter
    x = torch.from_numpy(mel)
    model.config.median_filter_width = width
    ids, steps = record_cross_attentions(model, lambda: model.generate(x, output_attentions=True, return_dict_in_generate=True))
    assert len(steps) == ids.shape[1] - 1, (len(steps), ids.shape)
    # in the shape of a GreedySearchEncoderDecoderOutput: sequences, cross_attentions[step][layer]
    out = types.SimpleNamespace(sequences=ids, cross_attentions=steps)
    with torch.no_grad():
        ts = model._extract_token_timestamps(out, heads)
    # the matrix the reference hands to its DTW: the same lines as _extract_token_timestamps, up to the mean over the heads
    cross = [torch.cat([s[i] for s in steps], dim=2) for i in range(cfg["decoder_layers"])]

    def formula(cross):
        w = torch.stack([cross[l][:, h] for l, h in heads]).permute([1, 0, 2, 3])
        std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
        return _median_filter((w - mean) / std, width).mean(dim=1)
    matrix = formula(cross)
    paths = [_dynamic_time_warping(-matrix[b].double().numpy()) for b in range(ids.shape[0])]

    def stepwise():   # the same model and formula in float64, fed the reference's ids step by step (its decoder applies no causal mask)
        enc64 = model64.model.encoder(x.double()).last_hidden_state
        past = None
        for t in range(ids.shape[1] - 1):
            past = model64(encoder_outputs=BaseModelOutput(last_hidden_state=enc64), decoder_input_ids=ids[:, t:t + 1], past_key_values=past, use_cache=True).past_key_values
    _o, c64 = record_cross_attentions(model64, stepwise)
    assert len(c64) == len(steps)
    m64 = formula([torch.cat([c[i] for c in c64], dim=2) for i in range(cfg["decoder_layers"])])
    return ids.numpy().astype(np.int64), ts.numpy(), matrix.numpy(), paths, float((matrix.double() - m64).abs().max())


def healthy(matrix, ts, dist, time_precision=0.02):
    import token_timestamps_ref as R
    bar = BAR_MULTIPLE * dist * max(1.0, float(np.abs(matrix).max()))
    amp = NOISE_MULTIPLE * bar
    rng = np.random.default_rng(12345)
    for _ in range(32):
        for b in range(matrix.shape[0]):
            noisy = (matrix[b].astype(np.float64) + rng.uniform(-amp, amp, matrix[b].shape)).astype(np.float32)
            if not np.array_equal(R.token_timestamps(noisy, time_precision)[0], ts[b]):
                return False, bar, amp
    return True, bar, amp


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    from whisper_trtllm_amd import synthetic
    import token_timestamps_ref as R
    WhisperConfig, Model, BaseModelOutput = import_reference_hf()
    only = set(sys.argv[1:])
    for case, cname, seed0, B, overrides, heads, width, scales in CASES:
        if only and case not in only:
            continue
        found = None
        for q_scale in scales:
            for seed in range(seed0, seed0 + SEEDS_PER_SCALE):
                wo = {"q_scale": q_scale}
                cfg = synthetic.get_config(cname)
                weights = R.apply_overrides(synthetic.make_weights(cfg, seed), wo)
                mel = synthetic.make_mel(cfg, index=7 * seed, batch=B)
                ov = dict(overrides)
                if "eos_from" in ov:
                    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                        plain = build_hf(cfg, weights, WhisperConfig, Model).generate(torch.from_numpy(mel))
                    ov["eos_token_id"] = int(plain[0, ov.pop("eos_from")])
                cfg.update(ov)
                model = build_hf(cfg, weights, WhisperConfig, Model)
                model64 = copy.deepcopy(model).double()
                ids, ts, matrix, paths, dist = reference_run(model, model64, cfg, mel, heads, width, BaseModelOutput)
                eos_rows = int((ids[:, 1:-1] == cfg["eos_token_id"]).any(1).sum())
                if not np.isfinite(dist) or dist > 1e-3:
                    print(f"[{case}] q_scale {q_scale} seed {seed}: f64 dist {dist:.3e}, skipped")
                    continue
                ok, bar, amp = healthy(matrix, ts, dist)
                # the restatement must agree with the reference on the reference's own matrix
                for b in range(B):
                    t, pi, pj = R.token_timestamps(matrix[b])
                    assert np.array_equal(t, ts[b]) and np.array_equal(pi, paths[b][0]) and np.array_equal(pj, paths[b][1])
                print(f"[{case}] q_scale {q_scale} seed {seed}: ids {ids.shape} early-EOS rows {eos_rows} max|matrix| {np.abs(matrix).max():.3f} "
                      f"f64 dist {dist:.3e} bar {bar:.3e} noise {amp:.3e} -> {'healthy' if ok else 'fragile'}")
                if ok and ("toy" not in case or 0 < eos_rows < B):
                    found = (seed, wo, mel, ids, ts, matrix, paths, dist, bar, amp, ov)
                    break
            if found:
                break
        assert found, f"{case}: no healthy seed"
        seed, wo, mel, ids, ts, matrix, paths, dist, bar, amp, ov = found
        plen = max(len(p[0]) for p in paths)
        text = np.full((B, plen), -9, dtype=np.int32)
        time = np.full((B, plen), -9, dtype=np.int32)
        for b, (pi, pj) in enumerate(paths):
            text[b, :len(pi)], time[b, :len(pj)] = pi, pj
        out = {"config_name": cname, "seed": seed, "batch": B, "mel_index": 7 * seed, "overrides_json": json.dumps(ov),
               "weight_overrides_json": json.dumps(wo), "ids": ids, "alignment_heads": np.array(heads, dtype=np.int32),
               "median_filter_width": width, "time_precision": 0.02, "matrix": matrix.astype(np.float32),
               "path_text": text, "path_time": time, "path_len": np.array([len(p[0]) for p in paths], dtype=np.int32),
               "token_timestamps": ts.astype(np.float32), "matrix_f64_dist": dist, "matrix_bar": bar, "health_noise": amp}
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print(f"   kept seed {seed} overrides {wo}: 32 perturbations at {amp:.3e} (10 x bar {bar:.3e}) leave token_timestamps unchanged")
        for b in range(B):
            print("   ids", ids[b].tolist())
            print("   ts ", np.round(ts[b], 2).tolist())
        print("   wrote", case + ".npz", os.path.getsize(os.path.join(HERE, case + ".npz")), "bytes")


if __name__ == "__main__":
    main()
