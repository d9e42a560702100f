#!/usr/bin/env python3
"""Cost of the long-form work: whisper-medium.en fp32 (synthetic weights), medians of `--reps` after one warm-up, each configuration in a
process of its own.

  step / step_t1   ms per decode step with no prompt set, batch 8, generate() over --steps steps, greedy and sampled at temperature 1
                   (the finish kernels and the sampling counter read per-row state now) -- on this commit and, with `--parent DIR`
                   (a checkout of the parent commit with its library built), on the parent
  long_rows<N>     seconds for --files noise recordings of --seconds each through runtime.transcribe_long(max_rows=N), N = 8 and 1
                   (one recording after the other: what a caller could do before), host clock ending in a device synchronise; thresholds
                   off and temperature 0 only, so both sides decode the same windows -- the windows are counted and must agree

A process differs from the next one on the same code by more than its own repeats do (where its buffers land, what shares the host), so
with a parent the two sides run ALTERNATELY, `--alternations` processes each, and the spread that a difference is held against is the
spread of those processes' medians.  Requirement (reported as booleans, the figures beside them): the no-prompt step time of this
commit, greedy and sampled, minus the parent's is within the spread of the processes of either side.  The speed-up of batching is
reported.  Writes profiles/longform_cost.json (or --out) and
prints it.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    sys.path.insert(0, a.root)   # this commit's package, or the parent checkout's
    import torch
    import whisper_trtllm_amd as w
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    kind, _, n = a.child.partition(":")
    out, extra = [], {}
    if kind in ("step", "step_t1"):
        hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
        kw = {"temperature": 1.0, "seed": 3} if kind == "step_t1" else {}
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = dec.generate(hidden, max_length=a.steps + 1, **kw)
            torch.cuda.synchronize()
            if rep:
                out.append(1e3 * (time.perf_counter() - t0) / (ids.shape[1] - 1))
    else:
        fe = w.audio.LogMelFrontend(n_frames=2 * cfg["max_source_positions"])
        gen = torch.Generator().manual_seed(5)
        audios = [(torch.randn(int(a.seconds * w.audio.SAMPLING_RATE), generator=gen) * 0.1).cuda() for _ in range(a.files)]
        opts = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files, trace = w.runtime.transcribe_long(enc, dec, fe, audios, max_rows=int(n), trace=True, **opts)
            torch.cuda.synchronize()
            if rep:
                out.append(time.perf_counter() - t0)
        extra = {"windows": len(trace), "segments": sum(len(f) for f in files)}
    return {"times": sorted(out), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=150.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built (python whisper-trtllm_amd/build.py)")
    ap.add_argument("--alternations", type=int, default=3, help="with --parent: processes per side of the step comparison, run alternately")
    ap.add_argument("--skip_long", action="store_true", help="only the step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longform_cost.json"))
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return
    med = lambda v: v[len(v) // 2]

    def child(what, root=ROOT):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", a.config, "--batch", str(a.batch), "--steps", str(a.steps), "--files", str(a.files),
               "--seconds", str(a.seconds), "--reps", str(a.reps), "--child", what, "--root", os.path.abspath(root)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=os.path.abspath(root))
        assert out.returncode == 0, out.stderr[-2000:]
        print(f"[{what} @ {os.path.basename(os.path.abspath(root))}] done", file=sys.stderr, flush=True)   # progress: a run takes minutes
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    res = {"config": a.config, "batch": a.batch, "steps": a.steps, "reps": a.reps}
    res["alternations"] = a.alternations if a.parent else 1
    for kind in ("step", "step_t1"):
        runs, runs_p = [], []
        for _ in range(res["alternations"]):   # this commit, the parent, this commit, ...
            runs.append(child(kind)["times"])
            if a.parent:
                runs_p.append(child(kind, a.parent)["times"])
        m = sorted(med(r) for r in runs)
        res.update({f"ms_per_{kind}": runs, f"process_medians_{kind}": m, f"median_{kind}": med(m), f"spread_{kind}": m[-1] - m[0],
                    f"spread_within_process_{kind}": max(r[-1] - r[0] for r in runs)})
        if a.parent:
            mp = sorted(med(r) for r in runs_p)
            res.update({f"ms_per_{kind}_parent": runs_p, f"process_medians_{kind}_parent": mp, f"median_{kind}_parent": med(mp),
                        f"spread_{kind}_parent": mp[-1] - mp[0], f"spread_within_process_{kind}_parent": max(r[-1] - r[0] for r in runs_p)})
            res[f"{kind}_within_spread_of_parent"] = med(m) - med(mp) <= max(m[-1] - m[0], mp[-1] - mp[0])
    if not a.skip_long:
        res.update(files=a.files, seconds_per_file=a.seconds)
        for rows in (8, 1):
            r = child(f"long:{rows}")
            res.update({f"long_rows{rows}_s": r["times"], f"median_long_rows{rows}_s": med(r["times"]), f"windows_rows{rows}": r["windows"],
                        f"segments_rows{rows}": r["segments"]})
        res["same_windows"] = res["windows_rows8"] == res["windows_rows1"] and res["segments_rows8"] == res["segments_rows1"]
        res["speedup_rows8_over_rows1"] = res["median_long_rows1_s"] / res["median_long_rows8_s"]
        res["audio_seconds_per_second_rows8"] = a.files * a.seconds / res["median_long_rows8_s"]
        res["audio_seconds_per_second_rows1"] = a.files * a.seconds / res["median_long_rows1_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
