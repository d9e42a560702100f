#!/usr/bin/env python3
"""Cost of language detection: whisper-medium.en fp32 (synthetic weights), batch 8, medians of `--reps` after one warm-up, each
configuration in a process of its own.

  step        ms per decode step with the mode off (generate() over --steps steps on the plain config) -- on this commit and, with
              `--parent DIR` (a checkout of the parent commit with its library built), on the parent
  first_off   ms of begin() + the first step, host clock ending in a device synchronise, on the config with a multilingual-shaped forced
              list ([[1, L0], [2, task], [3, <|notimestamps|>]], --n_lang language ids) and no `language=`
  first_auto  the same with language="auto": the language tables' upload, lang_select_kernel in the first step's graph

A process differs from the next one on the same code by more than its own repeats do, so the sides of a comparison run ALTERNATELY,
`--alternations` processes each, and the spread a difference is held against is the spread of those processes' medians.
(a) "not slower with the mode off": this commit's step time minus the parent's lies within that spread.  (b) the added time of a decode
with language="auto", first_auto - first_off, stays below one decode step of the parent (of this commit without --parent): what a
separate detection pass, the design not taken, would cost at the least.  Both are reported as booleans with the figures beside them.
Writes profiles/language_cost.json (or --out) and prints it.  Needs a GPU."""
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
    if a.child != "step":        # language ids scattered through the text vocabulary, away from the EOS
        step = (cfg["eos_token_id"] - 1000) // a.n_lang
        langs = [1000 + i * step for i in range(a.n_lang)]
        no_ts = cfg["forced_decoder_ids"][-1][1]
        cfg = dict(cfg, language_ids=langs, forced_decoder_ids=[[1, langs[0]], [2, no_ts - 3], [3, no_ts]])
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
    ms = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.child == "step":
            ids = dec.generate(hidden, max_length=a.steps + 1)
        else:
            dec.begin(hidden, **({"language": "auto"} if a.child == "first_auto" else {}))
            dec.steps(1)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep:
            ms.append(dt / (ids.shape[1] - 1) if a.child == "step" else dt)
    return sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--n_lang", type=int, default=99)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built (python whisper-trtllm_amd/build.py)")
    ap.add_argument("--alternations", type=int, default=3, help="processes per side of a comparison, run alternately")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "language_cost.json"))
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return
    med = lambda v: v[len(v) // 2]

    def child(what, root=ROOT):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", a.config, "--batch", str(a.batch), "--steps", str(a.steps), "--n_lang", str(a.n_lang),
               "--reps", str(a.reps), "--child", what, "--root", os.path.abspath(root)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=os.path.abspath(root))
        assert out.returncode == 0, out.stderr[-2000:]
        print(f"[{what} @ {os.path.basename(os.path.abspath(root))}] done", file=sys.stderr, flush=True)   # progress: a run takes minutes
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    def side(res, name, runs):
        m = sorted(med(r) for r in runs)
        res.update({f"ms_{name}": runs, f"process_medians_{name}": m, f"median_{name}": med(m), f"spread_{name}": m[-1] - m[0]})
        return m

    res = {"config": a.config, "batch": a.batch, "steps": a.steps, "n_lang": a.n_lang, "reps": a.reps, "alternations": a.alternations,
           "parent_measured": bool(a.parent)}
    runs, runs_p = [], []
    for _ in range(a.alternations):   # this commit, the parent, this commit, ...
        runs.append(child("step"))
        if a.parent:
            runs_p.append(child("step", a.parent))
    m = side(res, "step", runs)
    one_step = med(m)
    if a.parent:
        mp = side(res, "step_parent", runs_p)
        one_step = med(mp)
        res["step_minus_parent_ms"] = med(m) - med(mp)
        res["step_within_spread_of_parent"] = med(m) - med(mp) <= max(m[-1] - m[0], mp[-1] - mp[0])
    on, off = [], []
    for _ in range(a.alternations):   # off, auto, off, ...
        off.append(child("first_off"))
        on.append(child("first_auto"))
    m_off, m_on = side(res, "first_off", off), side(res, "first_auto", on)
    res["auto_added_ms"] = med(m_on) - med(m_off)
    res["auto_added_spread_ms"] = max(m_on[-1] - m_on[0], m_off[-1] - m_off[0])
    res["one_step_ms"] = one_step
    res["auto_added_under_one_step"] = res["auto_added_ms"] < one_step
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
