#!/usr/bin/env python3
"""Cost of a decoder prompt: whisper-medium.en fp32 (synthetic weights), batch 8, medians of `--reps` after one warm-up, each configuration
in a process of its own.

  begin_len<N>   wt_decoder_begin with a shared prompt of N tokens (N in --lens, default 4 16 64 222), host clock around begin() ending in
                 a device synchronise; "prefill_ms" is that minus "begin_len0", the same call without a prompt (the cross-K/V projection,
                 the state kernels)
  forced_len<N>  the way a prompt had to be fed before: N forced decode steps (start token = prompt[0], the rest through
                 forced_decoder_ids), host clock around steps(N) ending in a synchronise, begin() excluded -- measured on the PARENT commit
                 when `--parent DIR` names a checkout of it with its library built (else on this one, and the result says so)
  step           ms per decode step with no prompt set (generate() over --steps steps), on this commit and on the parent

Requirements (reported as booleans, the figures beside them): the no-prompt step time of this commit is within the spread of the repeats
of the parent's; the 222-token prefill takes less than a quarter of the parent's 222 forced steps.  The crossover at small N is reported,
not tuned for.  Writes profiles/prompt_cost.json (or --out) and prints it.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prompt_of(cfg, n):
    """prompt[0] stands for <|startofprev|>; text ids below the specials, away from the suppressed ones"""
    banned = set(cfg["suppress_tokens"]) | set(cfg["begin_suppress_tokens"]) | {cfg["eos_token_id"], cfg["pad_token_id"]}
    text = [t for t in range(1000, 1000 + 4 * n) if t not in banned][:n - 1]
    return [cfg["vocab_size"] - 1504] + text


def measure(a):
    sys.path.insert(0, a.root)   # this commit's package, or the parent checkout's
    import torch
    import whisper_trtllm_amd as w
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    kind, _, n = a.child.partition(":")
    n = int(n or 0)
    if kind == "forced":
        p = prompt_of(cfg, n)
        cfg = dict(cfg, decoder_start_token_id=p[0],
                   forced_decoder_ids=[[i, p[i]] for i in range(1, n)] + [[n, cfg["decoder_start_token_id"]]] +
                                      [[pos + n, tok] for pos, tok in cfg["forced_decoder_ids"]])
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
    ms = []
    for rep in range(a.reps + 1):
        if kind == "forced":
            dec.begin(hidden)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "begin":
            dec.begin(hidden, **({"prompt_ids": prompt_of(cfg, n)} if n else {}))
        elif kind == "forced":
            dec.steps(n)
        else:
            ids = dec.generate(hidden, max_length=a.steps + 1)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep:
            ms.append(dt / (ids.shape[1] - 1) if kind == "step" else dt)
    return sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lens", type=int, nargs="+", default=[4, 16, 64, 222])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built (python whisper-trtllm_amd/build.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_cost.json"))
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return
    med = lambda v: v[len(v) // 2]

    def child(what, root=ROOT):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", a.config, "--batch", str(a.batch), "--steps", str(a.steps),
               "--reps", str(a.reps), "--child", what, "--root", os.path.abspath(root)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=os.path.abspath(root))
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    old = a.parent or ROOT
    res = {"config": a.config, "batch": a.batch, "steps": a.steps, "reps": a.reps, "forced_steps_measured_on": "parent" if a.parent else "this commit"}
    b0 = child("begin:0")
    res.update(begin_len0_ms=b0, median_begin_len0=med(b0))
    for n in a.lens:
        b, f = child(f"begin:{n}"), child(f"forced:{n}", old)
        res[f"begin_len{n}_ms"], res[f"forced_len{n}_ms"] = b, f
        res[f"prefill_ms_len{n}"] = med(b) - med(b0)
        res[f"forced_ms_len{n}"] = med(f)
        res[f"prefill_over_forced_len{n}"] = (med(b) - med(b0)) / med(f)
    s = child("step")
    res.update(ms_per_step=s, median_step=med(s), spread_step=s[-1] - s[0])
    if a.parent:
        sp = child("step", a.parent)
        res.update(ms_per_step_parent=sp, median_step_parent=med(sp), spread_step_parent=sp[-1] - sp[0])
        res["step_within_spread_of_parent"] = med(s) - med(sp) <= max(s[-1] - s[0], sp[-1] - sp[0])
    big = max(a.lens)
    res[f"prefill_len{big}_under_a_quarter_of_forced"] = res[f"prefill_over_forced_len{big}"] < 0.25
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
