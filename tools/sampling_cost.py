#!/usr/bin/env python3
"""Cost of temperature sampling per decode step: whisper-medium.en fp32, batch 8, `--steps` steps on one decoder handle (graph replay,
host mailbox loop), each configuration in a process of its own, `--reps` timed decodes after one warm-up: the mode off ("off"), the
log-probability mode ("logprobs"), sampling at T = 1 ("sample"), timestamp mode ("ts") and sampling in timestamp mode ("ts_sample").
Time = host clock around generate() ending in a device synchronise (each decode runs to max_length: random weights emit no EOS), divided
by the steps taken.  `--parent_lib PATH` also times the mode-off decode of a library built from the PARENT commit: the two "off" figures
are the requirement -- this commit's must not be slower than the parent's by more than the spread of the repeats.  "sample" against
"logprobs" is the price of the Philox rounds and the two logarithms per (row, id); it is reported, not gated.
Writes profiles/sampling_cost.json (or --out) and prints it.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a, modes):
    import torch
    import whisper_trtllm_amd as w
    from whisper_trtllm_amd import _lib
    if a.lib:        # a parent build: it exports none of this commit's new symbols
        _lib.LIB_PATH = a.lib
        new = {"wt_decoder_set_sampling", "wt_dbg_sample_select_scratch_bytes", "wt_dbg_sample_select"}
        _lib.EXPORTS[:] = [s for s in _lib.EXPORTS if s not in new]
        _lib.DEBUG_EXPORTS[:] = [s for s in _lib.DEBUG_EXPORTS if s not in new]
        import ctypes
        import types

        class Absent:            # takes the argtypes / restype the binding sets on a symbol the parent does not have
            argtypes = restype = None

        class ParentLib(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name not in new:
                        raise
                    setattr(self, name, Absent())
                    return self.__dict__[name]
        _lib.ctypes = types.SimpleNamespace(CDLL=ParentLib, RTLD_GLOBAL=ctypes.RTLD_GLOBAL)
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = w.synthetic.get_config(a.config)
    weights = w.synthetic.make_weights(cfg, 77)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    del weights
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=300, batch=a.batch)).cuda())
    if a.lib:        # the parent's Python surface: begin() without the new setter
        dec._set_sampling = lambda *args, **kw: None
    kw = {"off": {}, "logprobs": {"return_logprobs": True}, "sample": {"return_logprobs": True, "temperature": 1.0, "seed": 1},
          "ts": {"return_timestamps": True}, "ts_sample": {"return_timestamps": True, "return_logprobs": True, "temperature": 1.0, "seed": 1}}
    ms = {m: [] for m in modes}
    for rep in range(a.reps + 1):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = dec.generate(hidden, max_length=a.steps + 1, **kw[m])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ids = out if torch.is_tensor(out) else out[0]
            if rep:
                ms[m].append(1e3 * dt / (ids.shape[1] - 1))
    return {m: sorted(v) for m, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="whisper-medium.en")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent_lib", default=None, help="libwhisper_trtllm_amd.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_cost.json"))
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)          # child process: time the mode-off decode of this library
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a, a.child.split(","))))
        return
    med = lambda v: v[len(v) // 2]

    def child(modes, lib=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", a.config, "--batch", str(a.batch), "--steps", str(a.steps),
               "--reps", str(a.reps), "--child", modes] + (["--lib", lib] if lib else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    modes = ["off", "logprobs", "sample", "ts", "ts_sample"]
    here = {m: child(m)[m] for m in modes}
    res = {"config": a.config, "batch": a.batch, "steps": a.steps, "reps": a.reps}
    for m in modes:
        res["ms_per_step_" + m] = here[m]
        res["median_" + m] = med(here[m])
        res["spread_" + m] = here[m][-1] - here[m][0]
    if a.parent_lib:
        parent = child("off", os.path.abspath(a.parent_lib))["off"]
        res.update(ms_per_step_off_parent=parent, median_off_parent=med(parent), spread_off_parent=parent[-1] - parent[0])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
