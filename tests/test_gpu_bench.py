"""GPU: bench.py's plain run and --dump-outputs, at a tiny size (whisper-tiny.en, batch 2, 15 decoder steps) in a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_times_steps_and_dumps_the_last_pass(tmp_path):
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    model, B, ml = "whisper-tiny.en", 2, 16
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", model, "--batch", str(B), "--max-length", str(ml),
                          "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "audio-seconds/second" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for key in ("roofline", "roofline_decode", "cpu_baseline", "varlen", "fp16_engines_b16"):   # --full only
        assert key not in line, key
    assert sorted(os.listdir(tmp_path / "dump")) == ["encoder_hidden.npy", "ids.npy"]

    # the same seeded inputs through the engines in this process
    cfg = w.synthetic.get_config(model)
    cfg["max_length"] = ml
    weights = w.synthetic.make_weights(cfg, 0)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights), cfg)
    hidden = enc(torch.from_numpy(w.synthetic.make_mel(cfg, index=0, batch=B)).cuda())
    ids = dec.generate(hidden).cpu().numpy()
    got_ids = np.load(tmp_path / "dump" / "ids.npy")
    got_hidden = np.load(tmp_path / "dump" / "encoder_hidden.npy")
    assert got_ids.dtype == np.float32 and got_hidden.dtype == np.float32
    np.testing.assert_array_equal(got_ids, ids.astype(np.float32))
    np.testing.assert_allclose(got_hidden, hidden.cpu().numpy(), rtol=1e-5, atol=1e-5)
