"""CPU: the decode configuration (csrc/host_logic.cpp: resolve_decode_config, StepKey) -- which decode modes go together, with which
error, what the captured step graphs are keyed on and what the arithmetic tuning choices give at the real model sizes.  Built with
g++ -fsanitize=address,undefined and run as a child process (tests/native/test_decode_config.cpp); nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import whisper_trtllm_amd as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san") / "test_decode_config"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "native", "test_decode_config.cpp"),
           os.path.join(ROOT, "whisper-trtllm_amd", "csrc", "host_logic.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True)
    return str(out)


def _run(program, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["toy-short", "whisper-tiny.en"])
def test_compatibility_table_and_key_algebra(program, name):
    cfg = w.synthetic.get_config(name)
    dims = [cfg["d_model"], cfg["decoder_attention_heads"], cfg["decoder_layers"], cfg["decoder_ffn_dim"], cfg["num_mel_bins"],
            cfg["max_source_positions"], cfg["max_target_positions"], cfg["vocab_size"]]
    _run(program, "table", *[str(v) for v in dims])


def test_derived_values_at_the_real_model_sizes(program):
    _run(program, "derived")
