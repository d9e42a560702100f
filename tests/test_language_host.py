"""Host side of language detection and per-utterance language tokens (no GPU): name / id resolution and its errors, the task
substitution, what `begin` hands the engine, the long-form bookkeeping of first window versus later windows, the checkpoint loader
carrying the name maps, the header, and the host_logic validation through a stand-alone native program built with the host sanitizers
(tests/native/test_language_config.cpp; nothing is loaded into Python)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import whisper_trtllm_amd as wt
from whisper_trtllm_amd import longform
from whisper_trtllm_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANGS = [402, 3, 130, 511, 0, 256]


def _cfg(**over):
    cfg = dict(wt.synthetic.get_config("toy-short"), forced_decoder_ids=[[1, 130], [2, 505], [3, 510]], language_ids=list(LANGS))
    cfg.update(over)
    return cfg


def test_language_resolution_and_its_errors():
    cfg = _cfg()
    assert rt.resolve_languages(cfg, "auto", 3) == (LANGS, [-1, -1, -1])
    assert rt.resolve_languages(cfg, 0, 2) == (LANGS, [0, 0])                        # id 0 is an id, not "off"
    assert rt.resolve_languages(cfg, [511, "auto", None, torch.tensor(3)], 4)[1] == [511, -1, -1, 3]
    for bad in (5, -1, True, 1.0, ["auto"], [3, 3, 3], "en", "<|en|>"):              # not listed / wrong count / a name without a map
        with pytest.raises(ValueError):
            rt.resolve_languages(cfg, bad, 2)
    names = _cfg(lang_to_id={"<|en|>": 130, "<|de|>": 402, "<|fr|>": 3})
    del names["language_ids"]
    ids, rows = rt.resolve_languages(names, ["en", "<|de|>", "auto", 3], 4)
    assert ids == [3, 130, 402] and rows == [130, 402, -1, 3]                        # the map's ids, ascending
    with pytest.raises(ValueError):
        rt.resolve_languages(names, "es", 1)
    with pytest.raises(ValueError):
        rt.resolve_languages(names, 511, 1)                                          # an id the map does not hold
    # a config without language ids, and a `.en` list (position 1 is <|notimestamps|>, no language slot)
    with pytest.raises(ValueError, match="language ids"):
        rt.resolve_languages(wt.synthetic.get_config("toy-short"), "auto", 1)
    with pytest.raises(ValueError, match="position 1"):
        rt.resolve_languages(_cfg(forced_decoder_ids=[[1, 510]]), "auto", 1)
    with pytest.raises(ValueError, match="position 1"):
        rt.resolve_languages(_cfg(forced_decoder_ids=None), "auto", 1)
    with pytest.raises(ValueError):
        rt.resolve_languages(_cfg(language_ids=list(range(129)), forced_decoder_ids=[[1, 5]]), "auto", 1)
    assert rt._check_language_args(cfg, None, 2, 4, True) == (None, None)            # off: nothing to refuse
    for kw in (dict(num_beams=2, return_token_timestamps=False), dict(num_beams=1, return_token_timestamps=True)):
        with pytest.raises(ValueError):
            rt._check_language_args(cfg, "auto", 2, **kw)


def _engine(cfg):
    dec = object.__new__(wt.WhisperDecoderEngine)
    dec.config = cfg
    return dec


def _pairs(p):
    return [(p.forced_decoder_ids[2 * i], p.forced_decoder_ids[2 * i + 1]) for i in range(p.n_forced)]


def test_task_replaces_the_token_at_forced_position_2():
    cfg = _cfg(task_to_id={"transcribe": 505, "translate": 504})
    dec = _engine(cfg)
    assert rt.resolve_task(cfg, "translate") == 504 and rt.resolve_task(cfg, 77) == 77
    assert _pairs(dec._params(None, None, None)) == [(1, 130), (2, 505), (3, 510)]
    p = dec._params(None, None, None, task_id=504)
    assert _pairs(p) == [(1, 130), (2, 504), (3, 510)] and p.begin_index == 4
    p = dec._params(None, None, None, prompt_len=6, task_id=504)                     # behind a prompt: position 2 of the list, shifted
    assert _pairs(p) == [(7, 130), (8, 504), (9, 510)] and p.begin_index == 10
    ts = dict(cfg, no_timestamps_token_id=510)
    p = _engine(ts)._params(None, None, None, return_timestamps=True, task_id=504)   # timestamp mode: <|notimestamps|> leaves, the task stays
    assert _pairs(p) == [(1, 130), (2, 504)] and p.begin_index == 3
    for bad in ("transcribe ", "dictate", -1, 512, True, None):
        with pytest.raises(ValueError):
            rt.resolve_task(cfg, bad)
    with pytest.raises(ValueError, match="task_to_id"):
        rt.resolve_task(_cfg(), "translate")
    with pytest.raises(ValueError, match="position 2"):
        rt.resolve_task(dict(wt.synthetic.get_config("toy-short"), task_to_id={"translate": 504}), "translate")


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def test_begin_hands_the_engine_ids_rows_and_the_task(monkeypatch):
    dec = _engine(_cfg(task_to_id={"transcribe": 505, "translate": 504}))
    info = types.SimpleNamespace(max_target_positions=40, vocab_size=512, precision=0, max_source_positions=96, d_model=128, n_layers=2, n_heads=2)
    dec.session = types.SimpleNamespace(handle=None, _lib=_Lib(), info=info)
    dec.max_batch = 16
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))   # no GPU here
    hidden = types.SimpleNamespace(dtype=torch.float32, shape=(3, 96, 128), is_cuda=True, contiguous=lambda: hidden, data_ptr=lambda: 0)
    calls = dec.session._lib.calls
    dec.begin(hidden, language=[511, "auto", 0], task="translate", prompts=[[9, 1, 2, 3, 4], [], [9, 5]])
    name, (_h, ids, n, rows, m) = [c for c in calls if c[0] == "wt_decoder_set_languages"][-1]
    assert (n, m) == (6, 3) and [ids[i] for i in range(6)] == LANGS and [rows[i] for i in range(3)] == [511, -1, 0]
    assert [c[0] for c in calls][-1] == "wt_decoder_begin"
    # the batch-wide rules sit behind the longest prompt (5): the language position the engine derives is prompt + 1 = 6, where the forced list
    # still carries the config's own language for a caller that never asks for the mode
    assert _pairs(dec._p) == [(6, 130), (7, 504), (8, 510)] and dec._p.begin_index == 9
    dec.begin(hidden)                                                                # the next decode: the mode is switched off again
    name, (_h, ids, n, rows, m) = [c for c in calls if c[0] == "wt_decoder_set_languages"][-1]
    assert ids is None and n == 0 and rows is None
    before = len(calls)
    for bad in (dict(language="auto", num_beams=2), dict(language=[3, 3]), dict(language=7), dict(task="sing")):
        with pytest.raises(ValueError):
            dec.begin(hidden, **bad)
    assert not [c for c in calls[before:] if c[0] == "wt_decoder_begin"]             # refused before anything reached the engine
    with pytest.raises(ValueError, match="at most 16"):
        dec.generate(types.SimpleNamespace(shape=(17, 96, 128)), language="auto")
    rt.DecodeStream(dec, 2)                                                          # a stream on this handle switches the mode off first
    names = [c[0] for c in calls]
    assert names[-1] == "wt_decoder_stream_begin" and "wt_decoder_set_languages" in names[before:]


def test_decode_languages_picks_every_rows_own_probability():
    langs = rt.DecodeLanguages(torch.tensor([130, 402, 0], dtype=torch.int32), torch.tensor([[.1, .2, .3, .1, .2, .1]] * 3), LANGS)
    assert langs.prob_of_ids().tolist() == pytest.approx([.3, .1, .2])


def test_long_form_detects_on_the_first_window_and_keeps_the_language():
    """Three recordings, two rows: a recording asks for detection (-1) on its first window only; later windows, and a recording whose
    language the caller chose, carry the id; first windows and later windows share calls."""
    seen = []

    def decode(requests):
        seen.append([(r["file"], r["seek"], r["language"]) for r in requests])
        out = []
        for r in requests:
            lang = r["language"] if r["language"] >= 0 else 100 + r["file"]        # what this window would detect
            out.append(dict(tokens=[200, 5, 6, 200 + 40], temperature=0.0, avg_logprob=-0.1, no_speech_prob=None, compression_ratio=1.0,
                            language=lang, language_prob=0.5 + 0.1 * r["file"] + 0.001 * r["seek"]))
        return out

    kw = dict(n_ctx=64, max_source_positions=50, timestamp_begin=200, eos_token_id=199, startofprev_token_id=198, max_rows=2)
    files, windows, langs = longform.transcribe(decode, [250, 100, 180], languages=[-1, 7, -1], trace=True, **kw)
    assert langs == [dict(language=100, language_prob=0.5), dict(language=7, language_prob=None), dict(language=102, language_prob=0.7)]
    assert seen[0] == [(0, 0, -1), (1, 0, 7)]
    flat = [r for call in seen for r in call]
    assert [r for r in flat if r[0] == 0] == [(0, 0, -1), (0, 100, 100), (0, 200, 100)]          # detected once, then kept
    assert [r for r in flat if r[0] == 2] == [(2, 0, -1), (2, 100, 102)]
    assert any({r[2] for r in call} == {100, -1} for call in seen)                              # a later window beside a first one
    assert all(len(f) for f in files) and len(windows) == 6
    # without `languages` the requests and the result are what they were
    def plain_decode(requests):
        assert all("language" not in r for r in requests)
        return [dict(tokens=[200, 5, 240], temperature=0.0, avg_logprob=-0.1, no_speech_prob=None) for _ in requests]

    plain = longform.transcribe(plain_decode, [100], **kw)
    assert isinstance(plain, list) and len(plain) == 1 and plain[0]
    with pytest.raises(ValueError):
        longform.transcribe(decode, [100, 100], languages=[-1], **kw)


def test_load_checkpoint_carries_the_name_maps(tmp_path):
    spec = importlib.util.spec_from_file_location("_common_under_test", os.path.join(ROOT, "examples", "whisper", "_common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    json.dump({"d_model": 8, "forced_decoder_ids": None, "vocab_size": 16}, open(tmp_path / "config.json", "w"))
    json.dump({"lang_to_id": {"<|en|>": 3, "<|de|>": 4}, "task_to_id": {"transcribe": 6, "translate": 5}, "forced_decoder_ids": [[1, None], [2, 6]],
               "no_timestamps_token_id": 9}, open(tmp_path / "generation_config.json", "w"))
    torch.save({"model.decoder.embed_tokens.weight": torch.zeros(16, 8)}, tmp_path / "pytorch_model.bin")
    cfg, sd = common.load_checkpoint(str(tmp_path))
    assert cfg["lang_to_id"] == {"<|en|>": 3, "<|de|>": 4} and cfg["task_to_id"]["translate"] == 5 and cfg["no_timestamps_token_id"] == 9
    assert cfg["forced_decoder_ids"] == [[1, None], [2, 6]] and "proj_out.weight" in sd
    assert rt.language_ids_of(cfg) == [3, 4]
    with pytest.raises(ValueError, match="position 1"):         # a [1, null] list predicts the language among all tokens: no rule for it here
        rt.resolve_languages(cfg, "auto", 1)


def test_header_declares_the_calls_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "whisper_trtllm_amd.h"), encoding="utf-8").read()
    debug = open(os.path.join(ROOT, "include", "whisper_trtllm_amd_debug.h"), encoding="utf-8").read()
    assert re.search(r"int\s+wt_decoder_set_languages\(wt_engine\*\s*dec,\s*const int32_t\*\s*lang_ids,\s*int n_lang,\s*const int32_t\*\s*row_tok,\s*int n_rows\);", header)
    assert re.search(r"int\s+wt_decoder_read_languages\(wt_engine\*\s*dec,\s*int32_t\*\s*tok,\s*float\*\s*prob,\s*void\*\s*stream\);", header)
    assert "wt_dbg_lang_select(" in debug and "wt_dbg_lang_select_scratch_bytes(" in debug
    assert re.search(r"#define\s+WT_ABI_VERSION\s+3\b", header) and wt._lib.ABI_VERSION == 3
    for sym in ("wt_decoder_set_languages", "wt_decoder_read_languages"):
        assert sym in wt._lib.EXPORTS
    for sym in ("wt_dbg_lang_select", "wt_dbg_lang_select_scratch_bytes"):
        assert sym in wt._lib.DEBUG_EXPORTS
    lib = wt._lib.load()
    assert lib.wt_abi_version() == 3 and hasattr(lib, "wt_decoder_set_languages") and hasattr(lib, "wt_dbg_lang_select")


@pytest.mark.parametrize("name", ["toy-short", "whisper-tiny.en"])
def test_host_logic_validates_the_language_tables(tmp_path, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = tmp_path / "test_language_config"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "test_language_config.cpp"),
                    os.path.join(ROOT, "whisper-trtllm_amd", "csrc", "host_logic.cpp"), "-o", str(out)], check=True)
    cfg = wt.synthetic.get_config(name)
    dims = [cfg["d_model"], cfg["decoder_attention_heads"], cfg["decoder_layers"], cfg["decoder_ffn_dim"], cfg["num_mel_bins"],
            cfg["max_source_positions"], cfg["max_target_positions"], cfg["vocab_size"]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(out), *[str(v) for v in dims]], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
