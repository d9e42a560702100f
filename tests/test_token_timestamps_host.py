"""CPU: the float64 / numpy restatement of the token-level timestamp post-pass (tests/token_timestamps_ref.py) against the goldens the
reference recorded (tests/golden/make_golden_token_timestamps.py), the argument refusals of the Python layer, and the C-ABI exports."""
import types

import numpy as np
import pytest

import token_timestamps_ref as R
from conftest import load_case

CASES = ["tt-toy-short_b3", "tt-tiny_b2"]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden_path_and_timestamps(case):
    z, cfg, _w, _mel = load_case(case)
    ids, matrix = z["ids"], z["matrix"]
    assert matrix.shape == (ids.shape[0], ids.shape[1] - 1, cfg["max_source_positions"]) and matrix.dtype == np.float32
    for b in range(ids.shape[0]):
        ts, text, time = R.token_timestamps(matrix[b], float(z["time_precision"]))
        n = int(z["path_len"][b])
        np.testing.assert_array_equal(text, z["path_text"][b, :n])
        np.testing.assert_array_equal(time, z["path_time"][b, :n])
        np.testing.assert_array_equal(ts, z["token_timestamps"][b])
        assert ts.dtype == np.float32 and ts[0] == 0


def test_golden_has_pad_steps_inside_the_alignment():
    z, cfg, _w, _mel = load_case("tt-toy-short_b3")
    ids = z["ids"]
    early = [(r[1:-1] == cfg["eos_token_id"]).any() for r in ids]
    assert any(early) and not all(early)
    assert cfg["pad_token_id"] != cfg["eos_token_id"] and (ids == cfg["pad_token_id"]).any()
    assert float(z["health_noise"]) == pytest.approx(10 * 8 * float(z["matrix_f64_dist"]) * max(1.0, float(np.abs(z["matrix"]).max())))


def test_median_filter_is_a_reflect_padded_selection():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 33))
    x[0, 1, 4] = np.nan
    for width in (1, 3, 7, 15):
        got = R.median_filter(x, width)
        pad = width // 2
        for s in (0, 1, 16, 31, 32):
            idx = [abs(s + k - pad) for k in range(width)]
            idx = [i if i < 33 else 2 * 32 - i for i in idx]
            want = np.sort(x[..., idx], axis=-1)[..., pad]
            np.testing.assert_array_equal(got[..., s], want)
    short = rng.standard_normal((1, 4, 7))
    assert R.median_filter(short, 15) is not None and np.array_equal(R.median_filter(short, 15), short)   # S <= width // 2: unchanged
    with pytest.raises(ValueError):
        R.median_filter(x, 4)


def test_dtw_degenerate_inputs():
    ts, text, time = R.token_timestamps(np.full((1, 6), np.nan, np.float32))      # one token: std = 0 -> an all-NaN matrix
    np.testing.assert_array_equal(text, [0] * 6)
    np.testing.assert_array_equal(time, np.arange(6))
    np.testing.assert_array_equal(ts, np.array([0, 0], np.float32))
    ts, text, time = R.token_timestamps(np.full((3, 4), np.nan, np.float32))      # all NaN: left along the last row, then up the border
    np.testing.assert_array_equal(text, [0, 1, 2, 2, 2, 2, 2])
    np.testing.assert_array_equal(time, [-1, -1, -1, 0, 1, 2, 3])
    np.testing.assert_array_equal(ts, np.float32([0, -0.02, -0.02, -0.02]))
    ts, text, time = R.token_timestamps(np.zeros((3, 3), np.float32))             # ties everywhere fall through to "left"
    assert len(text) == len(time) and text[0] == 0 and text[-1] == 2 and time[-1] == 2


def test_argument_refusals():
    import whisper_trtllm_amd as wt
    chk = wt.runtime._check_token_timestamp_args
    info = types.SimpleNamespace(n_layers=2, n_heads=2)
    assert chk({}, info, False, None, 7, 1) == []
    assert chk({"alignment_heads": [[1, 0]]}, info, True, None, 7, 1) == [(1, 0)]
    assert chk({"alignment_heads": [[1, 0]]}, info, True, [(0, 1), (1, 1)], 7, 1) == [(0, 1), (1, 1)]
    with pytest.raises(ValueError, match="no `alignment_heads`, token-level timestamps not available"):
        chk({}, info, True, None, 7, 1)
    with pytest.raises(ValueError, match="beam"):
        chk({}, info, True, [(0, 0)], 7, 4)
    for bad in ([(2, 0)], [(0, 2)], [(-1, 0)], [(0, 0), (0, 0)], [(0, 0)] * 33):
        with pytest.raises(ValueError):
            chk({}, info, True, bad, 7, 1)
    for width in (4, 0, 17, -3, 7.0):
        with pytest.raises(ValueError, match="odd"):
            chk({}, info, True, [(0, 0)], width, 1)
    with pytest.raises(ValueError, match="batch-decode"):
        wt.WhisperDecoderEngine.stream(object(), 4, return_token_timestamps=True)


def test_c_abi_exports_present():
    import whisper_trtllm_amd as wt
    lib = wt._lib.load()
    for sym in ("wt_decoder_set_token_timestamps", "wt_decoder_read_token_timestamps"):
        assert sym in wt._lib.EXPORTS and hasattr(lib, sym)
    for sym in ("wt_dbg_token_timestamps_scratch_bytes", "wt_dbg_token_timestamp_matrix_kernels", "wt_dbg_token_timestamp_median",
                "wt_dbg_token_timestamp_dtw", "wt_dbg_token_timestamp_q_hist", "wt_dbg_token_timestamp_matrix"):
        assert sym in wt._lib.DEBUG_EXPORTS and hasattr(lib, sym)
    assert lib.wt_abi_version() == 3
    assert lib.wt_decoder_set_token_timestamps(None, None) == -22      # not a decoder engine


def test_words_match_reference_grouping():
    """WhisperTokenDecoder.words / combine_tokens_into_words against the reference tokenizer's _combine_tokens_into_words and
    _collate_word_timestamps (tests/golden/make_golden_text_words.py)."""
    import json
    import os

    from conftest import GOLDEN_DIR
    from whisper_trtllm_amd.text import WhisperTokenDecoder
    base = json.load(open(os.path.join(GOLDEN_DIR, "text_timestamps.json"), encoding="utf-8"))
    gold = json.load(open(os.path.join(GOLDEN_DIR, "text_words.json"), encoding="utf-8"))
    dec = WhisperTokenDecoder(base["vocab"], base["added_tokens"])
    assert len(gold["cases"]) >= 12
    assert any(len(c["words"]) < len(c["ids"]) for c in gold["cases"]) and any('"' in w or "(" in w for c in gold["cases"] for w in c["words"])
    for c in gold["cases"]:
        words, toks, idx = dec.combine_tokens_into_words(c["ids"])
        assert (words, toks, idx) == (c["words"], c["word_tokens"], c["indices"]), c["ids"]
        got = dec.words(c["ids"], [tuple(s) for s in c["spans"]])
        assert [{"text": w["text"], "timestamp": list(w["timestamp"])} for w in got] == c["timed"], c["ids"]
        starts = [s[0] for s in c["spans"]]            # the flat form generate() returns: a token ends where the next one starts
        flat = dec.words(c["ids"], starts)
        assert [w["text"] for w in flat] == c["words"]
        for w, ix in zip(flat, idx):
            assert w["timestamp"] == (starts[ix[0]], starts[ix[-1] + 1] if ix[-1] + 1 < len(starts) else starts[ix[-1]])
    with pytest.raises(ValueError):
        dec.words([1, 2, 3], [0.0])
