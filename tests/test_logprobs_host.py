"""Host (no GPU): the log-probability mode's C-ABI surface, text.compression_ratio, DecodeScores arithmetic and the argument checks
of generate(..., return_logprobs=True)."""
import os
import re
import types
import zlib

import numpy as np
import pytest
import torch

import whisper_trtllm_amd as w
from whisper_trtllm_amd import _lib, runtime, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    pub = open(os.path.join(ROOT, "include", "whisper_trtllm_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "whisper_trtllm_amd_debug.h")).read()
    for sym, header, listed in (("wt_decoder_set_logprobs", pub, _lib.EXPORTS), ("wt_decoder_read_logprobs", pub, _lib.EXPORTS),
                                ("wt_dbg_logprob_select", dbg, _lib.DEBUG_EXPORTS), ("wt_dbg_logprob_select_scratch_bytes", dbg, _lib.DEBUG_EXPORTS)):
        assert hasattr(lib, sym), sym
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in listed
    assert "wt_logprob_params" in pub and [n for n, _ in _lib.LogprobParams._fields_] == ["enabled", "no_speech_token_id"]
    assert lib.wt_abi_version() == 3 and "#define WT_ABI_VERSION 3" in pub


@pytest.mark.parametrize("s", ["a", "the quick brown fox jumps over the lazy dog", "and so on " * 40, "naïve café — 你好 " * 7,
                               "x" * 1000])
def test_compression_ratio_is_openai_whispers(s):
    data = s.encode("utf-8")
    assert text.compression_ratio(s) == len(data) / len(zlib.compress(data))


def test_compression_ratio_flags_repetition():
    assert text.compression_ratio("and so on " * 40) > 2.4 > text.compression_ratio("the quick brown fox jumps over the lazy dog")


def test_decode_scores_avg_logprob():
    eos = 9
    ids = torch.tensor([[1, 4, 5, 9, 9, 9],      # EOS at position 3: three scored positions (two tokens + the EOS)
                        [1, 4, 5, 6, 7, 8],      # no EOS: all five generated positions
                        [1, 9, 9, 9, 9, 9]])     # EOS first: one scored position
    tok = torch.tensor([[0, -1.0, -2.0, -0.5, 0, 0], [0, -1, -1, -1, -1, -2.0], [0, -0.25, 0, 0, 0, 0]], dtype=torch.float32)
    total = torch.tensor([-3.5, -6.0, -0.25], dtype=torch.float32)
    sc = runtime.DecodeScores(ids, tok, total, None, eos)
    assert sc.n_scored.tolist() == [3, 5, 1]
    np.testing.assert_array_equal(sc.avg_logprob.numpy(), (total / torch.tensor([3.0, 5.0, 1.0])).numpy())
    assert sc.no_speech_prob is None and sc.token_logprobs is tok and sc.sum_logprob is total
    assert w.DecodeScores is runtime.DecodeScores


def _bare_decoder(vocab=100):
    dec = object.__new__(runtime.WhisperDecoderEngine)
    dec.session = types.SimpleNamespace(info=types.SimpleNamespace(vocab_size=vocab, n_layers=2, n_heads=2))
    dec.config, dec.max_batch = {}, 16
    return dec


def test_generate_rejects_logprobs_with_beams_before_anything_is_enqueued():
    dec = _bare_decoder()
    with pytest.raises(ValueError, match="beam search and return_logprobs"):
        dec.generate(None, num_beams=2, return_logprobs=True)
    with pytest.raises(ValueError, match="no_speech_token_id"):
        dec.generate(None, return_logprobs=True, no_speech_token_id=100)
    with pytest.raises(ValueError, match="no_speech_token_id"):
        dec.generate(None, return_logprobs=True, no_speech_token_id=-1)
    with pytest.raises(ValueError, match="needs return_logprobs"):
        dec.generate(None, no_speech_token_id=3)
