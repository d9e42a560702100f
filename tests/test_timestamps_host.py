"""CPU: Whisper's timestamp mode on the host side -- the Session path's WhisperTimeStampLogitsProcessor restatement driven by the
oracle's decoder against the reference-recorded goldens (tests/golden/make_golden_timestamps.py), the text decoder against the reference
tokenizer (tests/golden/make_golden_text_timestamps.py), the ctypes binding against the header, and the forced-list rule."""
import json
import os
import re

import numpy as np
import pytest
import torch

import cpu_ref
import whisper_trtllm_amd  # noqa: F401
from conftest import GOLDEN_DIR, load_case
from whisper_trtllm_amd import _lib, generation, runtime, synthetic
from whisper_trtllm_amd.text import WhisperTokenDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_CASES = ["ts-tiny_b2", "ts-toy_b3"]


def restated_decode(cfg, weights, mel, max_length):
    """cpu_ref decoder + generation.py's processors in timestamp mode + the run.py greedy loop."""
    W = cpu_ref.to_torch(weights)
    c = dict(cfg, max_length=max_length)
    with torch.no_grad():
        enc = cpu_ref.encoder_forward(W, cfg, torch.from_numpy(mel))
        model = lambda ids, e, past: cpu_ref.decoder_forward(W, cfg, ids.long(), e, past)
        start = torch.full((mel.shape[0], 1), cfg["decoder_start_token_id"], dtype=torch.long)
        return generation.greedy_search(model, enc, start, generation.get_logits_processor(c, 1, return_timestamps=True),
                                        generation.get_stopping_criteria(c), cfg["pad_token_id"], cfg["eos_token_id"]).numpy()


@pytest.mark.parametrize("case", TS_CASES)
def test_session_processor_reproduces_timestamp_goldens(case):
    z, cfg, weights, mel = load_case(case)
    tb = int(z["timestamp_begin"])
    want = z["ids"]
    assert tb == runtime.timestamp_rules(cfg)[1]
    # the golden exercises the rules it pins: <|0.00|> first, timestamps later on, no <|notimestamps|>
    assert (want[:, 1] == tb).all() and (want[:, 2:] >= tb).any() and not (want == tb - 1).any()
    np.testing.assert_array_equal(restated_decode(cfg, weights, mel, cfg["max_length"]), want)


def test_toy_golden_reaches_eos_and_max_length():
    z, cfg, _w, _m = load_case("ts-toy_b3")
    assert z["ids"].shape[1] == cfg["max_length"] and (z["ids"] == cfg["eos_token_id"]).any(1).any()


def test_timestamp_processor_rules_on_crafted_rows():
    """Each rule of WhisperTimeStampLogitsProcessor in isolation (vocabulary: eos 5, no_ts 7, timestamps 8..11, begin_index 2)."""
    p = generation.WhisperTimeStampLogitsProcessor(eos_token_id=5, no_timestamps_token_id=7, begin_index=2, max_initial_timestamp_index=1)
    def s():   # text id 1 well above the timestamps' total mass (rule 5 does not fire unless the masks make it)
        x = torch.zeros(1, 12)
        x[0, 1] = 3.0
        return x
    out = p(torch.tensor([[6]]), s())                        # cur_len 1 == begin_index - 1: <|0.00|> forced
    assert int(out.argmax()) == 8 and torch.isinf(out[0, :8]).all()
    out = p(torch.tensor([[6, 8]]), s())                     # cur_len 2 == begin_index: no timestamp above <|0.02|>
    assert torch.isinf(out[0, 10:]).all() and torch.isfinite(out[0, 8:10]).all() and torch.isfinite(out[0, :7]).all()
    out = p(torch.tensor([[6, 8, 9]]), s())                  # a timestamp first in the counted ids: text next
    assert torch.isinf(out[0, 8:]).all() and torch.isfinite(out[0, :7]).all()
    out = p(torch.tensor([[6, 8, 1, 9]]), s())               # text -> timestamp: its partner (or EOS..) next
    assert torch.isinf(out[0, :5]).all() and torch.isfinite(out[0, 8:]).all() and int(out.argmax()) == 8
    x = torch.full((1, 12), -5.0)
    x[0, 1] = 1.0
    x[0, 8:] = 0.0                                           # logsumexp(4 x 0) = 1.386 > 1: text masked
    out = p(torch.tensor([[6, 8, 1, 2]]), x.clone())
    assert int(out.argmax()) == 8 and torch.isinf(out[0, :8]).all()


def test_text_decoder_matches_reference_timestamps():
    gold = json.load(open(os.path.join(GOLDEN_DIR, "text_timestamps.json"), encoding="utf-8"))
    dec = WhisperTokenDecoder(gold["vocab"], gold["added_tokens"])
    assert dec.timestamp_begin == gold["timestamp_begin"]
    assert len(gold["cases"]) >= 4
    for c in gold["cases"]:
        ids = c["ids"]
        assert dec.decode(ids, skip_special_tokens=False) == c["keep"], ids
        assert dec.decode(ids, skip_special_tokens=True) == c["skip"], ids
        assert dec.decode_with_timestamps(ids) == c["with_timestamps"], ids
        got = [{"text": o["text"], "timestamp": list(o["timestamp"])} for o in dec.offsets(ids)]
        assert got == c["offsets"], ids


def test_timestamp_binding_matches_header():
    text = open(os.path.join(ROOT, "include", "whisper_trtllm_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} wt_timestamp_params;", text).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _t in _lib.TimestampParams._fields_]
    lib = _lib.load()
    assert len(lib.wt_decoder_set_timestamp_rules.argtypes) == 2
    dbg = open(os.path.join(ROOT, "include", "whisper_trtllm_amd_debug.h")).read()
    decl = re.search(r"int wt_dbg_timestamp_select\(([^)]*)\)", dbg).group(1)
    assert len(decl.split(",")) == len(lib.wt_dbg_timestamp_select.argtypes) == 12
    assert lib.wt_dbg_timestamp_select_scratch_bytes(16, 51864, 448) > 51864


def test_forced_list_rule_is_refused_by_the_builder():
    cfg = synthetic.get_config("whisper-tiny.en")
    assert runtime.timestamp_rules(cfg) == (50362, 50363, 2, 1, [])
    multi = dict(cfg, no_timestamps_token_id=50362, forced_decoder_ids=[[1, 50259], [2, 50359], [3, 50362]])
    assert runtime.timestamp_rules(multi)[2:] == (4, 1, [[1, 50259], [2, 50359]])
    bad = dict(cfg, no_timestamps_token_id=50362, forced_decoder_ids=[[1, 50362], [3, 100]])   # forced at the <|0.00|> step
    with pytest.raises(ValueError, match="forced"):
        runtime.timestamp_rules(bad)
    with pytest.raises(ValueError, match="forced"):
        generation.get_logits_processor(bad, 1, return_timestamps=True)
    with pytest.raises(ValueError, match="no_timestamps"):
        runtime.timestamp_rules(dict(cfg, forced_decoder_ids=[]))
    with pytest.raises(ValueError, match="batch-decode"):
        runtime.transcribe_continuous(None, None, [], return_timestamps=True)
