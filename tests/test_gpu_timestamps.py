"""GPU: Whisper's timestamp mode of the batch decode (wt_decoder_set_timestamp_rules; ts_select_kernel + greedy_finish_kernel<true>)
against the reference-recorded goldens (tests/golden/make_golden_timestamps.py), the two launches against an fp64 numpy restatement of
the rules on crafted rows (wt_dbg_timestamp_select), mode switching on one handle, the grammar at the headline model's size, the
continuous mode's refusal and run.py --return_timestamps --compare."""
import ctypes
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _engines(wt, cfg, weights):
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights), cfg)
    return enc, dec


def _check_golden(dec, hidden, z, cfg, trace=True):
    B, V, ml = hidden.shape[0], cfg["vocab_size"], cfg["max_length"]
    tr = torch.full((B, ml - 1, V), float("nan"), dtype=torch.float32, device="cuda") if trace else None
    ids = dec.generate(hidden, logits_trace=tr, return_timestamps=True).cpu().numpy()
    want = z["ids"]
    if tr is not None:
        steps = want.shape[1] - 1
        L = tr[:, :steps].cpu().numpy()
        stride = int(z["logits_stride"])
        err = np.abs(L[:, :, ::stride] - z["logits_sub"]).max()
        assert err < 1e-3, f"logits differ from the reference by {err}"
        np.testing.assert_allclose(L.max(-1), z["logits_max"], atol=1e-3)
    np.testing.assert_array_equal(ids, want)


@pytest.mark.parametrize("mode", ["graph", "graph_trace", "eager_trace"])
@pytest.mark.parametrize("case", ["ts-tiny_b2", "ts-toy_b3"])
def test_engine_matches_timestamp_golden(wt, case, mode):
    z, cfg, weights, mel = load_case(case)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    dec.set_profiling(mode.startswith("eager"))   # profiling: eager launches with per-kernel timers instead of the step graph
    _check_golden(dec, hidden, z, cfg, trace=mode.endswith("trace"))
    dec.set_profiling(False)


def test_mode_switching_on_one_handle(wt):
    """timestamp -> plain -> timestamp on ONE decoder handle (step graphs re-captured on each switch): the plain decode still equals
    tiny_b2.npz, both timestamp decodes ts-tiny_b2.npz (same weights and mels)."""
    z_ts, cfg_ts, weights, mel = load_case("ts-tiny_b2")
    z_pl, cfg_pl, _w, mel_pl = load_case("tiny_b2")
    assert np.array_equal(mel, mel_pl) and int(z_ts["seed"]) == int(z_pl["seed"])
    enc, dec = _engines(wt, cfg_ts, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    for _ in range(2):
        np.testing.assert_array_equal(dec.generate(hidden, return_timestamps=True).cpu().numpy(), z_ts["ids"])
        np.testing.assert_array_equal(dec.generate(hidden, max_length=cfg_pl["max_length"]).cpu().numpy(), z_pl["ids"])
    np.testing.assert_array_equal(dec.generate(hidden, return_timestamps=True).cpu().numpy(), z_ts["ids"])


# ---- the two launches against fp64 ---------------------------------------------------------------------------------------------------
def ref_select(x, ids, cur_len, no_ts, tb, tsbi, max_init, eos):
    """fp64 restatement of the timestamp rules (include/whisper_trtllm_amd.h (9b)) for one row: (token, logsumexp_ts, max_text)."""
    x = x.astype(np.float64).copy()
    V = x.shape[0]
    x[no_ts] = -np.inf
    seq = list(ids[tsbi:cur_len])
    last = len(seq) >= 1 and seq[-1] >= tb
    penult = len(seq) < 2 or seq[-2] >= tb
    if last and penult:
        x[tb:] = -np.inf
    elif last:
        x[:eos] = -np.inf
    if cur_len == tsbi and max_init >= 0:
        x[tb + max_init + 1:] = -np.inf
    ts = x[tb:]
    m = ts[np.isfinite(ts)].max() if np.isfinite(ts).any() else -np.inf
    lse = np.nan if np.isnan(ts).any() else (m + np.log(np.exp(ts - m).sum()) if m > -np.inf else -np.inf)
    mt = x[:tb].max()
    if cur_len == tsbi - 1:
        return tb, lse, mt
    if lse > mt:
        return tb + int(np.argmax(ts)), lse, mt
    return int(np.argmax(x)), lse, mt


def _crafted(V, tb, eos, B, rng, ml):
    """B rows cycling through the scenarios: (logits, ids history, cur_len, kind)."""
    text_hi = 100 if eos > 200 else 10
    rows = []
    kinds = ["forced0", "max_initial", "ts_ts", "text_ts", "won1", "lost1", "won30", "lost30", "all_ts_masked", "all_neginf", "nan",
             "plain30", "won1_hist", "lost30_hist", "text_ts_eos", "plain1"]
    for b in range(B):
        kind = kinds[(b + (3 * B) % 7) % len(kinds)] if B < len(kinds) else kinds[b % len(kinds)]
        scale = 30.0 if "30" in kind else 1.0
        x = (rng.standard_normal(V) * scale).astype(np.float32)
        ids = np.full(ml, text_hi, dtype=np.int32)
        cur = 6
        if kind == "forced0":
            cur = 1
        elif kind == "max_initial":
            cur = 2
            x[tb + 5] = 50.0                       # far above everything, but past the initial cap
        elif kind == "ts_ts":
            ids[4], ids[5] = tb + 3, tb + 5
            x[tb + 7] = 40.0
        elif kind in ("text_ts", "text_ts_eos"):
            ids[4], ids[5] = text_hi + 1, tb + 4
            x[3] = 40.0                            # a text id below EOS: masked
            if kind == "text_ts_eos":
                x[eos] = 35.0
        elif kind.startswith(("won", "lost")):
            if kind.endswith("_hist"):
                ids[3], ids[4], ids[5] = tb + 1, tb + 2, text_hi
            mt = float(x[:tb].max())
            d = 1e-3 if kind.startswith("won") else -1e-3
            x[tb:] = -np.inf
            x[[tb + 2, tb + 9, V - 1]] = np.float32(mt + d - np.log(3.0))
            x[no_ts_of(tb)] = 60.0                 # <|notimestamps|> is always masked
        elif kind == "all_ts_masked":
            x[tb:] = -np.inf
        elif kind == "all_neginf":
            x[:] = -np.inf
        elif kind == "nan":
            x[7] = np.nan
            x[tb + 1] = np.nan
        rows.append((x, ids, cur, kind))
    return rows


def no_ts_of(tb):
    return tb - 1


@pytest.mark.parametrize("V,tb,eos", [(51864, 50363, 50256), (1003, 901, 897)])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_timestamp_select_against_fp64(wt, V, tb, eos, B):
    lib = wt._lib.load()
    rng = np.random.default_rng(V + B)
    ml, tsbi, max_init, no_ts = 16, 2, 1, tb - 1
    rows = _crafted(V, tb, eos, B, rng, ml)
    logits = torch.from_numpy(np.stack([r[0] for r in rows])).cuda()
    ids = torch.from_numpy(np.stack([r[1] for r in rows])).cuda()
    cur = (ctypes.c_int32 * B)(*[r[2] for r in rows])
    tok = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(B, 2, dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(lib.wt_dbg_timestamp_select_scratch_bytes(B, V, ml)), dtype=torch.uint8, device="cuda")
    t = wt._lib.TimestampParams(1, no_ts, tb, tsbi, max_init)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.wt_dbg_timestamp_select(logits.data_ptr(), B, V, ids.data_ptr(), ml, cur, ctypes.byref(t), eos, tok.data_ptr(),
                                     stats.data_ptr(), scratch.data_ptr(), ctypes.c_void_p(stream))
    assert rc == 0, wt._lib.last_error()
    torch.cuda.synchronize()
    tok, stats = tok.cpu().numpy(), stats.cpu().numpy()
    for b, (x, h, c, kind) in enumerate(rows):
        assert 0 <= tok[b] < V, (kind, tok[b])
        if kind == "nan":
            continue        # no hang, a token in range; NaN ordering is the argmax's (tested with the plain path)
        want, lse, mt = ref_select(x, h, c, no_ts, tb, tsbi, max_init, eos)
        assert tok[b] == want, (kind, tok[b], want, lse, mt)
        for got, ref in ((stats[b, 0], lse), (stats[b, 1], mt)):
            if np.isfinite(ref):
                assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (kind, got, ref)
            else:
                assert got == ref, (kind, got, ref)
        if kind.startswith("won"):
            assert tok[b] >= tb and stats[b, 0] > stats[b, 1], kind
        if kind.startswith("lost"):
            assert tok[b] < tb and stats[b, 0] < stats[b, 1], kind
        if kind == "forced0":
            assert tok[b] == tb
        if kind == "max_initial":
            assert tok[b] <= tb + max_init or tok[b] < tb
        if kind == "all_ts_masked":
            assert stats[b, 0] == -np.inf and tok[b] < tb


# ---- the grammar at the headline size ------------------------------------------------------------------------------------------------
def test_grammar_medium_en_batch8(wt):
    """whisper-medium.en, batch 8, 96 steps in timestamp mode: every row starts with <|0.00|>, never emits <|notimestamps|>, never three
    timestamps in a row, never text right after a lone timestamp; row 0's first 24 steps equal the oracle + restated rules."""
    import cpu_ref
    cfg = wt.synthetic.get_config("whisper-medium.en")
    weights = wt.synthetic.make_weights(cfg, 77)
    mel = wt.synthetic.make_mel(cfg, index=300, batch=8)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ids = dec.generate(hidden, max_length=97, return_timestamps=True).cpu().numpy()
    no_ts, tb, tsbi, _mi, _f = wt.runtime.timestamp_rules(cfg)
    eos = cfg["eos_token_id"]
    for r in ids:
        assert r[1] == tb and not (r == no_ts).any()
        seq = list(r[tsbi:])
        if eos in seq:
            seq = seq[:seq.index(eos)]
        for k in range(2, len(seq)):
            assert not (seq[k] >= tb and seq[k - 1] >= tb and seq[k - 2] >= tb), (k, seq[k - 2:k + 1])
        for k in range(1, len(seq)):
            lone = seq[k - 1] >= tb and k >= 2 and seq[k - 2] < tb
            assert not (lone and seq[k] < eos), (k, seq[max(0, k - 2):k + 1])
    W = cpu_ref.to_torch(weights)
    c = dict(cfg, max_length=25)
    with torch.no_grad():
        h = cpu_ref.encoder_forward(W, cfg, torch.from_numpy(mel[:1]))
        model = lambda i, e, past: cpu_ref.decoder_forward(W, cfg, i.long(), e, past)
        start = torch.full((1, 1), cfg["decoder_start_token_id"], dtype=torch.long)
        ref = wt.generation.greedy_search(model, h, start, wt.generation.get_logits_processor(c, 1, return_timestamps=True),
                                          wt.generation.get_stopping_criteria(c), cfg["pad_token_id"], eos)[0].numpy()
    np.testing.assert_array_equal(ids[0, :len(ref)], ref)


def test_continuous_mode_refuses_timestamps(wt):
    z, cfg, weights, mel = load_case("ts-toy_b3")
    _enc, dec = _engines(wt, cfg, weights)
    lib, h = dec.session._lib, dec.session.handle
    t = wt._lib.TimestampParams(1, 502, 503, 2, 1)
    assert lib.wt_decoder_set_timestamp_rules(h, ctypes.byref(t)) == 0
    p = dec._params(None, None, None)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.wt_decoder_stream_begin(h, 4, 0, ctypes.byref(p), ctypes.c_void_p(stream)) == -38   # WT_E_UNSUPPORTED
    bad = wt._lib.TimestampParams(1, 503, 503, 2, 1)                                              # no_ts must lie below timestamp_begin
    assert lib.wt_decoder_set_timestamp_rules(h, ctypes.byref(bad)) == -22
    with pytest.raises(ValueError):
        dec.stream(slots=4, return_timestamps=True)
    dec.stream(slots=4)       # the Python stream turns the mode off first


def test_run_py_return_timestamps_compare(wt, tmp_path):
    z, cfg, weights, mel = load_case("ts-toy_b3")
    eng = tmp_path / "eng"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(wt.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(wt.convert.build_decoder_engine(cfg, weights))
    (eng / "config.pkl").write_bytes(pickle.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "3",
                          "--synthetic_start", str(int(z["mel_index"])), "--compare", "--return_timestamps", "--dump_ids",
                          str(tmp_path / "ids.json")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Compare Result: same [3], diff [0]" in out.stdout, out.stdout[-1500:]
    assert "<|0.00|>" in out.stdout
    got = json.load(open(tmp_path / "ids.json"))
    eos = cfg["eos_token_id"]
    for g, w in zip(got, z["ids"].tolist()):        # batch 1 rows per utterance in the golden's own batch of 3: same ids up to EOS
        cut = lambda r: r[:r.index(eos, 1) + 1] if eos in r[1:] else r
        assert cut(g) == cut(w)
