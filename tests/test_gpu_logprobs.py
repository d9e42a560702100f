"""GPU: token log-probabilities, sum / avg_logprob and no_speech_prob of the batch decode (wt_decoder_set_logprobs; the log-sum-exp
epilogue of the vocabulary GEMV, greedy_select_kernel<true> / ts_select_kernel<true> and the LP finish kernels) against the
reference-recorded goldens (tests/golden/make_golden_logprobs.py), the launches per element against an fp64 numpy log-softmax
(wt_dbg_logprob_select), the timestamp-mode pick on crafted rows, repeatability, mode switching, the refusals, the headline
model's grid and run.py --return_logprobs."""
import ctypes
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP_CASES = ["lp-tiny_b2", "lp-toy-short_b3", "lp-ts-toy_b3"]


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


def _fp32_running_sum(row):
    acc = np.float32(0.0)
    for v in row:
        acc = np.float32(acc + np.float32(v))
    return acc


# ---- 1. the engine against the reference-recorded goldens ------------------------------------------------------------------------
def check_golden(wt, case):
    """ids equal; token_logprobs through each row's EOS within 2e-3 (twice the project's 1e-3 logit bound: x_tok - lse moves by at most
    |dx_tok| + max|dx|); forced positions and positions behind the EOS exactly 0; sum_logprob the fp32 running sum of the row;
    no_speech_prob within 2e-3 x p."""
    z, cfg, weights, mel = load_case(case)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ts = bool(int(z["timestamp_mode"]))
    ids, sc = dec.generate(hidden, return_timestamps=ts, return_logprobs=True, no_speech_token_id=int(z["no_speech_token_id"]))
    ids = ids.cpu().numpy()
    np.testing.assert_array_equal(ids, z["ids"])
    got, want = sc.token_logprobs.cpu().numpy(), z["token_logprobs"]
    assert got.shape == ids.shape and want.shape[1] == ids.shape[1] - 1
    eos = cfg["eos_token_id"]
    forced_pos = [1]     # <|notimestamps|> by forced_decoder_ids, or the timestamp mode's <|0.00|>
    worst = 0.0
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, 1:] == eos)[0]
        last = int(hit[0]) + 1 if hit.size else ids.shape[1] - 1      # last scored position
        assert got[b, 0] == 0.0
        err = np.abs(got[b, 1:last + 1] - want[b, :last]).max()
        worst = max(worst, float(err))
        assert err <= 2e-3, (case, b, err)
        for t in forced_pos:
            assert got[b, t] == 0.0 and want[b, t - 1] == 0.0
        assert (got[b, last + 1:] == 0.0).all()
        assert sc.sum_logprob[b].item() == _fp32_running_sum(got[b, 1:last + 1])
        assert int(sc.n_scored[b]) == last
        assert sc.avg_logprob[b].item() == np.float32(sc.sum_logprob[b].item()) / np.float32(last)
    p = z["no_speech_prob"]
    rel = np.abs(sc.no_speech_prob.cpu().numpy().astype(np.float64) - p) / p
    print(f"{case}: max |token_logprob - reference| {worst:.3e}, no_speech_prob relative error {rel.max():.3e}")
    assert rel.max() <= 2e-3, (case, rel)


@pytest.mark.parametrize("case", LP_CASES)
def test_engine_matches_logprob_golden(wt, case):
    check_golden(wt, case)


def test_unfused_form_matches_logprob_goldens():
    """WT_NO_FUSED_ARGMAX=1 (latched per process): logits to memory + greedy_select_kernel<true>, same checks in a fresh process."""
    env = dict(os.environ, WT_NO_FUSED_ARGMAX="1", WT_TUNING="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--check-goldens"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.count("max |token_logprob - reference|") == len(LP_CASES)


# ---- 2. the launches per element against fp64 -------------------------------------------------------------------------------------
def ref_logprob(L, mask, at_begin, tok_override=None):
    """fp64 log-softmax of one step: (token by torch.argmax's NaN-aware rule, its log-probability) per row."""
    s = L.astype(np.float64).copy()
    s[:, (mask & 1) != 0] = -np.inf
    if at_begin:
        s[:, (mask & 2) != 0] = -np.inf
    toks, lps = [], []
    for r in s:
        tok = int(np.argmax(np.isnan(r))) if np.isnan(r).any() else int(np.argmax(r))
        fin = r[r > -np.inf]
        if fin.size == 0 or np.isnan(fin).any():
            lp = np.nan
        else:
            m = fin.max()
            lp = r[tok] - (m + np.log(np.exp(fin - m).sum()))
        toks.append(tok)
        lps.append(lp)
    return np.array(toks), np.array(lps)


def tolerance(L, mask, at_begin):
    """16 x the largest error of torch.log_softmax in fp32 on the CPU against fp64 on the same (processed) rows, floored at 4 ulp of
    the largest |logit|: the margin covers another summation tree and the device's expf."""
    s = torch.from_numpy(L.copy())
    s[:, torch.from_numpy((mask & 1) != 0)] = -np.inf
    if at_begin:
        s[:, torch.from_numpy((mask & 2) != 0)] = -np.inf
    ok = torch.isfinite(s).any(1) & ~torch.isnan(s).any(1)
    s = s[ok]
    if s.shape[0] == 0:
        return 0.0, 0.0, 0.0
    d = (torch.log_softmax(s, -1).double() - torch.log_softmax(s.double(), -1))
    ref_err = float(d[torch.isfinite(d)].abs().max())
    fin = np.abs(L[np.isfinite(L)])
    floor = 4.0 * float(np.spacing(np.float32(fin.max())))
    return max(16.0 * ref_err, floor), ref_err, floor


def run_select(wt, form, L, mask, cur_len, begin_index, eos, ml=8, step=0, ns=-1, ts=None, ids=None, forced=None, force_eos_step=-1, nan_row=None):
    """One step through wt_dbg_logprob_select.  form 0 builds the GEMV operands whose product is L exactly: X = unit rows, W[:, b] = L[b]
    (a NaN row comes from a NaN in X, since 0 x NaN would spread a NaN weight to every row)."""
    lib = wt._lib.load()
    B, V = L.shape
    dev = "cuda"
    K = 64
    X = W = lg = None
    if form == 0:
        Xh = np.zeros((B, K), dtype=np.float32)
        Xh[np.arange(B), np.arange(B)] = 1.0
        Wh = np.zeros((V, K), dtype=np.float32)
        Wh[:, :B] = L.T
        if nan_row is not None:
            Xh[nan_row, nan_row] = np.nan
        X, W = torch.from_numpy(Xh).to(dev), torch.from_numpy(Wh).to(dev)
    else:
        lg = torch.from_numpy(np.ascontiguousarray(L)).to(dev)
    mk = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    ids_d = torch.from_numpy(ids if ids is not None else np.full((B, ml), 3, dtype=np.int32)).to(dev)
    fo = (ctypes.c_int32 * ml)(*([-1] * ml if forced is None else forced))
    lp = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    sm = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    nsp = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.wt_dbg_logprob_select_scratch_bytes(B, V, ml), dtype=torch.uint8, device=dev)
    t = wt._lib.TimestampParams(1, *ts) if ts is not None else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    rc = lib.wt_dbg_logprob_select(form, ptr(X), ptr(W), K, ptr(lg), mk.data_ptr(), fo, ids_d.data_ptr(), B, V, ml, cur_len, step, begin_index, eos,
                                   force_eos_step, ctypes.byref(t) if t is not None else None, ns, lp.data_ptr(), sm.data_ptr(),
                                   nsp.data_ptr() if ns >= 0 else None, scratch.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, wt._lib.last_error())
    return ids_d[:, cur_len].cpu().numpy(), lp.cpu().numpy(), sm.cpu().numpy(), nsp.cpu().numpy()


def _compare(got_tok, got_lp, got_sum, L, mask, at_begin, what):
    want_tok, want_lp = ref_logprob(L, mask, at_begin)
    tol, ref_err, floor = tolerance(L, mask, at_begin)
    np.testing.assert_array_equal(got_tok, want_tok, err_msg=what)
    assert np.array_equal(np.isnan(got_lp), np.isnan(want_lp)), (what, got_lp, want_lp)
    live = ~np.isnan(want_lp)
    err = float(np.abs(got_lp[live] - want_lp[live]).max()) if live.any() else 0.0
    print(f"{what}: max error {err:.3e} | fp32 torch.log_softmax error {ref_err:.3e}, 4 ulp floor {floor:.3e} -> tolerance {tol:.3e}")
    assert err <= tol, (what, err, tol)
    assert np.array_equal(got_sum[live], got_lp[live])     # one step: the sum is the step's entry
    return want_lp


@pytest.mark.parametrize("form", [0, 1], ids=["fused", "unfused"])
@pytest.mark.parametrize("B,V", [(1, 612), (3, 1000), (8, 51864), (16, 515), (16, 1000), (8, 612)])
def test_select_matches_fp64_log_softmax(wt, B, V, form):
    rng = np.random.default_rng(1000 * B + V)
    eos, begin = V - 7, 3
    scales = [1.0, 30.0, 1e-3, 1.0, 5.0, 1.0, 30.0, 1e-3]
    L = np.stack([(rng.standard_normal(V) * scales[b % len(scales)]).astype(np.float32) for b in range(B)])
    mask = np.zeros(V, dtype=np.uint8)
    mask[rng.choice(V, V // 10, replace=False)] |= 1
    mask[rng.choice(V, 5, replace=False)] |= 2
    sup, beg = int(np.nonzero(mask == 1)[0][3]), int(np.nonzero(mask == 2)[0][0])
    L[0, sup] = np.abs(L[0]).max() + 3.0            # the maximum sits on a suppressed id
    if B > 1:
        L[1, beg] = np.abs(L[1]).max() + 40.0       # ... on a begin-suppressed id (masked at begin_index, the winner away from it)
    if B > 2:
        L[2, :] = -50.0                             # all mass in the tail of the last workgroup
        L[2, V - 3:] = 20.0
        mask[V - 3:] = 0
    ns = 11
    for cur_len in (begin, begin + 1):
        tok, lp, sm, nsp = run_select(wt, form, L, mask, cur_len, begin, eos, ns=ns)
        _compare(tok, lp, sm, L, mask, cur_len == begin, f"B{B} V{V} form{form} cur_len{cur_len}")
        raw = L.astype(np.float64)
        want = raw[:, ns] - (raw.max(1) + np.log(np.exp(raw - raw.max(1, keepdims=True)).sum(1)))
        tol, _r, _f = tolerance(L, np.zeros(V, dtype=np.uint8), False)
        # the same bound on log p, stated on p (+ the rounding of p itself; below fp32's normal range p may flush to zero)
        assert (np.abs(nsp.astype(np.float64) - np.exp(want)) <= (np.expm1(tol) + 4 * np.finfo(np.float32).eps) * np.exp(want) + 1e-37).all()
    # one survivor among -inf: the log-probability is exactly 0
    one = np.ones(V, dtype=np.uint8)
    one[V // 2] = 0
    tok, lp, sm, _ = run_select(wt, form, L, one, begin + 1, begin, eos)
    assert (tok == V // 2).all() and (lp == 0.0).all() and (sm == 0.0).all()
    # every id masked: NaN, as log_softmax of a row of -inf; the token is still the NaN-aware argmax (index 0)
    tok, lp, sm, _ = run_select(wt, form, L, np.ones(V, dtype=np.uint8), begin + 1, begin, eos)
    want_tok, _ = ref_logprob(L, np.ones(V, dtype=np.uint8), False)
    np.testing.assert_array_equal(tok, want_tok)
    assert np.isnan(lp).all()
    # a NaN: that row's entry is NaN and its token the first NaN id, the other rows are untouched
    if form == 0:
        Ln = L.copy()
        Ln[0, :] = np.nan
        tok, lp, sm, _ = run_select(wt, form, L, mask, begin + 1, begin, eos, nan_row=0)
    else:
        Ln = L.copy()
        Ln[0, 17] = np.nan
        Ln[0, V - 2] = np.nan
        tok, lp, sm, _ = run_select(wt, form, Ln, mask, begin + 1, begin, eos)
    _compare(tok, lp, sm, Ln, mask, False, f"B{B} V{V} form{form} NaN row")
    assert np.isnan(lp[0]) and not np.isnan(lp[1:]).any()
    if form == 1:   # a row whose only finite entries are masked (per-row -inf needs logits in memory)
        Lm = L.copy()
        Lm[0, :] = -np.inf
        Lm[0, sup] = 4.0
        tok, lp, sm, _ = run_select(wt, form, Lm, mask, begin + 1, begin, eos)
        _compare(tok, lp, sm, Lm, mask, False, f"B{B} V{V} form{form} finite-only-masked row")
        assert np.isnan(lp[0])


def test_forced_and_bench_eos_positions(wt):
    """A forced position scores exactly 0 whatever the logits; force_eos_step scores the step's EOS score, not the replaced argmax."""
    rng = np.random.default_rng(5)
    B, V, eos = 3, 1000, 990
    L = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    mask = np.zeros(V, dtype=np.uint8)
    for form in (0, 1):
        tok, lp, sm, _ = run_select(wt, form, L, mask, 2, 5, eos, forced=[-1, -1, 123, -1, -1, -1, -1, -1])
        assert (tok == 123).all() and (lp == 0.0).all()
        tok, lp, sm, _ = run_select(wt, form, L, mask, 2, 5, eos, step=4, force_eos_step=4)
        assert (tok == eos).all()
        s = L.astype(np.float64)
        want = s[:, eos] - (s.max(1) + np.log(np.exp(s - s.max(1, keepdims=True)).sum(1)))
        tol, _r, _f = tolerance(L, mask, False)
        assert np.abs(lp - want).max() <= tol


# ---- 3. the timestamp-mode pick ----------------------------------------------------------------------------------------------------
def ref_ts_logprob(x, ids, cur_len, no_ts, tb, tsbi, max_init, eos):
    """fp64 restatement of the timestamp rules (include/whisper_trtllm_amd.h (9b)) for one row: (token, log-probability)."""
    x = x.astype(np.float64).copy()
    if cur_len == tsbi - 1:
        return tb, 0.0
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
    lse = lambda v: (v[v > -np.inf].max() + np.log(np.exp(v[v > -np.inf] - v[v > -np.inf].max()).sum())) if (v > -np.inf).any() else -np.inf
    if lse(x[tb:]) > x[:tb].max():
        x[:tb] = -np.inf
    tok = int(np.argmax(x))
    return tok, x[tok] - lse(x)


def test_timestamp_mode_pick(wt):
    """Rule 5 fired: the softmax runs over the timestamps alone; not fired: over text and timestamps together; the forced <|0.00|>: 0."""
    rng = np.random.default_rng(9)
    V, tb, no_ts, eos, tsbi, ml = 612, 503, 502, 500, 2, 8
    B = 4
    L = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    mt = L[:, :tb].max(1)
    L[0, tb:] = -30.0
    L[0, [tb + 2, tb + 9, V - 1]] = np.float32(mt[0] + 0.5 - np.log(3.0))     # timestamp mass beats the best text id: rule 5
    L[1, tb:] = -30.0
    L[1, [tb + 2, tb + 9, V - 1]] = np.float32(mt[1] - 0.5 - np.log(3.0))     # ... loses: the merged pair, a text id wins
    L[2, tb + 4] = mt[2] + 6.0                                                # one timestamp above everything: rule 5 as well
    ids = np.full((B, ml), 10, dtype=np.int32)
    mask = np.zeros(V, dtype=np.uint8)
    mask[[5, 77]] = 1
    cur_len = 5
    tok, lp, sm, _ = run_select(wt, 2, L, mask, cur_len, -1, eos, ml=ml, ts=(no_ts, tb, tsbi, 1), ids=ids)
    Lm = L.copy()
    Lm[:, mask != 0] = -np.inf
    want = [ref_ts_logprob(Lm[b], ids[b], cur_len, no_ts, tb, tsbi, 1, eos) for b in range(B)]
    np.testing.assert_array_equal(tok, [w[0] for w in want])
    assert tok[0] >= tb and tok[1] < tb and tok[2] == tb + 4
    tol, ref_err, floor = tolerance(L, mask, False)
    err = np.abs(lp - np.array([w[1] for w in want])).max()
    print(f"timestamp pick: max error {err:.3e}, tolerance {tol:.3e} (fp32 reference error {ref_err:.3e}, floor {floor:.3e})")
    assert err <= tol
    tok, lp, sm, _ = run_select(wt, 2, L, mask, tsbi - 1, -1, eos, ml=ml, ts=(no_ts, tb, tsbi, 1), ids=ids)
    assert (tok == tb).all() and (lp == 0.0).all() and (sm == 0.0).all()


# ---- 4-6. repeatability, mode switching, refusals ----------------------------------------------------------------------------------
def test_bitwise_repeatable_and_mode_switching(wt):
    z, cfg, weights, mel = load_case("lp-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    lib, h = dec.session._lib, dec.session.handle
    plain = dec.generate(hidden)
    assert torch.is_tensor(plain)                                   # the bare ids, as before
    np.testing.assert_array_equal(plain.cpu().numpy(), z["ids"])
    ids1, s1 = dec.generate(hidden, return_logprobs=True)
    ids2, s2 = dec.generate(hidden, return_logprobs=True)
    assert s1.no_speech_prob is None
    assert torch.equal(ids1, plain) and torch.equal(ids2, plain)
    assert torch.equal(s1.token_logprobs.view(torch.int32), s2.token_logprobs.view(torch.int32))
    assert torch.equal(s1.sum_logprob.view(torch.int32), s2.sum_logprob.view(torch.int32))
    again = dec.generate(hidden)
    assert torch.is_tensor(again) and torch.equal(again, plain)
    buf, tot = torch.empty(3, cfg["max_length"], device="cuda"), torch.empty(3, device="cuda")
    rc = lib.wt_decoder_read_logprobs(h, buf.data_ptr(), cfg["max_length"], tot.data_ptr(), None, None)
    assert rc == -1, rc                                             # WT_E_STATE: the mode is off
    for name in ("qkv", "self_attn", "pair", "cross_attn", "cross_out", "fc1", "fc2"):     # the step's seven launch kinds, unchanged
        assert dec.time_kernel(name, 2) > 0.0


def test_refusals(wt):
    z, cfg, weights, mel = load_case("lp-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    lib, h = dec.session._lib, dec.session.handle
    L = wt._lib
    bad = L.LogprobParams(1, cfg["vocab_size"])
    assert lib.wt_decoder_set_logprobs(h, ctypes.byref(bad)) == -22
    bad = L.LogprobParams(1, -2)
    assert lib.wt_decoder_set_logprobs(h, ctypes.byref(bad)) == -22
    on = L.LogprobParams(1, -1)
    assert lib.wt_decoder_set_logprobs(h, ctypes.byref(on)) == 0
    p = dec._params(None, None, None)
    assert lib.wt_decoder_stream_begin(h, 2, 0, ctypes.byref(p), None) == -38
    beams = L.BeamParams(2, 1.0, 0)
    assert lib.wt_decoder_set_beam_search(h, ctypes.byref(beams)) == 0
    enc_c = hidden.contiguous()
    assert lib.wt_decoder_begin(h, enc_c.data_ptr(), 3, ctypes.byref(p), None) == -38
    assert lib.wt_decoder_set_beam_search(h, None) == 0 and lib.wt_decoder_set_logprobs(h, None) == 0
    np.testing.assert_array_equal(dec.generate(hidden).cpu().numpy(), z["ids"])     # the handle is still good


# ---- 7. the headline model's grid inside the step graph ----------------------------------------------------------------------------
def test_medium_en_batch8_against_oracle(wt):
    import cpu_ref
    cfg = wt.synthetic.get_config("whisper-medium.en")
    weights = wt.synthetic.make_weights(cfg, 77)
    mel = wt.synthetic.make_mel(cfg, index=300, batch=8)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ns = 50361
    ids, sc = dec.generate(hidden, max_length=7, return_logprobs=True, no_speech_token_id=ns)
    ids, got = ids.cpu().numpy(), sc.token_logprobs.cpu().numpy()
    W = cpu_ref.to_torch(weights)
    rows = [0, 5]
    with torch.no_grad():
        ref_ids, logits = cpu_ref.greedy_search(W, cfg, hidden[rows].cpu(), max_length=7, return_logits=True)
    np.testing.assert_array_equal(ids[rows], ref_ids.numpy())
    for t in range(1, 7):
        s = cpu_ref.apply_logits_processors(cfg, t, 1, logits[:, t - 1].clone()).double()
        want = torch.log_softmax(s, -1)[torch.arange(2), torch.from_numpy(ids[rows, t]).long()].numpy()
        assert np.abs(got[rows, t] - want).max() <= 2e-3, (t, got[rows, t], want)
    p = torch.softmax(logits[:, 0].double(), -1)[:, ns].numpy()
    assert (np.abs(sc.no_speech_prob.cpu().numpy()[rows] - p) / p).max() <= 2e-3
    assert got[:, 1].tolist() == [0.0] * 8      # the forced <|notimestamps|>


# ---- 8. run.py --return_logprobs -----------------------------------------------------------------------------------------------------
def test_run_py_return_logprobs(wt, tmp_path):
    z, cfg, weights, mel = load_case("lp-toy-short_b3")
    eng = tmp_path / "engine"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(wt.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(wt.convert.build_decoder_engine(cfg, weights))
    with open(eng / "config.pkl", "wb") as f:
        pickle.dump(cfg, f)
    ns = int(z["no_speech_token_id"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "3",
                          "--synthetic_start", str(int(z["mel_index"])), "--batching", "dataset", "--workers", "1", "--return_logprobs",
                          "--no_speech_token_id", str(ns), "--dump_ids", str(tmp_path / "ids.json")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    np.testing.assert_array_equal(np.array(json.load(open(tmp_path / "ids.json"))), z["ids"])
    lines = re.findall(r"utterance (\d+): avg_logprob (\S+)  no_speech_prob (\S+)  compression_ratio (\S+)", out.stdout)
    assert [int(l[0]) for l in lines] == [0, 1, 2], out.stdout[-2000:]
    enc, dec = _engines(wt, cfg, weights)
    _ids, sc = dec.generate(enc(torch.from_numpy(mel).cuda()), return_logprobs=True, no_speech_token_id=ns)
    assert [l[1] for l in lines] == [f"{v:.6f}" for v in sc.avg_logprob.cpu().tolist()]
    assert [l[2] for l in lines] == [f"{v:.6f}" for v in sc.no_speech_prob.cpu().tolist()]


if __name__ == "__main__":
    if sys.argv[1:] == ["--check-goldens"]:
        import whisper_trtllm_amd as _w
        for _case in LP_CASES:
            check_golden(_w, _case)
