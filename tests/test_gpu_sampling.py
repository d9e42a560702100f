"""GPU: temperature sampling on the device (wt_decoder_set_sampling; the sampling forms of the vocabulary GEMV's argmax epilogue, of
ts_select_kernel and of the finish kernels, and sample_select_kernel) -- the launches per element against an fp64 restatement
(tests/sampling_ref.py) through wt_dbg_sample_select, fused against non-fused, seed against slot, the timestamp-mode pick on crafted rows,
the engine against the reference-recorded goldens (tests/golden/make_golden_sampling.py), repeatability and mode switching, the
refusals, generate_with_fallback and run.py."""
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

import sampling_ref as ref
from conftest import load_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SM_CASES = ["sm-tiny_b2", "sm-toy-short_b3", "sm-ts-toy_b3"]


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


# ---- 1. the engine against the reference-recorded goldens ------------------------------------------------------------------------
def check_golden(wt, case):
    """ids equal; token_logprobs through each row's EOS within 2e-3 (the lp-* bound: twice the project's 1e-3 logit bound)."""
    z, cfg, weights, mel = load_case(case)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ts = bool(int(z["timestamp_mode"]))
    ids, sc = dec.generate(hidden, return_timestamps=ts, return_logprobs=True, temperature=float(z["temperature"]),
                           seeds=[int(s) for s in z["sampler_seeds"]])
    ids = ids.cpu().numpy()
    np.testing.assert_array_equal(ids, z["ids"])
    got, want = sc.token_logprobs.cpu().numpy(), z["token_logprobs"]
    eos = cfg["eos_token_id"]
    worst = 0.0
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, 1:] == eos)[0]
        last = int(hit[0]) + 1 if hit.size else ids.shape[1] - 1
        err = float(np.abs(got[b, 1:last + 1] - want[b, :last]).max())
        worst = max(worst, err)
        assert err <= 2e-3, (case, b, err)
        assert got[b, 0] == 0.0 and got[b, 1] == 0.0 and (got[b, last + 1:] == 0.0).all()
    print(f"{case}: max |token_logprob - reference| {worst:.3e}")


@pytest.mark.parametrize("case", SM_CASES)
def test_engine_matches_sampling_golden(wt, case):
    check_golden(wt, case)


def test_unfused_form_matches_sampling_goldens():
    """WT_NO_FUSED_ARGMAX=1 (latched per process): logits to memory + sample_select_kernel, same checks in a fresh process."""
    env = dict(os.environ, WT_NO_FUSED_ARGMAX="1", WT_TUNING="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--check-goldens"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.count("max |token_logprob - reference|") == len(SM_CASES)


# ---- 2. the launches per element against fp64 -------------------------------------------------------------------------------------
def tolerance(L, mask, at_begin):
    """(tests/test_gpu_logprobs.py's) 16 x the largest error of torch.log_softmax in fp32 on the CPU against fp64 on the same (processed)
    rows, floored at 4 ulp of the largest |logit|: the margin covers another summation tree and the device's expf."""
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


def key_tolerance(s_tok, T, key):
    """4 ulp of the largest of |key|, |s / T| and |g| (the division, the addition and the conversions round in fp32) + the noise's own
    error: g = -logf(-logf(u)) with u exact; a logf within 2 ulp moves the inner logarithm by 2^-22 relative, which moves g by 2^-22
    absolute, and the outer logf adds 2^-22 |g|."""
    g = key - s_tok / T
    big = max(abs(key), abs(s_tok / T), abs(g))
    return 4.0 * float(np.spacing(np.float32(big))) + 2.0 ** -22 * (1.0 + abs(g))


def processed(L, mask, at_begin):
    s = L.astype(np.float64).copy()
    s[:, (mask & 1) != 0] = -np.inf
    if at_begin:
        s[:, (mask & 2) != 0] = -np.inf
    return s


def run_sample(wt, form, L, mask, cur_len, begin_index, eos, T, seeds, ml=8, step=0, ts=None, ids=None, forced=None, nan_row=None):
    """One step through wt_dbg_sample_select.  form 0 builds the GEMV operands whose product is L exactly (X = unit rows, W[:, b] = L[b]);
    a NaN row comes from a NaN in X."""
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
    sd = (ctypes.c_uint64 * B)(*[int(s) for s in seeds])
    lp = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    sm = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    key = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.wt_dbg_sample_select_scratch_bytes(B, V, ml), dtype=torch.uint8, device=dev)
    t = wt._lib.TimestampParams(1, *ts) if ts is not None else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    rc = lib.wt_dbg_sample_select(form, ptr(X), ptr(W), K, ptr(lg), mk.data_ptr(), fo, ids_d.data_ptr(), B, V, ml, cur_len, step, begin_index, eos,
                                  -1, ctypes.byref(t) if t is not None else None, -1, float(T), sd, lp.data_ptr(), sm.data_ptr(), None,
                                  key.data_ptr(), scratch.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, wt._lib.last_error())
    return ids_d[:, cur_len].cpu().numpy(), lp.cpu().numpy(), sm.cpu().numpy(), key.cpu().numpy()


def make_inputs(B, V, rng_seed):
    rng = np.random.default_rng(rng_seed)
    scales = [1.0, 30.0, 1e-3, 1.0, 5.0, 1.0, 30.0, 1e-3]
    L = np.stack([(rng.standard_normal(V) * scales[b % len(scales)]).astype(np.float32) for b in range(B)])
    mask = np.zeros(V, dtype=np.uint8)
    mask[rng.choice(V, V // 10, replace=False)] |= 1
    mask[rng.choice(V, 5, replace=False)] |= 2
    sup, beg = int(np.nonzero(mask == 1)[0][3]), int(np.nonzero(mask == 2)[0][0])
    L[0, sup] = np.abs(L[0]).max() + 3.0            # the maximum sits on a suppressed id
    if B > 1:
        L[1, beg] = np.abs(L[1]).max() + 40.0       # ... on a begin-suppressed id
    if B > 2:
        L[2, :] = -50.0                             # all mass in the tail of the last workgroup
        L[2, V - 3:] = 20.0
        mask[V - 3:] = 0
    return L, mask


def reference_rows(L, mask, at_begin, T, seeds, t):
    s = processed(L, mask, at_begin)
    return [ref.sample_step(s[b], T, seeds[b], t) for b in range(L.shape[0])], s


@pytest.mark.parametrize("form", [0, 1], ids=["fused", "unfused"])
@pytest.mark.parametrize("T", [0.2, 1.0])
@pytest.mark.parametrize("B,V", [(1, 612), (3, 1000), (8, 51864), (16, 515), (16, 1000), (8, 612)])
def test_sample_matches_fp64(wt, B, V, T, form):
    eos, begin = V - 7, 3
    seeds = [1000 + 17 * b for b in range(B)]
    # the inputs' seed: the first whose fp64 key has a top-2 gap of at least 1e-4 x (1 + |key|) in every row, at both positions
    for rng_seed in range(1000 * B + V, 1000 * B + V + 50):
        L, mask = make_inputs(B, V, rng_seed)
        rows = {cl: reference_rows(L, mask, cl == begin, T, seeds, cl) for cl in (begin, begin + 1)}
        if all(r[3] >= 1e-4 * (1.0 + abs(r[2])) for cl in rows for r in rows[cl][0]):
            break
    for cl in (begin, begin + 1):
        want, s = rows[cl]
        for b, r in enumerate(want):
            assert r[3] >= 1e-4 * (1.0 + abs(r[2])), (rng_seed, cl, b, r)
        tok, lp, sm, key = run_sample(wt, form, L, mask, cl, begin, eos, T, seeds)
        np.testing.assert_array_equal(tok, [r[0] for r in want])
        tol, ref_err, floor = tolerance(L, mask, cl == begin)
        err = float(np.abs(lp - np.array([r[1] for r in want])).max())
        kerr = max(abs(float(key[b]) - want[b][2]) / key_tolerance(s[b, want[b][0]], T, want[b][2]) for b in range(B))
        print(f"B{B} V{V} T{T} form{form} cur_len{cl}: logprob error {err:.3e} (tolerance {tol:.3e}), key error {kerr:.3f} of its tolerance")
        assert err <= tol and kerr <= 1.0
        assert np.array_equal(sm, lp)
    if B > 2:
        assert want[2][0] >= V - 3                      # the maximum in the tail of the last workgroup
    t = begin + 1
    # one survivor among -inf: the token is the survivor, the log-probability exactly 0
    one = np.ones(V, dtype=np.uint8)
    one[V // 2] = 0
    tok, lp, sm, key = run_sample(wt, form, L, one, t, begin, eos, T, seeds)
    assert (tok == V // 2).all() and (lp == 0.0).all() and (sm == 0.0).all()
    # every id masked: NaN, the token the NaN-aware argmax of equal -inf keys (index 0)
    tok, lp, sm, key = run_sample(wt, form, L, np.ones(V, dtype=np.uint8), t, begin, eos, T, seeds)
    assert (tok == 0).all() and np.isnan(lp).all() and (key == -np.inf).all()
    # a NaN: that row's token is the first NaN id and its entry NaN, the other rows are untouched
    Ln = L.copy()
    if form == 0:
        Ln[0, :] = np.nan
        tok, lp, sm, key = run_sample(wt, form, L, mask, t, begin, eos, T, seeds, nan_row=0)
    else:
        Ln[0, 17] = np.nan
        Ln[0, V - 2] = np.nan
        tok, lp, sm, key = run_sample(wt, form, Ln, mask, t, begin, eos, T, seeds)
    want, _s = reference_rows(Ln, mask, False, T, seeds, t)
    np.testing.assert_array_equal(tok, [r[0] for r in want])
    assert np.isnan(lp[0]) and np.isnan(key[0]) and not np.isnan(lp[1:]).any()
    clean, _s = rows[t]
    np.testing.assert_array_equal(tok[1:], [r[0] for r in clean[1:]])


FORM_SHAPES = [(3, 1000), (8, 51864), (16, 515)]


def _both_forms(wt, B, V):
    L, mask = make_inputs(B, V, 77 + V)
    seeds = [5 + b for b in range(B)]
    return [(run_sample(wt, 0, L, mask, 4, 3, V - 7, T, seeds), run_sample(wt, 1, L, mask, 4, 3, V - 7, T, seeds)) for T in (0.2, 1.0)]


@pytest.mark.parametrize("B,V", FORM_SHAPES)
def test_fused_and_unfused_draw_the_same_tokens(wt, B, V):
    """Same inputs and seeds: the two forms give equal tokens and bitwise equal winning keys."""
    for a, b in _both_forms(wt, B, V):
        np.testing.assert_array_equal(a[0], b[0])
        assert np.array_equal(a[3].view(np.int32), b[3].view(np.int32))


@pytest.mark.parametrize("B,V", FORM_SHAPES)
def test_fused_and_unfused_logprobs_are_bitwise_equal(wt, B, V):
    """Same inputs and seeds: bitwise equal log-probabilities.  The numerator s[tok] is the same float in both forms, and
    sample_select_kernel accumulates the log-sum-exp pairs in the partition and order of the GEMV's sampling epilogue, so the denominator
    is too.  (Summed over greedy_select_kernel's eight chunks instead, 3 of 16 rows of (16, 515) differed, by up to 6 ulp.)"""
    for a, b in _both_forms(wt, B, V):
        diff = np.abs(a[1].view(np.int32).astype(np.int64) - b[1].view(np.int32).astype(np.int64))
        print(f"B{B} V{V}: rows that differ {int((diff != 0).sum())}, largest distance {int(diff.max())} ulp")
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_draw_depends_on_the_seed_not_on_the_slot(wt):
    rng = np.random.default_rng(3)
    V, T = 1000, 1.0
    row = (rng.standard_normal(V) * 2).astype(np.float32)
    mask = np.zeros(V, dtype=np.uint8)
    L16 = (rng.standard_normal((16, V)) * 2).astype(np.float32)
    L16[11] = row
    for form in (0, 1):
        one = run_sample(wt, form, row[None], mask, 4, 3, V - 7, T, [42])
        many = run_sample(wt, form, L16, mask, 4, 3, V - 7, T, [100 + b if b != 11 else 42 for b in range(16)])
        assert one[0][0] == many[0][11] and one[3][0].view(np.int32) == many[3][11].view(np.int32)
    same = np.stack([row, row])
    differ = 0
    for pos in range(1, 65):      # 64 positions of two identical rows with two seeds
        tok, _lp, _sm, _key = run_sample(wt, 1, same, mask, pos, 3, V - 7, T, [1, 2], ml=66)
        differ += int(tok[0] != tok[1])
    assert differ > 0


# ---- 3. the timestamp-mode pick ----------------------------------------------------------------------------------------------------
def ref_ts_sample(x, ids, cur_len, no_ts, tb, tsbi, max_init, eos, T, seed):
    """fp64 restatement of the timestamp rules over the unperturbed scores, then the Gumbel-max draw among the survivors."""
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
    tok = ref.nan_argmax(ref.keys(x, T, seed, cur_len))
    return tok, x[tok] - lse(x)


def test_timestamp_mode_pick(wt):
    """Rule 2 still yields <|0.00|>; when rule 5 fires the token is a timestamp even if a text id has the best key; otherwise the token
    is the best key of the union; the log-probability's denominator is that of the log-probability mode."""
    rng = np.random.default_rng(9)
    V, tb, no_ts, eos, tsbi, ml = 612, 503, 502, 500, 2, 8
    B, T = 4, 1.0
    L = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    mt = L[:, :tb].max(1)
    L[0, tb:] = -30.0
    L[0, [tb + 2, tb + 9, V - 1]] = np.float32(mt[0] + 0.5 - np.log(3.0))     # timestamp mass beats the best text id: rule 5
    L[1, tb:] = -30.0
    L[1, [tb + 2, tb + 9, V - 1]] = np.float32(mt[1] - 0.5 - np.log(3.0))     # ... loses: text and timestamps compete by key
    L[2, tb + 4] = mt[2] + 6.0                                                # one timestamp above everything: rule 5 as well
    ids = np.full((B, ml), 10, dtype=np.int32)
    mask = np.zeros(V, dtype=np.uint8)
    mask[[5, 77]] = 1
    cur_len = 5
    Lm = L.copy()
    Lm[:, mask != 0] = -np.inf
    # a seed for row 0 under which a TEXT id holds the best key of the whole row although rule 5 masks the text
    seed0 = next(s for s in range(1, 500) if ref.nan_argmax(ref.keys(np.where(np.arange(V) == no_ts, -np.inf, Lm[0]), T, s, cur_len)) < tb)
    seeds = [seed0, 21, 22, 23]
    tok, lp, sm, key = run_sample(wt, 1, L, mask, cur_len, -1, eos, T, seeds, ml=ml, ts=(no_ts, tb, tsbi, 1), ids=ids)
    want = [ref_ts_sample(Lm[b], ids[b], cur_len, no_ts, tb, tsbi, 1, eos, T, seeds[b]) for b in range(B)]
    np.testing.assert_array_equal(tok, [w[0] for w in want])
    assert tok[0] >= tb and tok[2] >= tb
    union = [ref.nan_argmax(ref.keys(np.where(np.arange(V) == no_ts, -np.inf, Lm[b]), T, seeds[b], cur_len)) for b in (1, 3)]
    assert [tok[1], tok[3]] == union
    tol, ref_err, floor = tolerance(L, mask, False)
    err = np.abs(lp - np.array([w[1] for w in want])).max()
    print(f"timestamp pick: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    tok, lp, sm, key = run_sample(wt, 1, L, mask, tsbi - 1, -1, eos, T, seeds, ml=ml, ts=(no_ts, tb, tsbi, 1), ids=ids)
    assert (tok == tb).all() and (lp == 0.0).all() and (sm == 0.0).all()


# ---- 4-5. determinism, switching, refusals ------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_mode_switching(wt):
    z, cfg, weights, mel = load_case("sm-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    T, seeds = float(z["temperature"]), [int(s) for s in z["sampler_seeds"]]
    fresh = _engines(wt, cfg, weights)[1].generate(hidden)
    ids1, s1 = dec.generate(hidden, return_logprobs=True, temperature=T, seeds=seeds)
    greedy = dec.generate(hidden)
    ids2, s2 = dec.generate(hidden, return_logprobs=True, temperature=T, seeds=seeds)
    assert torch.equal(ids1, ids2) and torch.equal(s1.token_logprobs.view(torch.int32), s2.token_logprobs.view(torch.int32))
    np.testing.assert_array_equal(ids1.cpu().numpy(), z["ids"])
    assert torch.equal(greedy, fresh)
    bare = dec.generate(hidden, temperature=T, seeds=seeds)           # without return_logprobs: the bare ids
    assert torch.is_tensor(bare) and torch.equal(bare, ids1)
    # temperature = 0 and the mode off enqueue the same kernels: ids and, with profiling on, the per-kernel launch counts
    counts = []
    for kw in ({}, {"temperature": 0.0, "seed": 9}):
        other = _engines(wt, cfg, weights)[1]
        other.set_profiling(True)
        ids = other.generate(hidden, **kw)
        assert torch.equal(ids, fresh)
        counts.append({name: other.timer(name)[1] for name in ("dec_cross_attn", "vocab_proj")})
    assert counts[0] == counts[1] and counts[0]["vocab_proj"] > 0, counts


def test_refusals(wt):
    z, cfg, weights, mel = load_case("sm-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    lib, h = dec.session._lib, dec.session.handle
    L = wt._lib
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert lib.wt_decoder_set_sampling(h, ctypes.byref(L.SamplingParams(bad, None, 0, 0))) == -22
    two = (ctypes.c_uint64 * 2)(1, 2)
    few = L.SamplingParams(0.5, ctypes.cast(two, ctypes.POINTER(ctypes.c_uint64)), 2, 0)
    assert lib.wt_decoder_set_sampling(h, ctypes.byref(few)) == 0
    p = dec._params(None, None, None)
    enc_c = hidden.contiguous()
    assert lib.wt_decoder_begin(h, enc_c.data_ptr(), 3, ctypes.byref(p), None) == -22        # two seeds, three rows
    on = L.SamplingParams(0.5, None, 0, 7)
    assert lib.wt_decoder_set_sampling(h, ctypes.byref(on)) == 0
    assert lib.wt_decoder_stream_begin(h, 2, 0, ctypes.byref(p), None) == -38
    beams = L.BeamParams(2, 1.0, 0)
    assert lib.wt_decoder_set_beam_search(h, ctypes.byref(beams)) == 0
    assert lib.wt_decoder_begin(h, enc_c.data_ptr(), 3, ctypes.byref(p), None) == -38
    assert lib.wt_decoder_set_beam_search(h, None) == 0 and lib.wt_decoder_set_sampling(h, None) == 0
    greedy = np.load(os.path.join(ROOT, "tests", "golden", "lp-toy-short_b3.npz"))["ids"]
    np.testing.assert_array_equal(dec.generate(hidden).cpu().numpy(), greedy)                  # the handle is still good


# ---- 6. generate_with_fallback --------------------------------------------------------------------------------------------------------
def test_generate_with_fallback_on_a_toy_model(wt):
    z, cfg, weights, mel = load_case("sm-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    _ids, g = dec.generate(hidden, return_logprobs=True)
    avg = g.avg_logprob.cpu().numpy()
    order = np.argsort(avg)
    thr = float((avg[order[0]] + avg[order[1]]) / 2)      # above the lowest row's greedy avg_logprob, below the others'
    temps = (0.0, 1.0)
    ids, sc, used = dec.generate_with_fallback(hidden, temperatures=temps, compression_ratio_threshold=None, logprob_threshold=thr,
                                               no_speech_threshold=None, seed=40)
    used = used.cpu().numpy()
    failing = [int(order[0])]
    assert [b for b in range(3) if used[b] > 0] == failing
    for b in range(3):
        kw = {"temperature": float(used[b]), "seeds": [40 + b]} if used[b] > 0 else {}
        alone, s = dec.generate(hidden[b:b + 1], return_logprobs=True, **kw)
        n = alone.shape[1]
        assert torch.equal(ids[b, :n], alone[0]) and (ids[b, n:] == cfg["pad_token_id"]).all()
        assert torch.equal(sc.token_logprobs[b, :n].view(torch.int32), s.token_logprobs[0].view(torch.int32))
        assert sc.sum_logprob[b].item() == s.sum_logprob[0].item()


def test_run_py_sampling_and_fallback(wt, tmp_path):
    z, cfg, weights, mel = load_case("sm-toy-short_b3")
    eng = tmp_path / "engine"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(wt.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(wt.convert.build_decoder_engine(cfg, weights))
    with open(eng / "config.pkl", "wb") as f:
        pickle.dump(cfg, f)
    base = [sys.executable, os.path.join(ROOT, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "3",
            "--synthetic_start", str(int(z["mel_index"])), "--batching", "dataset", "--workers", "1"]
    for extra in (["--temperature", "0.6", "--seed", "3"], ["--temperature_fallback"]):
        got = []
        for k in range(2):
            path = tmp_path / f"ids{k}.json"
            out = subprocess.run(base + extra + ["--dump_ids", str(path)], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr[-2000:]
            got.append(json.load(open(path)))
            lines = re.findall(r"utterance (\d+): avg_logprob (\S+)  no_speech_prob (\S+)  compression_ratio (\S+)  temperature (\S+)", out.stdout)
            assert [int(l[0]) for l in lines] == [0, 1, 2], out.stdout[-2000:]
        assert got[0] == got[1]


if __name__ == "__main__":
    if sys.argv[1:] == ["--check-goldens"]:
        import whisper_trtllm_amd as _w
        for _case in SM_CASES:
            check_golden(_w, _case)
