"""GPU: language detection and per-utterance language tokens (wt_decoder_set_languages, generate(language=...), detect_language).

1. Against the lg-* goldens (tests/golden/make_golden_language.py: detect_language restated on the reference model, then the reference's
   greedy_search at batch 1 per row with the detected language forced): detected ids equal, log(prob) within 2e-3 (the project's bound for
   log-probabilities against reference goldens), the ids of the mixed-language batch equal the per-row goldens, token log-probabilities
   within 2e-3 and exactly 0 at the language position; the same in a fresh process without the fused argmax.
2. lang_select_kernel per element against fp64 through wt_dbg_lang_select, which builds the launch with the engine's own helper.
3. Properties, with the path that existed before (the language in the CONFIG's forced list) as the yardstick.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_case
import longform_language_ref

pytestmark = pytest.mark.gpu
LG_CASES = ["lg-tiny_b2", "lg-toy-short_b3", "lg-ts-toy_b3"]
U = 2.0 ** -24    # unit roundoff of fp32


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _case(case, precision="float32"):
    return _build(case, precision)


@functools.lru_cache(maxsize=None)
def _build(case, precision):
    """(golden, cfg, encoder engine, decoder engine, encoder output on the GPU): built once per case, never modified."""
    import whisper_trtllm_amd as w
    z, cfg, weights, mel = load_case(case)
    enc = w.WhisperEncoderEngine(w.convert.build_encoder_engine(cfg, weights))
    dec = w.WhisperDecoderEngine(w.convert.build_decoder_engine(cfg, weights, precision=precision), cfg)
    return z, cfg, enc, dec, enc(torch.from_numpy(mel).cuda())


def _view(dec, lang):
    """The same engine under a config with `lang` at forced position 1: the batch-wide forced id, the path before per-row languages."""
    import whisper_trtllm_amd as w
    return longform_language_ref.language_view(w, dec, lang)


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------
def check_golden(case):
    """Returns what the fused / unfused A/B compares bitwise: (ids, language ids, language probabilities)."""
    z, cfg, enc, dec, hidden = _case(case)
    ts = bool(int(z["timestamp_mode"]))
    B = int(z["batch"])
    assert list(z["language_ids"]) == cfg["language_ids"] and len(set(z["lang_detected"].tolist())) > 1   # a mixed-language batch
    tok, probs = dec.detect_language(hidden)
    np.testing.assert_array_equal(tok.cpu().numpy(), z["lang_detected"])
    lerr = np.abs(np.log(probs.cpu().numpy().astype(np.float64)) - np.log(z["lang_probs"])).max()
    ids, sc, langs = dec.generate(hidden, language="auto", return_logprobs=True, return_timestamps=ts)
    got, lp = ids.cpu().numpy(), sc.token_logprobs.cpu().numpy()
    assert torch.equal(langs.ids, tok) and torch.equal(langs.probs, probs)       # the decode's first step IS the detection
    assert abs(float(probs.sum(1).max()) - 1) < 1e-5
    np.testing.assert_array_equal(langs.prob_of_ids().cpu().numpy(), probs.max(1).values.cpu().numpy())
    worst = 0.0
    for b in range(B):                                    # every row against ITS batch-1 golden
        n = int(z["row_len"][b])
        np.testing.assert_array_equal(got[b, :n], z["ids"][b, :n])
        assert (got[b, n:] == cfg["pad_token_id"]).all() and got[b, 1] == z["lang_detected"][b]
        worst = max(worst, float(np.abs(lp[b, 1:n] - z["token_logprobs"][b, :n - 1]).max()))
        assert lp[b, 0] == 0.0 and lp[b, 1] == 0.0 and lp[b, 2] == 0.0           # start, language position, task: exactly 0
    print(f"{case}: max |log(language prob) - reference| {lerr:.3e}, max |token_logprob - reference| {worst:.3e}")
    assert lerr <= 2e-3 and worst <= 2e-3, (case, lerr, worst)
    return got, tok.cpu().numpy(), probs.cpu().numpy()


@pytest.mark.parametrize("case", LG_CASES)
def test_engine_matches_language_golden(wt, case):
    check_golden(case)


def test_unfused_form_matches_goldens_and_agrees_bitwise(wt, tmp_path):
    """WT_NO_FUSED_ARGMAX=1 (latched per process): logits to memory + the select kernels, the same checks in a fresh process.  What the
    language rule touches agrees bitwise between the two forms: the ids, the language tokens and their probabilities (the token
    log-probabilities come from different partial sums in the two forms, and are held to the goldens' bound in both)."""
    env = dict(os.environ, WT_NO_FUSED_ARGMAX="1", WT_TUNING="1")
    dump = str(tmp_path / "unfused.npz")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--check-goldens", dump], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.count("max |token_logprob - reference|") == len(LG_CASES)
    other = np.load(dump)
    for case in LG_CASES:
        for name, mine in zip(("ids", "tok", "probs"), check_golden(case)):
            assert mine.tobytes() == other[f"{case}.{name}"].tobytes(), (case, name)


@pytest.mark.parametrize("case", ["lg-toy-short_b3", "lg-ts-toy_b3"])
def test_ragged_prompts_lengths_5_0_2(wt, case):
    """Per-row prompts of 5 / 0 / 2 tokens: the language position is Lmax + 1 for every row.  The row without a prompt detects what the
    golden says; every row's language is the argmax of the step's own raw logits at the language ids (the vocabulary projection's, taken
    through logits_trace); and the rows decode bitwise what the same ragged batch decodes with their language as the batch-wide forced id."""
    z, cfg, enc, dec, hidden = _case(case)
    ts = bool(int(z["timestamp_mode"]))
    lang_ids = cfg["language_ids"]
    prompts = [[9, 40, 41, 42, 43], [], [9, 50]]
    L, ml = 5, cfg["max_length"] + 5
    ids, sc, langs = dec.generate(hidden, prompts=prompts, language="auto", return_logprobs=True, return_timestamps=ts, max_length=ml)
    tok = langs.ids.cpu().numpy()
    assert tok[1] == z["lang_detected"][1]
    assert np.abs(np.log(langs.probs[1].cpu().numpy().astype(np.float64)) - np.log(z["lang_probs"][1])).max() <= 2e-3
    assert torch.equal(ids[:, L + 1], langs.ids) and (ids[:, L] == cfg["decoder_start_token_id"]).all()
    assert (sc.token_logprobs[:, :L + 2] == 0).all() and sc.prompt_len == L
    n = int(z["row_len"][1])
    assert wt.runtime.strip_prompts(ids.cpu(), L)[1][:n] == z["ids"][1, :n].tolist()
    # the step's raw logits as the vocabulary projection computes them: another summation order of the same fp32 quantity
    trace = torch.full((3, ml - 1, cfg["vocab_size"]), float("nan"), device="cuda")
    _view(dec, lang_ids[0]).generate(hidden, prompts=prompts, logits_trace=trace, return_timestamps=ts, max_length=ml)
    raw = trace[:, 0].cpu().numpy().astype(np.float64)[:, lang_ids]
    want = np.exp(raw - raw.max(1, keepdims=True))
    want /= want.sum(1, keepdims=True)
    margin = np.sort(raw, 1)[:, -1] - np.sort(raw, 1)[:, -2]
    err = np.abs(np.log(langs.probs.cpu().numpy().astype(np.float64)) - np.log(want)).max()
    print(f"{case}: behind prompts 5 / 0 / 2 detected {tok.tolist()}, |log prob - vocabulary projection's| {err:.2e}, top-2 margins {margin.round(4).tolist()}")
    assert err <= 2e-3
    for b in range(3):
        if margin[b] > 1e-3:
            assert tok[b] == lang_ids[int(raw[b].argmax())]
    for lang in sorted(set(tok.tolist())):
        ref_ids, ref_sc = _view(dec, lang).generate(hidden, prompts=prompts, return_logprobs=True, return_timestamps=ts, max_length=ml)
        rows = torch.as_tensor(tok == lang, device="cuda")
        assert torch.equal(ids[rows], ref_ids[rows]) and torch.equal(sc.token_logprobs[rows], ref_sc.token_logprobs[rows])


# ---- 2. lang_select_kernel per element ------------------------------------------------------------------------------------------------
V_DBG = 257


def _inputs(d, n_lang, B, seed, half=False):
    """x [B][d], LayerNorm weights, an embedding table [V][d] and `n_lang` unsorted ids that hold 0 and V - 1 where they fit."""
    g = np.random.default_rng([seed, d, n_lang, B])
    x = (g.standard_normal((B, d)) * 1.5 + 0.3).astype(np.float32)
    ln_w = (1 + 0.1 * g.standard_normal(d)).astype(np.float32)
    ln_b = (0.1 * g.standard_normal(d)).astype(np.float32)
    emb = (0.12 * g.standard_normal((V_DBG, d))).astype(np.float32)
    if half:
        emb = emb.astype(np.float16)
    ids = g.permutation(np.arange(1, V_DBG - 1))[:n_lang]
    ids[0] = V_DBG - 1
    if n_lang >= 2:
        ids[-1] = 0
    return x, ln_w, ln_b, emb, [int(i) for i in ids]


def _run(wt, x, ln_w, ln_b, emb, ids, preset=None):
    """wt_dbg_lang_select on these inputs -> (lang_tok [B], lang_prob [B][n_lang]) as numpy."""
    lib = wt._lib.load()
    B, d = x.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, wd, bd, ed = dev(x), dev(ln_w), dev(ln_b), dev(emb)
    tok = torch.full((B,), -1, dtype=torch.int32, device="cuda") if preset is None else torch.tensor(preset, dtype=torch.int32, device="cuda")
    prob = torch.full((B, len(ids)), -7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.wt_dbg_lang_select_scratch_bytes(), dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_int32 * len(ids))(*ids)
    rc = lib.wt_dbg_lang_select(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), ed.data_ptr(), int(emb.dtype == np.float16), arr, len(ids), emb.shape[0],
                                B, d, tok.data_ptr(), prob.data_ptr(), scratch.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tok.cpu().numpy(), prob.cpu().numpy()


def _reference(x, ln_w, ln_b, emb, ids):
    """fp64 from the same inputs: (logits z [B][n], softmax, per-logit error bound of the fp32 kernel).
    Bound, with u = 2^-24, c = ceil(d / 256) chunks per lane and xn = (x - mean) rstd g + b.  The kernel's sums are blocked: inside a
    lane c partial terms, then a 6-level exchange over the wave -- a sum of the statistics rounds at most ks = c + 9 times on any path
    (2 inside a float4, c accumulations, 6 levels, 1 spare), a dot product at most kd = c + 10 times (4 in the fmaf chain), and a blocked
    sum of depth k errs by at most (k + 1) u sum|terms|.  So the mean errs by (ks + 1) u mean|x|, rstd relatively by ((ks + 3) / 2 + 3) u
    (the variance's sum, its division, the added epsilon, rsqrtf), and the affine map adds 4 u:
        |xn_k - xn64_k| <= u [((ks + 3) / 2 + 7) (|xn_k| + |b_k|) + (ks + 1) mean|x| rstd |g_k|]
        |z - z64|       <= u [((ks + 3) / 2 + 7 + kd + 1) A + (ks + 1) mean|x| rstd G],   A = sum_k (|xn_k| + |b_k|) |E_k|,   G = sum_k |g_k E_k|."""
    x64, g64, b64 = x.astype(np.float64), ln_w.astype(np.float64), ln_b.astype(np.float64)
    E = emb.astype(np.float64)[ids]                                            # [n][d]
    d = x.shape[1]
    mean = x64.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x64 - mean) ** 2).mean(1, keepdims=True) + 1e-5)
    xn = (x64 - mean) * rstd * g64 + b64
    z = xn @ E.T
    A = (np.abs(xn) + np.abs(b64)) @ np.abs(E).T
    G = (np.abs(g64)[None, :] * np.abs(E)).sum(1)[None, :]
    c = -(-d // 256)
    ks, kd = c + 9, c + 10
    bz = U * (((ks + 3) / 2 + 7 + kd + 1) * A + (ks + 1) * np.abs(x64).mean(1, keepdims=True) * rstd * G)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - np.nanmax(z, 1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
    return z, p, bz


def _check(tok, prob, z, p, bz, ids):
    """Probabilities: p_l = exp(z_l - m) / sum.  The relative error of exp(z_l - m) is at most 2 max(bz) (both logits moved) +
    u |z_l - m| (the subtraction) + 2 u (expf), the sum of n terms adds n u and the division u:
        |p - p64| <= p64 (2 max bz + u (|z - m| + n + 4)) + 2^-126   (the floor: results below the normal range)."""
    n = len(ids)
    rel = 2 * bz.max(1, keepdims=True) + U * (np.abs(z - z.max(1, keepdims=True)) + n + 4)
    err = np.abs(prob.astype(np.float64) - p)
    assert (err <= p * rel + 2.0 ** -126).all(), (float((err / (p * rel + 2.0 ** -126)).max()), float(rel.max()))
    order = np.sort(z, 1)
    for b in range(z.shape[0]):          # the winner: decided where the fp64 margin exceeds both logits' bounds
        if n == 1 or order[b, -1] - order[b, -2] > 2 * bz[b].max():
            assert tok[b] == ids[int(z[b].argmax())], (b, tok[b])
        assert tok[b] in ids
    return float((err / (p * rel + 2.0 ** -126)).max())


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("n_lang", [1, 2, 7, 99, 128])
@pytest.mark.parametrize("d", [64, 384, 1280])
def test_lang_select_per_element(wt, d, n_lang, B):
    x, ln_w, ln_b, emb, ids = _inputs(d, n_lang, B, 1)
    assert V_DBG - 1 in ids and (n_lang == 1 or (0 in ids and ids != sorted(ids)))
    tok, prob = _run(wt, x, ln_w, ln_b, emb, ids)
    z, p, bz = _reference(x, ln_w, ln_b, emb, ids)
    ratio = _check(tok, prob, z, p, bz, ids)
    print(f"d {d} n_lang {n_lang} B {B}: worst error / bound {ratio:.3f}, logit bound {bz.max():.2e}")
    assert np.abs(prob.sum(1) - 1).max() <= (n_lang + 4) * 2 * U


@pytest.mark.parametrize("d", [64, 384, 1280])
def test_lang_select_half_weights(wt, d):
    """The fp16 `w_half` form of the table: the reference widens the same half values, the arithmetic (and the bound) stays fp32's."""
    x, ln_w, ln_b, emb, ids = _inputs(d, 7, 3, 2, half=True)
    tok, prob = _run(wt, x, ln_w, ln_b, emb, ids)
    _check(tok, prob, *_reference(x, ln_w, ln_b, emb, ids), ids)


def test_lang_select_wide_logits_do_not_overflow(wt):
    """Logits spread over +-1e4: the maximum is subtracted, nothing overflows, the probabilities sum to 1 and the winner takes it all."""
    d, n = 384, 99
    x, ln_w, ln_b, emb, ids = _inputs(d, n, 3, 3)
    z0 = _reference(x, ln_w, ln_b, emb, ids)[0]
    xn = _reference(x, ln_w, ln_b, np.eye(d, dtype=np.float32), list(range(d)))[0]      # the normalised rows themselves
    unit = xn[0] / (xn[0] @ xn[0])
    emb = emb.copy()
    for k, i in enumerate(ids):           # row 0's logits: -1e4 .. 1e4 in steps of ~200, in a shuffled order
        emb[i] = (unit * (-1e4 + 2e4 * ((k * 37) % n) / (n - 1))).astype(np.float32)
    tok, prob = _run(wt, x, ln_w, ln_b, emb, ids)
    z, p, bz = _reference(x, ln_w, ln_b, emb, ids)
    assert z[0].max() > 9.9e3 and z[0].min() < -9.9e3 and np.abs(z0).max() < 100
    assert np.isfinite(prob).all() and np.abs(prob.sum(1) - 1).max() <= (n + 4) * 2 * U
    assert bz[0].max() < 5 and tok[0] == ids[int(z[0].argmax())] and prob[0].max() == 1.0    # (steps of 200 >> the logit bound)
    _check(tok, prob, z, p, bz, ids)


def test_lang_select_equal_rows_go_to_the_lowest_id(wt):
    """Two identical embedding rows give bitwise equal logits: torch.argmax over the masked vocabulary returns the lower TOKEN ID,
    wherever the two stand in the list."""
    d = 384
    x, ln_w, ln_b, emb, ids = _inputs(d, 7, 3, 4)
    xn = _reference(x, ln_w, ln_b, np.eye(d, dtype=np.float32), list(range(d)))[0]      # the normalised rows themselves
    free = [v for v in range(1, V_DBG - 1) if v not in ids]
    lo, hi = free[0], free[-1]
    for lo_first in (False, True):
        e2, i2 = emb.copy(), list(ids)
        i2[1], i2[5] = (lo, hi) if lo_first else (hi, lo)
        e2[lo] = e2[hi] = (30 * xn[0] / (xn[0] @ xn[0])).astype(np.float32)      # row 0's logit there: 30, far above the others
        tok, prob = _run(wt, x, ln_w, ln_b, e2, i2)
        assert tok[0] == lo and prob[0, 1] == prob[0, 5] and abs(prob[0, 1] - 0.5) < 1e-6


def test_lang_select_nan_row_and_neighbours(wt):
    """A NaN row: NaN probabilities and the lowest listed id (torch.argmax: the first NaN of the masked vocabulary); the other rows are
    bitwise what they are without it."""
    x, ln_w, ln_b, emb, ids = _inputs(384, 7, 3, 5)
    tok0, prob0 = _run(wt, x, ln_w, ln_b, emb, ids)
    bad = x.copy()
    bad[1, 17] = np.nan
    tok, prob = _run(wt, bad, ln_w, ln_b, emb, ids)
    assert np.isnan(prob[1]).all() and tok[1] == min(ids)
    for b in (0, 2):
        assert tok[b] == tok0[b] and prob[b].tobytes() == prob0[b].tobytes()
    e2 = emb.copy()                       # one NaN logit among numbers: NaN wins, as in torch.argmax
    e2[ids[3], 5] = np.nan
    tok, prob = _run(wt, x, ln_w, ln_b, e2, ids)
    assert (tok == ids[3]).all() and np.isnan(prob).all()


def test_lang_select_keeps_a_preset_row_and_rows_do_not_depend_on_the_batch(wt):
    x, ln_w, ln_b, emb, ids = _inputs(1280, 99, 16, 6)
    tok, prob = _run(wt, x, ln_w, ln_b, emb, ids)
    preset = [-1] * 16
    preset[4], preset[9] = ids[0], ids[98]
    tok2, prob2 = _run(wt, x, ln_w, ln_b, emb, ids, preset)
    assert tok2[4] == ids[0] and tok2[9] == ids[98] and prob2.tobytes() == prob.tobytes()      # kept; the probabilities still written
    assert all(tok2[b] == tok[b] for b in range(16) if b not in (4, 9))
    for b in (0, 7, 15):                  # row b of B = 16 is bitwise the row run alone
        t1, p1 = _run(wt, x[b:b + 1], ln_w, ln_b, emb, ids)
        assert t1[0] == tok[b] and p1[0].tobytes() == prob[b].tobytes()


def test_lang_select_refuses_bad_shapes(wt):
    x, ln_w, ln_b, emb, ids = _inputs(64, 2, 1, 7)
    lib = wt._lib.load()
    dev = lambda a: torch.from_numpy(a).cuda()
    xd, wd, bd, ed = dev(x), dev(ln_w), dev(ln_b), dev(emb)
    tok, prob = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, 2, device="cuda")
    scratch = torch.empty(lib.wt_dbg_lang_select_scratch_bytes(), dtype=torch.uint8, device="cuda")
    call = lambda ids, n, V, B, d: lib.wt_dbg_lang_select(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), ed.data_ptr(), 0, (ctypes.c_int32 * 130)(*ids), n, V,
                                                          B, d, tok.data_ptr(), prob.data_ptr(), scratch.data_ptr(), None)
    assert call(ids, 2, V_DBG, 1, 64) == 0
    for bad in ((ids, 0, V_DBG, 1, 64), (list(range(129)), 129, V_DBG, 1, 64), ([0, V_DBG], 2, V_DBG, 1, 64), ([0, -1], 2, V_DBG, 1, 64),
                (ids, 2, V_DBG, 17, 64), (ids, 2, V_DBG, 1, 62), (ids, 2, V_DBG, 1, 1284)):
        assert call(*bad) == -22, bad
    torch.cuda.synchronize()


# ---- 3. properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,precision", [("lg-toy-short_b3", "float32"), ("lg-toy-short_b3", "float16"), ("lg-ts-toy_b3", "float32")])
def test_per_row_languages_equal_the_forced_list_path(wt, case, precision):
    """A per-row language list decodes, row by row, bitwise what the same batch decodes with that language as the config's batch-wide
    forced id: ids and log-probabilities.  (Each row alone at batch 1: the goldens of part 1.)"""
    z, cfg, enc, dec, hidden = _case(case, precision)
    ts = bool(int(z["timestamp_mode"]))
    lang_ids = cfg["language_ids"]
    want = [lang_ids[3], lang_ids[0], lang_ids[-1]]
    ids, sc, langs = dec.generate(hidden, language=want, return_logprobs=True, return_timestamps=ts)
    assert langs.ids.cpu().tolist() == want and ids[:, 1].cpu().tolist() == want and (sc.token_logprobs[:, 1] == 0).all()
    assert (langs.probs == 0).all()                       # no row was left to detect: no kernel ran
    for b, lang in enumerate(want):
        ref_ids, ref_sc = _view(dec, lang).generate(hidden, return_logprobs=True, return_timestamps=ts)
        assert torch.equal(ids[b], ref_ids[b]) and torch.equal(sc.token_logprobs[b], ref_sc.token_logprobs[b]), b
        assert sc.sum_logprob[b] == ref_sc.sum_logprob[b]
    mixed = dec.generate(hidden, language=[want[0], "auto", want[2]], return_timestamps=ts)      # chosen rows beside a detected one
    found = mixed[1].ids.cpu().tolist()
    assert found[0] == want[0] and found[2] == want[2] and found[1] in lang_ids
    if precision == "float32":
        assert found[1] == int(z["lang_detected"][1])
    assert (mixed[1].probs.sum(1) - 1).abs().max() < 1e-5                                      # ... every row still gets its probabilities
    assert torch.equal(mixed[0][0], ids[0]) and torch.equal(mixed[0][2], ids[2])


@pytest.mark.parametrize("case,precision", [("lg-toy-short_b3", "float32"), ("lg-tiny_b2", "float16")])
def test_auto_equals_detect_then_language(wt, case, precision):
    z, cfg, enc, dec, hidden = _case(case, precision)
    tok, probs = dec.detect_language(hidden)
    a_ids, a_sc, a_l = dec.generate(hidden, language="auto", return_logprobs=True)
    b_ids, b_sc, b_l = dec.generate(hidden, language=tok.cpu().tolist(), return_logprobs=True)
    assert torch.equal(a_l.ids, tok) and torch.equal(a_l.probs, probs) and torch.equal(b_l.ids, tok)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc.token_logprobs, b_sc.token_logprobs) and torch.equal(a_sc.sum_logprob, b_sc.sum_logprob)
    c_ids, _c_sc, temps, c_l = dec.generate_with_fallback(hidden, temperatures=(0.0,), language="auto")
    assert torch.equal(c_ids, a_ids) and torch.equal(c_l.ids, tok) and (temps == 0).all()


def test_mode_off_is_bitwise_the_decode_that_never_mentions_it(wt):
    z, cfg, enc, dec, hidden = _case("lg-toy-short_b3")
    fresh = wt.WhisperDecoderEngine(None, cfg, _session=dec.session.clone())
    ids0, sc0 = fresh.generate(hidden, return_logprobs=True)
    captures = wt._lib.load().wt_dbg_step_graph_captures(fresh.session.handle)
    fresh.generate(hidden, language="auto")
    ids1, sc1 = fresh.generate(hidden, return_logprobs=True)
    assert torch.equal(ids0, ids1) and torch.equal(sc0.token_logprobs, sc1.token_logprobs) and torch.equal(sc0.sum_logprob, sc1.sum_logprob)
    assert ids0[0, 1] == cfg["forced_decoder_ids"][0][1]
    with pytest.raises(RuntimeError):     # no language decode in flight any more
        fresh.read_languages()
    # a caller-chosen list runs no detection: one step graph, as the decode without the mode captured
    before = wt._lib.load().wt_dbg_step_graph_captures(fresh.session.handle)
    fresh.generate(hidden, language=[cfg["language_ids"][0]] * 3, return_logprobs=True)
    assert wt._lib.load().wt_dbg_step_graph_captures(fresh.session.handle) - before == captures


def test_refused_combinations_raise(wt):
    z, cfg, enc, dec, hidden = _case("lg-toy-short_b3")
    lang = cfg["language_ids"]
    for bad in (dict(language="auto", num_beams=2), dict(language="auto", return_token_timestamps=True, alignment_heads=[(0, 0)]),
                dict(language=5), dict(language=["auto", "auto"]), dict(language="en"), dict(task="transcribe"), dict(task=-1)):
        with pytest.raises(ValueError):
            dec.generate(hidden, **bad)
    en = wt.WhisperDecoderEngine(None, dict(cfg, forced_decoder_ids=[[1, 510]]), _session=dec.session)     # a .en-style list: no language slot
    with pytest.raises(ValueError):
        en.generate(hidden, language="auto")
    with pytest.raises(ValueError):
        en.detect_language(hidden)
    # the C-ABI itself
    dec.begin(hidden)                     # every mode of an earlier decode on this handle off
    lib, h = wt._lib.load(), dec.session.handle
    L = wt._lib
    I32 = ctypes.POINTER(ctypes.c_int32)
    arr = lambda v: ctypes.cast((ctypes.c_int32 * max(len(v), 1))(*v), I32)
    p = dec._params(None, None, None)
    begin = lambda: lib.wt_decoder_begin(h, hidden.data_ptr(), 3, ctypes.byref(p), None)
    dec._set_languages(None)
    assert lib.wt_decoder_set_languages(h, arr(list(range(129))), 129, None, 0) == -22       # WT_E_INVALID
    assert lib.wt_decoder_set_languages(h, arr(lang), len(lang), None, 0) == 0
    assert lib.wt_decoder_set_beam_search(h, ctypes.byref(L.BeamParams(2, 1.0, 0))) == 0
    rc = begin()
    assert rc != 0 and rc != -22 and "beam search" in L.last_error()                          # WT_E_UNSUPPORTED
    assert lib.wt_decoder_set_beam_search(h, None) == 0
    heads = arr([0, 0])
    assert lib.wt_decoder_set_token_timestamps(h, ctypes.byref(L.TokenTimestampParams(1, heads, 7, 0.02))) == 0
    assert begin() == rc and "token-level timestamps" in L.last_error()
    assert lib.wt_decoder_set_token_timestamps(h, None) == 0
    assert lib.wt_decoder_stream_begin(h, 2, 0, ctypes.byref(p), None) == rc and "batch-decode feature" in L.last_error()
    for ids, rows in (([lang[0], lang[0]], None), ([lang[0], cfg["eos_token_id"]], None), ([lang[0], cfg["vocab_size"]], None),
                      (lang, [lang[0], 5, -1]), (lang, [lang[0], -1])):
        assert lib.wt_decoder_set_languages(h, arr(ids), len(ids), arr(rows) if rows else None, len(rows) if rows else 0) == 0
        assert begin() == -22, (ids, rows)
    assert lib.wt_decoder_set_languages(h, None, 0, None, 0) == 0 and begin() == 0
    assert lib.wt_decoder_read_languages(h, None, None, None) != 0


def _audio(seed, seconds):
    """Noise plus modulated tones (the recipe of tests/test_gpu_longform.py)."""
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * 16000)
    t = torch.arange(n) / 16000.0
    x = torch.randn(n, generator=g) * 0.05
    for _ in range(4):
        f, a, m = torch.rand(3, generator=g).tolist()
        x += 0.2 * a * torch.sin(2 * np.pi * (200 + 3000 * f) * t) * (0.5 + 0.5 * torch.sin(2 * np.pi * (0.3 + 2 * m) * t))
    return x.float().cuda()


def test_transcribe_long_detects_on_first_windows(wt):
    """Three short recordings on the toy timestamp model, two rows: every recording's language is detected on its first window and kept; rows on
    their first window and rows further along share decode calls; the result equals the sequential restatement
    (tests/longform_language_ref.py: detect_language on the first window, then every window through the forced-list path at batch 1).
    The random model's greedy decisions are compared across batch sizes, as in tests/test_gpu_longform.py: the logits of a batched row
    differ from batch 1 by summation order alone."""
    z, cfg, enc, dec, hidden = _case("lg-ts-toy_b3")
    fe = wt.audio.LogMelFrontend(n_frames=2 * cfg["max_source_positions"])
    # windows of 1.92 s: the first recording needs at least three, the second is over earlier, so the third starts beside a later window
    audios = [_audio(31, 5.5), _audio(32, 1.0), _audio(33, 3.3)]
    off = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None, no_speech_token_id=None)
    want_segments, want_windows, want_langs = longform_language_ref.transcribe_sequential(wt, enc, dec, fe, audios, startofprev=9, seed=5, **off)
    calls = []
    inner = dec.generate_with_fallback

    def recording(hidden, **kw):
        calls.append(list(kw["language"]))
        return inner(hidden, **kw)

    dec.generate_with_fallback = recording
    try:
        files, trace, langs = wt.runtime.transcribe_long(enc, dec, fe, audios, startofprev_token_id=9, max_rows=2, seed=5, trace=True,
                                                         language="auto", **off)
    finally:
        del dec.generate_with_fallback
    print(f"\nlanguages {langs}, calls {calls}")
    for f in range(3):
        assert [(seek, plen, kind, temp) for file, seek, plen, kind, temp in trace if file == f] == want_windows[f], f
        assert [(s["start"], s["end"], s["ids"], s["temperature"], s["seek"]) for s in files[f]] == want_segments[f], f
        assert langs[f]["language"] == want_langs[f][0] and abs(langs[f]["language_prob"] - want_langs[f][1]) <= 2e-3 * want_langs[f][1]
    assert calls[0] == ["auto", "auto"]                                       # both rows on their first window
    assert any("auto" in c and any(x != "auto" for x in c) for c in calls), calls    # a first window beside a later one: the per-row table
    assert len(calls) >= 3 and all(x == "auto" or x in cfg["language_ids"] for c in calls for x in c)
    # a language per recording, chosen by the caller
    pick = [cfg["language_ids"][0], "auto", cfg["language_ids"][1]]
    _files2, langs2 = wt.runtime.transcribe_long(enc, dec, fe, audios, startofprev_token_id=9, max_rows=3, seed=5, language=pick, **off)
    assert [l["language"] for l in langs2] == [pick[0], want_langs[1][0], pick[2]] and langs2[0]["language_prob"] is None


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--check-goldens":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for _case_name in LG_CASES:
        for _name, _value in zip(("ids", "tok", "probs"), check_golden(_case_name)):
            out[f"{_case_name}.{_name}"] = _value
    np.savez(sys.argv[2], **out)
