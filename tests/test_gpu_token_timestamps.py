"""GPU: token-level timestamps (wt_decoder_set_token_timestamps / wt_decoder_read_token_timestamps): the DTW kernel and the matrix kernels
alone through their hooks against the float64 restatement (tests/token_timestamps_ref.py), the engine against the reference-recorded
goldens (tests/golden/make_golden_token_timestamps.py), the captured queries against the restated decoder, the real size, mode hygiene.

Matrix bar (engine against the reference's fp32 `matrix`): 8 x matrix_f64_dist x max(1, max |matrix|), matrix_f64_dist being the recorded
distance of the reference's own fp32 matrix from the same formula in float64 -- 8 x is the margin the logits bars of this project keep
over their measured distances.  Recorded: tt-toy-short_b3 dist 4.4e-6 -> bar 5.5e-5, tt-tiny_b2 dist 8.3e-6 -> bar 8.8e-5; the goldens'
health criterion perturbs at 10 x these bars.  The hook and real-size tests have no reference run, so their bar is built the same way from
a float32 torch evaluation of the same formula on the same inputs (the reference's arithmetic: fp32 scores, softmax, std_mean, median,
mean) against the float64 one, token_timestamps_ref.matrix_from_queries_fp32.  At real size the engine's timestamps are held to those
of the float64 matrix on the rows whose float64 path passes the goldens' health criterion; measured: medium.en 2 of 8 rows stable, all
tokens equal on 7 rows and 98.5 % on the eighth (an unstable one); tiny.en fp16 decoder 3 of 4 rows stable, all tokens equal on all 4."""
import ctypes

import numpy as np
import pytest
import torch

import token_timestamps_ref as R
from conftest import load_case

pytestmark = pytest.mark.gpu
BAR_MULTIPLE = 8.0


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scratch(lib, n_sel, B, N, S):
    n = int(lib.wt_dbg_token_timestamps_scratch_bytes(n_sel, B, N, S))
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device="cuda")


# ---- the DTW kernel alone --------------------------------------------------------------------------------------------------------------
def _run_dtw(wt, matrix):
    lib = wt._lib.load()
    B, N, S = matrix.shape
    m = torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float32)).cuda()
    ts = torch.full((B, N + 1), -7.0, dtype=torch.float32, device="cuda")
    path = torch.full((B, 2, N + S), -9, dtype=torch.int32, device="cuda")
    plen = torch.zeros(B, dtype=torch.int32, device="cuda")
    scratch = _scratch(lib, 1, B, N, S)
    rc = lib.wt_dbg_token_timestamp_dtw(m.data_ptr(), B, N, S, 0.02, ts.data_ptr(), path.data_ptr(), plen.data_ptr(), scratch.data_ptr(), _stream())
    assert rc == 0, wt._lib.last_error()
    torch.cuda.synchronize()
    return ts.cpu().numpy(), path.cpu().numpy(), plen.cpu().numpy()


def _check_dtw(wt, matrix):
    ts, path, plen = _run_dtw(wt, matrix)
    for b in range(matrix.shape[0]):
        want_ts, text, time = R.token_timestamps(matrix[b], 0.02)
        n = int(plen[b])
        assert n == len(text), (b, n, len(text))
        np.testing.assert_array_equal(path[b, 0, :n][::-1], text)     # the kernel reports the path in backtrace order
        np.testing.assert_array_equal(path[b, 1, :n][::-1], time)
        np.testing.assert_array_equal(ts[b], want_ts)


@pytest.mark.parametrize("case", ["tt-toy-short_b3", "tt-tiny_b2"])
def test_dtw_kernel_on_golden_matrices(wt, case):
    z, _cfg, _w, _mel = load_case(case)
    ts, path, plen = _run_dtw(wt, z["matrix"])
    np.testing.assert_array_equal(ts, z["token_timestamps"])
    for b in range(ts.shape[0]):
        n = int(z["path_len"][b])
        assert plen[b] == n
        np.testing.assert_array_equal(path[b, 0, :n][::-1], z["path_text"][b, :n])
        np.testing.assert_array_equal(path[b, 1, :n][::-1], z["path_time"][b, :n])


@pytest.mark.parametrize("N,S", [(1, 1), (1, 96), (2, 1500), (47, 96), (63, 1500), (447, 1500)])
def test_dtw_kernel_random(wt, N, S):
    rng = np.random.default_rng(1000 * N + S)
    B = 2 if N * S > 100000 else 3
    _check_dtw(wt, rng.standard_normal((B, N, S)).astype(np.float32))


@pytest.mark.parametrize("N,S", [(5, 7), (47, 96), (63, 300)])
def test_dtw_kernel_ties(wt, N, S):
    rng = np.random.default_rng(N + S)
    _check_dtw(wt, np.stack([rng.integers(-2, 3, (N, S)), np.zeros((N, S)), rng.integers(0, 2, (N, S))]).astype(np.float32))


def test_dtw_kernel_nan_and_inf(wt):
    rng = np.random.default_rng(5)
    N, S = 23, 96
    base = rng.standard_normal((6, N, S)).astype(np.float32)
    base[0][:] = np.nan                                             # the matrix of a one-token column normalisation
    base[1][rng.random((N, S)) < 0.1] = np.nan
    base[2][rng.random((N, S)) < 0.1] = np.inf
    base[3][rng.random((N, S)) < 0.1] = -np.inf
    base[4][rng.random((N, S)) < 0.05] = np.inf
    base[4][rng.random((N, S)) < 0.05] = -np.inf
    base[4][rng.random((N, S)) < 0.05] = np.nan
    base[5][:, 40:] = np.nan
    _check_dtw(wt, base)
    _check_dtw(wt, np.full((2, 1, 96), np.nan, np.float32))       # N = 1: std = 0 -> all NaN


# ---- the matrix kernels alone ----------------------------------------------------------------------------------------------------------
def _crafted_qk(n_sel, N, S, rng, half):
    # each token attends around its own frame region with some spread, so that the statistics over the tokens are well away from zero
    k = rng.standard_normal((n_sel, S, 64)).astype(np.float32)
    centre = np.linspace(0, S - 1, N).astype(int)
    q = np.stack([0.35 * k[h][centre] + 0.3 * rng.standard_normal((N, 64)) for h in range(n_sel)]).astype(np.float32)
    if half:
        k = k.astype(np.float16)
    return q, k


@pytest.mark.parametrize("half", [False, True], ids=["f32K", "halfK"])
@pytest.mark.parametrize("n_sel,N,S,width", [(1, 9, 96, 1), (3, 19, 96, 7), (6, 47, 200, 15), (18, 33, 1500, 7), (32, 5, 64, 7), (2, 11, 5, 15),
                                               (2, 11, 7, 15), (2, 11, 8, 15)])
def test_matrix_kernels_against_float64(wt, n_sel, N, S, width, half):
    lib = wt._lib.load()
    rng = np.random.default_rng(n_sel * 1000 + N + S + width)
    q, k = _crafted_qk(n_sel, N, S, rng, half)
    qd, kd = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda()
    w_out = torch.empty(n_sel, N, S, dtype=torch.float32, device="cuda")
    m_out = torch.empty(N, S, dtype=torch.float32, device="cuda")
    scratch = _scratch(lib, n_sel, 1, N, S)
    rc = lib.wt_dbg_token_timestamp_matrix_kernels(qd.data_ptr(), kd.data_ptr(), int(half), n_sel, N, S, width, w_out.data_ptr(), m_out.data_ptr(),
                                                   scratch.data_ptr(), _stream())
    assert rc == 0, wt._lib.last_error()
    torch.cuda.synchronize()
    kf = k.astype(np.float32)
    ref, w64 = R.matrix_from_queries(q, kf, width)
    w_err = np.abs(w_out.cpu().numpy() - w64).max()
    assert w_err <= 8 * 2.0 ** -23, f"softmax rows differ from float64 by {w_err}"
    ref32 = R.matrix_from_queries_fp32(q, kf, width)      # the reference's arithmetic on the same inputs
    dist32 = float(np.abs(ref32.astype(np.float64) - ref).max())
    bar = BAR_MULTIPLE * max(dist32, 2.0 ** -23) * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(m_out.cpu().numpy() - ref).max())
    print(f"matrix kernels n_sel {n_sel} N {N} S {S} width {width} half {half}: err {err:.3e} fp32-formula dist {dist32:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("width", [1, 3, 7, 15])
@pytest.mark.parametrize("S", [5, 7, 8, 96, 1500])
def test_median_kernel_is_exact(wt, width, S):
    lib = wt._lib.load()
    rng = np.random.default_rng(width * 31 + S)
    N = 13
    x = rng.standard_normal((1, N, S)).astype(np.float32)
    x[0, 2, ::5] = x[0, 2, 0]                      # ties
    x[0, 3, S // 2] = np.nan
    x[0, 4, :] = np.round(x[0, 4, :])
    x[0, 5, 0] = np.inf
    x[0, 5, S - 1] = -np.inf
    xd = torch.from_numpy(x).cuda()
    out = torch.empty(N, S, dtype=torch.float32, device="cuda")
    scratch = _scratch(lib, 1, 1, N, S)
    rc = lib.wt_dbg_token_timestamp_median(xd.data_ptr(), 1, N, S, width, out.data_ptr(), scratch.data_ptr(), _stream())
    assert rc == 0, wt._lib.last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), R.median_filter(x, width)[0])


def test_hooks_refuse_bad_arguments(wt):
    lib = wt._lib.load()
    t = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
    s = _scratch(lib, 1, 1, 4, 4)
    assert lib.wt_dbg_token_timestamp_median(t.data_ptr(), 1, 4, 4, 4, t.data_ptr(), s.data_ptr(), _stream()) == -22    # even width
    assert lib.wt_dbg_token_timestamp_median(t.data_ptr(), 1, 4, 4, 17, t.data_ptr(), s.data_ptr(), _stream()) == -22   # width > 15
    assert lib.wt_dbg_token_timestamp_median(t.data_ptr(), 33, 4, 4, 7, t.data_ptr(), s.data_ptr(), _stream()) == -22   # > 32 heads
    assert lib.wt_dbg_token_timestamps_scratch_bytes(1, 1, 2000, 4) == 0


# ---- the engine against the goldens ----------------------------------------------------------------------------------------------------
def _engines(wt, cfg, weights, fp16=False):
    enc = wt.WhisperEncoderEngine(wt.convert.build_encoder_engine(cfg, weights))
    kw = {"precision": "float16"} if fp16 else {}
    dec = wt.WhisperDecoderEngine(wt.convert.build_decoder_engine(cfg, weights, **kw), cfg)
    return enc, dec


def _golden(case):
    z, cfg, weights, mel = load_case(case)
    weights = R.apply_overrides(weights, __import__("json").loads(str(z["weight_overrides_json"])))
    heads = [tuple(int(x) for x in p) for p in z["alignment_heads"]]
    return z, cfg, weights, mel, heads


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("case", ["tt-toy-short_b3", "tt-tiny_b2"])
def test_engine_matches_golden(wt, case, mode):
    """Measured engine distances from the reference's matrix are printed; the bar is the recorded one (module docstring)."""
    z, cfg, weights, mel, heads = _golden(case)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    dec.set_profiling(mode == "eager")
    ids, ts = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads, median_filter_width=int(z["median_filter_width"]))
    dec.set_profiling(False)
    ids, ts = ids.cpu().numpy(), ts.cpu().numpy()
    np.testing.assert_array_equal(ids, z["ids"])
    N = ids.shape[1] - 1
    matrix = dec.token_timestamp_matrix().cpu().numpy()[:, :N]
    ref = z["matrix"]
    bar = BAR_MULTIPLE * float(z["matrix_f64_dist"]) * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(matrix - ref).max())
    print(f"{case} [{mode}]: engine matrix differs from the reference's by {err:.3e}, bar {bar:.3e} (reference fp32 noise {float(z['matrix_f64_dist']):.3e})")
    assert float(z["matrix_bar"]) == pytest.approx(bar)
    assert err <= bar
    np.testing.assert_array_equal(ts, z["token_timestamps"])
    for b in range(ids.shape[0]):      # and the DTW kernel on the engine's own matrix equals the restated DTW on it
        np.testing.assert_array_equal(ts[b], R.token_timestamps(matrix[b], 0.02)[0])


@pytest.mark.parametrize("case", ["tt-toy-short_b3", "tt-tiny_b2"])
def test_q_hist_matches_restated_queries(wt, case):
    """The captured queries against the float64 decoder restated over the recorded ids (pad inputs of finished rows included) and the
    engine's own encoder output: a capture at the wrong step or row, after the finished-row exit, or of the wrong residual buffer
    moves whole rows by O(1); fp32 rounding through the layers stays below 1e-4 x max |q|."""
    z, cfg, weights, mel, heads = _golden(case)
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ids, _ts = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads)
    np.testing.assert_array_equal(ids.cpu().numpy(), z["ids"])
    N = ids.shape[1] - 1
    qh = dec.token_timestamp_q_hist().cpu().numpy()[:, :, :N]
    q64, k64 = R.decoder_queries_f64(weights, cfg, z["ids"], hidden.cpu().numpy(), heads)
    err = float(np.abs(qh - q64).max())
    scale = float(np.abs(q64).max())
    print(f"{case}: q_hist differs from the float64 queries by {err:.3e} (max |q| {scale:.3f})")
    assert err <= 1e-4 * max(1.0, scale)
    for i, (l, h) in enumerate(heads):
        kerr = float(np.abs(dec.cross_k_head(l, h) - k64[i]).max())
        assert kerr <= 1e-4 * max(1.0, float(np.abs(k64[i]).max())), (l, h, kerr)


# ---- real size: the engine against the restatement on its own q_hist and K cache -------------------------------------------------------
def _real_size(wt, cname, B, steps, heads, fp16):
    cfg = wt.synthetic.get_config(cname)
    weights = wt.synthetic.make_weights(cfg, 77)
    mel = wt.synthetic.make_mel(cfg, index=300, batch=B)
    enc, dec = _engines(wt, cfg, weights, fp16=fp16)
    hidden = enc(torch.from_numpy(mel).cuda())
    ids, ts = dec.generate(hidden, max_length=steps + 1, return_token_timestamps=True, alignment_heads=heads)
    N = ids.shape[1] - 1
    assert N == steps        # random weights never emit EOS
    ts = ts.cpu().numpy()
    matrix = dec.token_timestamp_matrix().cpu().numpy()[:, :N]
    qh = dec.token_timestamp_q_hist().cpu().numpy()[:, :, :N]
    K = np.stack([dec.cross_k_head(l, h) for l, h in heads])             # [heads][B][S][64]
    worst, n_stable = 0.0, 0
    for b in range(B):
        ref, w64 = R.matrix_from_queries(qh[:, b], K[:, b], 7)
        ref32 = R.matrix_from_queries_fp32(qh[:, b], K[:, b], 7)
        dist32 = float(np.abs(ref32.astype(np.float64) - ref).max())
        bar = BAR_MULTIPLE * max(dist32, 2.0 ** -23) * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(matrix[b] - ref).max())
        worst = max(worst, err / bar)
        print(f"{cname} fp16={fp16} row {b}: matrix err {err:.3e} fp32-formula dist {dist32:.3e} bar {bar:.3e}")
        assert err <= bar
        np.testing.assert_array_equal(ts[b], R.token_timestamps(matrix[b], 0.02)[0])
        assert ts[b, 0] == 0 and (np.diff(ts[b, 1:]) >= 0).all() and ts[b].max() <= 0.02 * cfg["max_source_positions"]
        # the timestamps of the float64 matrix: where that row's path is stable under the goldens' health criterion (32 perturbations of
        # the float64 matrix at 10 x the bar leave its timestamps unchanged) the engine's must equal them exactly; a row whose path
        # through flat cost turns under such noise has no timestamps to be held to
        want = R.token_timestamps(ref, 0.02)[0]
        rng = np.random.default_rng(b)
        stable = all(np.array_equal(R.token_timestamps(ref + rng.uniform(-10 * bar, 10 * bar, ref.shape), 0.02)[0], want) for _ in range(32))
        same = float((ts[b] == want).mean())
        print(f"{cname} fp16={fp16} row {b}: float64-matrix timestamps stable {stable}, engine tokens equal {same:.3f}")
        if stable:
            n_stable += 1
            np.testing.assert_array_equal(ts[b], want)
    assert n_stable >= 1, "no row with a stable float64 path: the timestamp check would be empty"
    return worst


def test_real_size_medium_en_fp32(wt):
    heads = [(l, h) for l in (10, 13, 16, 19, 21, 23) for h in (1, 7, 12)]          # 18 heads, as medium.en's alignment list is long
    _real_size(wt, "whisper-medium.en", 8, 64, heads, fp16=False)


def test_real_size_tiny_en_fp16_decoder(wt):
    _real_size(wt, "whisper-tiny.en", 4, 48, [(2, 1), (3, 0), (3, 3), (3, 5), (1, 2), (2, 4)], fp16=True)


# ---- mode hygiene on one handle --------------------------------------------------------------------------------------------------------
def test_mode_hygiene_on_one_handle(wt):
    z, cfg, weights, mel, heads = _golden("tt-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    _enc2, never = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    plain = never.generate(hidden).cpu().numpy()
    off0 = dec.generate(hidden).cpu().numpy()
    ids_on, ts_on = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads)
    off1 = dec.generate(hidden).cpu().numpy()
    np.testing.assert_array_equal(off0, plain)
    np.testing.assert_array_equal(off1, plain)
    np.testing.assert_array_equal(ids_on.cpu().numpy(), z["ids"])
    np.testing.assert_array_equal(ts_on.cpu().numpy(), z["token_timestamps"])
    lib, h = dec.session._lib, dec.session.handle
    buf = torch.empty(3, cfg["max_length"], dtype=torch.float32, device="cuda")
    assert lib.wt_decoder_read_token_timestamps(h, buf.data_ptr(), cfg["max_length"], _stream()) == -1       # mode off: WT_E_STATE
    # a changed head list takes effect: one head alone gives that head's own matrix
    ids1, ts1 = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads[:1])
    N = ids1.shape[1] - 1
    m1 = dec.token_timestamp_matrix().cpu().numpy()[:, :N]
    qh = dec.token_timestamp_q_hist().cpu().numpy()[:, :, :N]
    assert qh.shape[0] == 1
    k = dec.cross_k_head(*heads[0])
    for b in range(3):
        ref, _w = R.matrix_from_queries(qh[:, b], k[None, b], 7)
        assert np.abs(m1[b] - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())
        np.testing.assert_array_equal(ts1.cpu().numpy()[b], R.token_timestamps(m1[b], 0.02)[0])
    assert np.abs(m1 - z["matrix"]).max() > 1e-2
    # and back to the full list
    _ids, ts2 = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads)
    np.testing.assert_array_equal(ts2.cpu().numpy(), z["token_timestamps"])


def test_with_timestamp_mode_and_forced_eos(wt):
    z, cfg, weights, mel = load_case("ts-toy_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    heads = [(1, 0), (0, 1)]
    ids, ts = dec.generate(hidden, return_timestamps=True, return_token_timestamps=True, alignment_heads=heads)
    np.testing.assert_array_equal(ids.cpu().numpy(), z["ids"])          # the <|t|> grammar is untouched by the capture
    N = ids.shape[1] - 1
    m = dec.token_timestamp_matrix().cpu().numpy()[:, :N]
    for b in range(3):
        np.testing.assert_array_equal(ts.cpu().numpy()[b], R.token_timestamps(m[b], 0.02)[0])
    ids, ts = dec.generate(hidden, force_eos_steps=[3, 9, 5], return_token_timestamps=True, alignment_heads=heads)
    assert ids.shape[1] == 11 and ts.shape == (3, 11)
    m = dec.token_timestamp_matrix().cpu().numpy()[:, :10]
    for b in range(3):
        np.testing.assert_array_equal(ts.cpu().numpy()[b], R.token_timestamps(m[b], 0.02)[0])


def test_refused_with_beams_and_in_a_stream(wt):
    z, cfg, weights, mel, heads = _golden("tt-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    with pytest.raises(ValueError):
        dec.generate(hidden, num_beams=2, return_token_timestamps=True, alignment_heads=heads)
    with pytest.raises(ValueError):
        dec.stream(slots=4, return_token_timestamps=True)
    lib, h = dec.session._lib, dec.session.handle
    arr = (ctypes.c_int32 * 2)(1, 0)
    t = wt._lib.TokenTimestampParams(1, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), 7, 0.02)
    assert lib.wt_decoder_set_token_timestamps(h, ctypes.byref(t)) == 0
    p = dec._params(None, None, None)
    assert lib.wt_decoder_stream_begin(h, 4, 0, ctypes.byref(p), _stream()) == -38                      # WT_E_UNSUPPORTED
    b = wt._lib.BeamParams(2, 1.0, 0)
    assert lib.wt_decoder_set_beam_search(h, ctypes.byref(b)) == 0
    assert lib.wt_decoder_begin(h, hidden.data_ptr(), 3, ctypes.byref(p), _stream()) == -38
    assert lib.wt_decoder_set_beam_search(h, None) == 0
    for bad_heads, width in (((2, 0), 7), ((0, 2), 7), ((0, 0), 4), ((0, 0), 17)):
        arr = (ctypes.c_int32 * 2)(*bad_heads)
        t = wt._lib.TokenTimestampParams(1, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), width, 0.02)
        assert lib.wt_decoder_set_token_timestamps(h, ctypes.byref(t)) == -22
    arr = (ctypes.c_int32 * 66)(*([0, 0] * 33))
    t = wt._lib.TokenTimestampParams(33, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), 7, 0.02)
    assert lib.wt_decoder_set_token_timestamps(h, ctypes.byref(t)) == -22
    assert lib.wt_decoder_set_token_timestamps(h, None) == 0
    dec.stream(slots=4)       # the Python stream turns the mode off first


def test_smaller_batch_and_shorter_length_on_one_handle(wt):
    """The same heads on one handle with a smaller batch, then a shorter max_length, then more than 16 utterances (16 + 4): the head
    table and the query history keep their places or are uploaded again -- ids, timestamps and captured queries equal those of a
    handle that only ever ran that decode."""
    z, cfg, weights, mel, heads = _golden("tt-toy-short_b3")
    enc, dec = _engines(wt, cfg, weights)
    hidden = enc(torch.from_numpy(mel).cuda())
    ids3, ts3 = dec.generate(hidden, return_token_timestamps=True, alignment_heads=heads)
    np.testing.assert_array_equal(ts3.cpu().numpy(), z["token_timestamps"])

    def fresh(h, **kw):
        _e, d = _engines(wt, cfg, weights)
        i, t = d.generate(h, return_token_timestamps=True, alignment_heads=heads, **kw)
        return i.cpu().numpy(), t.cpu().numpy(), d.token_timestamp_q_hist().cpu().numpy()

    for h, kw in ((hidden[:2], {}), (hidden[:2], {"max_length": 9}), (hidden, {"max_length": 12}), (hidden[1:2], {})):
        i, t = dec.generate(h, return_token_timestamps=True, alignment_heads=heads, **kw)
        q = dec.token_timestamp_q_hist().cpu().numpy()
        wi, wt_, wq = fresh(h, **kw)
        np.testing.assert_array_equal(i.cpu().numpy(), wi)
        np.testing.assert_array_equal(q, wq)
        np.testing.assert_array_equal(t.cpu().numpy(), wt_)
    many = torch.cat([hidden] * 7)[:20]                                   # 16 utterances, then 4, on the same handle
    i20, t20 = dec.generate(many, return_token_timestamps=True, alignment_heads=heads)
    assert i20.shape[0] == 20 and t20.shape == i20.shape
    i16, t16, _q = fresh(many[:16])
    i4, t4, _q = fresh(many[16:])
    np.testing.assert_array_equal(i20.cpu().numpy()[:16, :i16.shape[1]], i16)
    np.testing.assert_array_equal(t20.cpu().numpy()[:16, :t16.shape[1]], t16)
    np.testing.assert_array_equal(i20.cpu().numpy()[16:, :i4.shape[1]], i4)
    np.testing.assert_array_equal(t20.cpu().numpy()[16:, :t4.shape[1]], t4)


def test_run_py_return_token_timestamps(wt, tmp_path):
    import json
    import os
    import pickle
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z, cfg, weights, mel, heads = _golden("tt-toy-short_b3")
    eng = tmp_path / "eng"
    eng.mkdir()
    (eng / "WhisperEncoder.engine").write_bytes(wt.convert.build_encoder_engine(cfg, weights))
    (eng / "WhisperDecoder.engine").write_bytes(wt.convert.build_decoder_engine(cfg, weights))
    (eng / "config.pkl").write_bytes(pickle.dumps(cfg))
    cmd = [sys.executable, os.path.join(root, "examples", "whisper", "run.py"), "--engine_dir", str(eng), "--synthetic", "3", "--synthetic_start",
           str(int(z["mel_index"])), "--batching", "dataset", "--workers", "1", "--return_token_timestamps", "--dump_ids", str(tmp_path / "ids.json")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)        # synthetic model, no heads given: refused as transformers does
    assert out.returncode != 0 and "alignment_heads" in out.stderr
    out = subprocess.run(cmd + ["--alignment_heads"] + [f"{l},{h}" for l, h in heads], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.load(open(tmp_path / "ids.json")) == z["ids"].tolist()
    lines = [l for l in out.stdout.splitlines() if l.startswith("utterance ") and "token times:" in l]
    assert len(lines) == 3, out.stdout[-1500:]
    for b, line in enumerate(lines):       # "id[start-->end]" per token: the golden's times, a token ending where the next one starts
        ts = z["token_timestamps"][b]
        first = line.split("token times:")[1].split()[:4]
        want = [f"{int(z['ids'][b, k])}[{ts[k]:.2f}-->{ts[k + 1]:.2f}]" for k in range(4)]
        assert first == want, (first, want)
