"""The log-mel front-end's kernels (csrc/frontend.hip: dft_power_f64_kernel, the mel GEMM launch, log_max_kernel,
normalize_transpose_kernel) per element and per stage against tests/frontend_ref.py, through wt_logmel_create / wt_logmel_forward and
the wt_dbg_logmel_stages hook: the power spectrum BEFORE the log and the clamp hide it, at the geometries that reach every path of the
DFT kernel, under a window that tells a reversed frame, on inputs that sit on the padding edges; per-utterance floors, handle reuse,
non-finite input and the geometries wt_logmel_create refuses.  tests/test_frontend_ref.py holds the CPU half (the reference itself,
the float32 budget of every input used here, and which kernel path each geometry reaches)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frontend_ref as fr
from conftest import GOLDEN_DIR
from test_frontend import CASES, synthetic_waveform

pytestmark = pytest.mark.gpu

IDS = ["-".join(map(str, g)) for g in fr.GEOMETRIES]


class LogMel:
    """Test-local handle on wt_logmel_* for any geometry, window and filter bank (audio.LogMelFrontend is fixed to Whisper's)."""

    def __init__(self, geom, window, filters):
        from whisper_trtllm_amd import _lib
        if not torch.cuda.is_available():
            pytest.fail("GPU test selected but no GPU is visible")
        self.lib, self._check = _lib.load(), _lib.check
        self.n_fft, self.hop, self.n_mels, self.T, self.npw = geom
        win = np.ascontiguousarray(window, dtype=np.float64)
        filt = np.ascontiguousarray(fr.pad_filters(filters, self.npw))
        self.handle = ctypes.c_void_p()
        self._check(self.lib.wt_logmel_create(torch.cuda.current_device(), self.n_fft, self.hop, self.n_mels, self.T, win.ctypes.data,
                                              filt.ctypes.data, self.npw, ctypes.byref(self.handle)), "wt_logmel_create")

    def __call__(self, waves, stages=True):
        """f32 [B, n_in] (numpy) -> features [B, n_mels, T], and with `stages` pw [B, T, npw] and logmel [B, T, n_mels]; numpy."""
        w = torch.from_numpy(np.ascontiguousarray(waves, dtype=np.float32)).cuda()
        B = w.shape[0]
        out = torch.full((B, self.n_mels, self.T), 777.0, dtype=torch.float32, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._check(self.lib.wt_logmel_forward(self.handle, w.data_ptr(), B, w.shape[1], out.data_ptr(), stream), "wt_logmel_forward")
        if not stages:
            return out.cpu().numpy()
        pw = torch.full((B, self.T, self.npw), 777.0, dtype=torch.float32, device="cuda")
        lm = torch.full((B, self.T, self.n_mels), 777.0, dtype=torch.float32, device="cuda")
        self._check(self.lib.wt_dbg_logmel_stages(self.handle, B, pw.data_ptr(), lm.data_ptr(), stream), "wt_dbg_logmel_stages")
        return out.cpu().numpy(), pw.cpu().numpy(), lm.cpu().numpy()

    def close(self):
        if self.handle.value:
            self.lib.wt_logmel_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_stages(got, ref, n_bins, tag):
    """One utterance: (features [n_mels, T], pw [T, npw], logmel [T, n_mels]) of the GPU against frontend_ref.Stages."""
    feats, pw, logmel = got
    assert np.isfinite(pw).all() and (pw >= 0).all(), tag
    assert not pw[:, n_bins:].any(), tag                                   # the padded power columns are exactly 0
    err = np.abs(np.sqrt(pw[:, :n_bins].astype(np.float64)) - ref.amp)
    bound = fr.amp_bound(ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (tag, "frame, bin", worst, "error", err[worst], "bound", bound[worst], "amp", ref.amp[worst])
    assert np.abs(logmel - ref.logmel).max() < fr.FEATURE_ATOL, (tag, np.abs(logmel - ref.logmel).max())
    assert np.abs(feats - ref.features).max() < fr.FEATURE_ATOL, (tag, np.abs(feats - ref.features).max())


def filter_sets(geom):
    sets = [("mel", fr.mel_filters(geom))]
    if geom[2] == 128:
        sets.append(("random", fr.random_filters(geom)))   # dense: all 128 mel rows and every power column count
    return sets


@pytest.mark.parametrize("window_kind", ["hann", "asym"])
@pytest.mark.parametrize("geom", fr.GEOMETRIES, ids=IDS)
def test_every_stage_per_element_at_the_geometries_that_reach_every_path(geom, window_kind):
    """Power spectrum on amplitudes: |sqrt(pw) - amp_ref| <= 2^-22 amp_ref + 2 n_fft 2^-53 sum_k |x_k w_k| (frontend_ref.amp_bound:
    float32 roundings of the spectrum and the power, fp64 dot-product bound of both DFTs; derived, not measured -- an fp32 DFT misses
    it by orders of magnitude on the tones), padded columns exactly 0; log-mel before the clamp and features within the front-end's
    2e-5.  Every shared input (noise, tones, DC, edge impulses, every n_in around the padding edges), rows of a batch of 3 checked
    each against its own reference.  The "asym" window is what would tell a frame read backwards (test_frontend_ref.py)."""
    n_fft, hop, n_mels, T, npw = geom
    n_bins = fr.derived(geom)["n_bins"]
    window = fr.hann(n_fft) if window_kind == "hann" else fr.asymmetric_window(n_fft)
    for fname, filters in filter_sets(geom):
        with LogMel(geom, window, filters) as fe:
            for name, batch in fr.input_batches(geom):
                feats, pw, logmel = fe(batch)
                for r in range(3):
                    ref = fr.stages(batch[r], n_fft, hop, T, window, filters)
                    check_stages((feats[r], pw[r], logmel[r]), ref, n_bins, (fname, name, "row", r))


@pytest.fixture(scope="module")
def whisper_refs():
    """The Whisper-geometry rows and their references (rfft: the matrix DFT is pinned to it in test_frontend_ref.py), computed once.
    key (name, n_mels) -> Stages; rows by name."""
    (loud, quiet, clip), _ = fr.whisper_floor_batch()
    rows = {"loud": loud, "quiet": quiet, "clip": clip, "plain": fr.whisper_plain_row()}
    refs = {}

    def ref(name, geom):
        if (name, geom[2]) not in refs:
            refs[(name, geom[2])] = fr.stages(rows[name], geom[0], geom[1], geom[3], fr.hann(geom[0]), fr.mel_filters(geom), use_rfft=True)
        return refs[(name, geom[2])]
    return rows, ref


def padded(rows, n=480000):
    out = np.zeros((len(rows), n), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


@pytest.mark.parametrize("geom", [fr.WHISPER, fr.WHISPER_V3], ids=["80mels", "128mels"])
def test_each_utterance_of_a_batch_has_its_own_floor(whisper_refs, geom):
    """A loud full-length row (floor max - 8, half of it on the floor), a row at 1e-3 (floor: the 1e-10 clamp, -1.5) and a short clip in
    ONE batch: each matches its own single-utterance reference at every stage and is bit-identical to the same row run alone (a
    batch-global maximum, or bmax indexed without the utterance, fails both).  Frames wholly inside the zero padding are bit-identical
    columns equal to (max(-10, max - 8) + 4) / 4, which is what audio.valid_frames counts."""
    from whisper_trtllm_amd import audio
    rows, ref = whisper_refs
    names = ["loud", "quiet", "clip"]
    n_bins, T = 201, geom[3]
    with LogMel(geom, fr.hann(geom[0]), fr.mel_filters(geom)) as fe:
        feats, pw, logmel = fe(padded([rows[n] for n in names]))
        for i, n in enumerate(names):
            check_stages((feats[i], pw[i], logmel[i]), ref(n, geom), n_bins, n)
        for i, n in enumerate(names):
            alone = fe(rows[n][None], stages=False)       # its own n_in: the zero padding is the kernel's
            assert same_bits(alone[0], feats[i]), n
        plain = fe(rows["plain"][None], stages=False)[0]
    assert np.abs(plain - ref("plain", geom).features).max() < fr.FEATURE_ATOL
    assert abs(float(feats[0].min()) - (float(ref("loud", geom).logmel.max()) - 8.0 + 4.0) / 4.0) < fr.FEATURE_ATOL
    assert 0.2 < (feats[0] == feats[0].min()).mean() < 0.95 and feats[2].min() > -1.4
    # 0.4 s, 5 s and 30 s: ceil((n_in + n_fft / 2) / hop) frames touch a sample, the rest are the floor bit for bit.  Silence is
    # log10f(1e-10f), -10 to the 2 float32 ulps the device's log10f is specified to (the reference's float64 log10 gives -10 exactly),
    # so the floor is checked exactly in float32 from the kernel's own silence and to those 2 ulps / 4 against -10.
    ulp10 = float(np.spacing(np.float32(10.0)))
    expected = {"clip": 42, "quiet": 502}
    for i, n in ((2, "clip"), (1, "quiet")):
        v = expected[n]
        assert v == -(-(len(rows[n]) + 200) // 160)
        pad = feats[i][:, v:]
        silence = logmel[i][v:]
        assert same_bits(silence, np.full_like(silence, silence[0, 0])) and abs(float(silence[0, 0]) + 10.0) <= 2 * ulp10, n
        floor = (np.maximum(silence[0, 0], logmel[i].max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)   # float32, as the kernel
        assert same_bits(pad, np.full_like(pad, floor)), n
        tol = 2 * ulp10 / 4 if n == "quiet" else fr.FEATURE_ATOL     # quiet: the -10 clamp itself; clip: max - 8 of a computed maximum
        assert abs(float(floor) - (max(-10.0, float(ref(n, geom).logmel.max()) - 8.0) + 4.0) / 4.0) <= tol, n
        assert not (feats[i][:, v - 1] == floor).all(), n
    assert abs(float(feats[1].min()) + 1.5) <= 2 * ulp10 / 4
    stack = torch.from_numpy(np.stack([plain, feats[1], feats[2]]))
    assert audio.valid_frames(stack) == [3000, 502, 42]
    ref_stack = torch.from_numpy(np.stack([ref(n, geom).features for n in ("plain", "quiet", "clip")]))
    assert audio.valid_frames(ref_stack) == [3000, 502, 42]
    assert audio.valid_frames(stack.cuda()) == [3000, 502, 42]


def test_handle_reuse_across_batch_sizes_is_bit_identical_to_a_fresh_handle(whisper_refs):
    """One handle runs batch 1, then 3 (the workspace regrows and moves), then 2 (smaller than the workspace: pw / mel / bmax keep the
    strides of 3), then 1; every result, stages included, equals a fresh handle's bit for bit."""
    rows, _ = whisper_refs
    geom = fr.WHISPER
    waves = padded([rows["plain"], rows["loud"], rows["quiet"]], 30 * 16000 + 7)      # n_in past 30 s: trimmed
    window, filters = fr.hann(400), fr.mel_filters(geom)
    with LogMel(geom, window, filters) as reused:
        assert reused.lib.wt_dbg_logmel_stages(reused.handle, 1, None, None, None) == -22     # nothing run yet: no workspace
        for B in (1, 3, 2, 1):
            got = reused(waves[:B])
            assert reused.lib.wt_dbg_logmel_stages(reused.handle, B, None, None, None) == 0   # both pointers may be NULL
            assert reused.lib.wt_dbg_logmel_stages(reused.handle, 4, None, None, None) == -22  # beyond the workspace
            with LogMel(geom, window, filters) as fresh:
                want = fresh(waves[:B])
            for g, w, what in zip(got, want, ("features", "pw", "logmel")):
                assert same_bits(g, w), (B, what)
            assert not (got[0] == 777.0).any() and not (got[1] == 777.0).any() and not (got[2] == 777.0).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("geom", [fr.WHISPER, fr.WHISPER_V3], ids=["80mels", "128mels"])
def test_nonfinite_sample_makes_its_utterance_nan_and_leaves_the_others_alone(whisper_refs, geom, bad):
    """Row 1 of a batch of 3 carries ONE NaN (or +Inf) sample: like the reference (np.maximum and ndarray.max propagate NaN; asserted
    for frontend_ref and the oracle in test_frontend_ref.py) all n_mels x T features of row 1 are NaN -- fmaxf would turn the frames
    the sample touches into -10, i.e. silence, and leave the rest finite -- and rows 0 and 2 are bit-identical to the clean batch."""
    rows, _ = whisper_refs
    clean = padded([rows["plain"], rows["clip"], rows["quiet"]])
    dirty = clean.copy()
    dirty[1, 3210] = bad
    with LogMel(geom, fr.hann(400), fr.mel_filters(geom)) as fe:
        base = fe(clean, stages=False)
        got, pw, logmel = fe(dirty)
    assert np.isfinite(base).all()
    assert np.isnan(got[1]).all(), f"{np.isnan(got[1]).sum()} of {got[1].size} NaN, finite minimum {np.nanmin(got[1])}"
    assert same_bits(got[0], base[0]) and same_bits(got[2], base[2])
    touched = np.isnan(logmel[1]).all(axis=1)                  # the frames that hold the sample: t * 160 - 200 <= 3210 < t * 160 + 200
    assert np.flatnonzero(touched).tolist() == list(range(19, 22)) and np.isfinite(logmel[1][~touched]).all()
    assert np.isfinite(pw[0]).all() and np.isfinite(pw[2]).all()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN_DIR, "frontend.npz")))


@pytest.mark.parametrize("case", CASES)
def test_finite_golden_waveforms_keep_their_recorded_features(gold, case):
    """The NaN-propagating clamp and reductions change nothing for finite input: the four golden waveforms at the recorded reference
    features' existing tolerance, every stage against the reference."""
    wav = synthetic_waveform(int(gold[f"{case}_seed"]), float(gold[f"{case}_seconds"]))
    geom = fr.WHISPER
    with LogMel(geom, fr.hann(400), fr.mel_filters(geom)) as fe:
        feats, pw, logmel = fe(wav[None])
    check_stages((feats[0], pw[0], logmel[0]), fr.stages(wav, 400, 160, 3000, fr.hann(400), fr.mel_filters(geom), use_rfft=True), 201, case)
    np.testing.assert_allclose(feats[0][::5, ::37], gold[f"{case}_sub"], atol=2e-5)
    np.testing.assert_allclose(feats[0][:, :4], gold[f"{case}_frames_head"], atol=2e-5)
    np.testing.assert_allclose(feats[0][:, -4:], gold[f"{case}_frames_tail"], atol=2e-5)


REFUSED = {   # why -> (n_fft, hop, n_mels, T, npw)
    "n_fft-not-multiple-of-4": (18, 5, 8, 70, 12),
    "n_fft-448-nbt-15": (448, 112, 80, 65, 228),             # 225 bins: 15 bin tiles > 2 * DFT_MAX_BT
    "npw-below-n_bins": (64, 16, 20, 200, 32),               # n_bins 33
    "npw-not-multiple-of-4": (64, 16, 20, 200, 38),
    "npw-above-16-nbt": (64, 16, 20, 200, 52),               # 16 * nbt = 48
    "n_mels-129": (64, 16, 129, 200, 36),                    # the transpose tile has 128 columns
    "lds-above-160KiB": (16, 650, 8, 70, 12),                # 16 * 8 + (63 * 650 + 16) * 4 = 163992 bytes
}


@pytest.mark.parametrize("why", list(REFUSED))
def test_create_refuses_what_the_kernels_cannot_run(why):
    geom = REFUSED[why]
    from whisper_trtllm_amd import _lib
    lib = _lib.load()
    n_fft, hop, n_mels, T, npw = geom
    window = np.ones(n_fft, dtype=np.float64)
    filt = np.zeros((n_mels, max(npw, 4)), dtype=np.float32)
    handle = ctypes.c_void_p(0xdead)
    rc = lib.wt_logmel_create(torch.cuda.current_device(), n_fft, hop, n_mels, T, window.ctypes.data, filt.ctypes.data, npw, ctypes.byref(handle))
    assert rc == -22 and not handle.value, why
    assert "bad geometry" in _lib.last_error()
    if hop == 650:   # one step inside the limit is accepted (163740 bytes; not launched here)
        ok = ctypes.c_void_p()
        filt = np.zeros((n_mels, npw), dtype=np.float32)
        assert lib.wt_logmel_create(torch.cuda.current_device(), n_fft, 649, n_mels, T, window.ctypes.data, filt.ctypes.data, npw, ctypes.byref(ok)) == 0
        lib.wt_logmel_destroy(ok)
