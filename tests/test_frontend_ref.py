"""tests/frontend_ref.py, the per-stage fp64 reference the GPU front-end tests (test_gpu_frontend_kernels.py) compare against: pinned
to the oracle and the recorded reference features at Whisper's geometry, its matrix DFT against rfft, and the properties of the shared
inputs and geometries that those GPU tests rely on.  No GPU."""
import os

import numpy as np
import pytest

import cpu_ref
import frontend_ref as fr
from conftest import GOLDEN_DIR
from test_frontend import CASES, synthetic_waveform

ALL_GEOMETRIES = fr.GEOMETRIES
IDS = ["-".join(map(str, g)) for g in ALL_GEOMETRIES]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN_DIR, "frontend.npz")))


@pytest.mark.parametrize("case", CASES)
def test_reference_equals_oracle_and_goldens_at_whisper_geometry(gold, case):
    wav = synthetic_waveform(int(gold[f"{case}_seed"]), float(gold[f"{case}_seconds"]))
    n_fft, hop, _, T, _ = fr.WHISPER
    filters = cpu_ref.whisper_mel_filters().T
    oracle = cpu_ref.log_mel_spectrogram(wav)
    for use_rfft in (True, False):
        st = fr.stages(wav, n_fft, hop, T, fr.hann(n_fft), filters, use_rfft=use_rfft)
        assert st.features.shape == (80, 3000) and st.features.dtype == np.float32 and st.logmel.shape == (3000, 80)
        assert np.abs(st.features - oracle).max() <= 1e-6
        np.testing.assert_allclose(st.features[::5, ::37], gold[f"{case}_sub"], atol=1e-5)
        np.testing.assert_allclose(st.features[:, :4], gold[f"{case}_frames_head"], atol=1e-5)
        np.testing.assert_allclose(st.features[:, -4:], gold[f"{case}_frames_tail"], atol=1e-5)


def test_product_filter_bank_equals_oracle_bank_at_both_widths():
    for geom in (fr.WHISPER, fr.WHISPER_V3):
        np.testing.assert_allclose(fr.mel_filters(geom), cpu_ref.whisper_mel_filters(201, geom[2]).T, atol=1e-15)


def test_geometries_reach_the_paths_they_are_listed_for():
    """The kernel-path quantities of every geometry, derived as csrc/frontend.hip derives them (comments at frontend_ref.GEOMETRIES)."""
    d = [fr.derived(g) for g in fr.GEOMETRIES]
    assert [x["nbt"] for x in d] == [1, 1, 2, 3, 3, 1, 14]
    assert [(x["nb_low"], x["nb_high"]) for x in d] == [(1, 0), (1, 0), (1, 1), (2, 1), (2, 1), (1, 0), (7, 7)]   # nb = 0, unequal, full
    assert [x["ksteps"] for x in d] == [4, 7, 9, 16, 16, 4, 111] and sum(x["ksteps"] % 2 for x in d) == 3          # odd: prefetch tails
    assert [x["tail"] for x in d] == [6, 0, 2, 8, 8, 6, 1] and all(x["blocks"] >= 2 for x in d if x["tail"])
    assert [x["dma_gemm"] for x in d] == [False, True, False, False, True, False, True]
    assert not fr.derived(fr.WHISPER)["dma_gemm"] and fr.derived(fr.WHISPER)["ksteps"] % 2 == 0 and fr.derived(fr.WHISPER)["tail"] == 56
    for (n_fft, hop, n_mels, T, npw), x in zip(fr.GEOMETRIES, d):
        assert n_fft // 2 < T * hop and x["n_bins"] <= npw <= 16 * x["nbt"] and npw % 4 == 0 and n_mels <= 128
    assert max(g[2] for g in fr.GEOMETRIES) == 128 and any(g[1] > g[0] for g in fr.GEOMETRIES)


@pytest.mark.parametrize("geom", ALL_GEOMETRIES, ids=IDS)
def test_asymmetric_window_sees_a_reversed_frame_and_hann_does_not(geom):
    """Why every geometry also runs with an asymmetric window: with samples and window indexed against each other (x[n_fft - k] w[k])
    the power spectrum under the periodic Hann window is unchanged, under the asymmetric window it moves by far more than the bound."""
    n_fft = geom[0]
    x = np.random.default_rng(5).uniform(-1.0, 1.0, n_fft)
    xr = x[(n_fft - np.arange(n_fft)) % n_fft]
    c, s = fr.dft_matrices(n_fft)

    def amp(frame, w):
        return np.hypot(c @ (frame * w), s @ (frame * w))

    slack = 2.0 ** -22 * amp(x, fr.hann(n_fft)) + 2.0 * n_fft * 2.0 ** -53 * np.abs(x * fr.hann(n_fft)).sum()
    assert (np.abs(amp(x, fr.hann(n_fft)) - amp(xr, fr.hann(n_fft))) <= slack).all()
    w = fr.asymmetric_window(n_fft)
    assert np.abs(amp(x, w) - amp(xr, w)).max() > 1e-2 * amp(x, w).max()


def _filter_sets(geom):
    sets = [("mel", fr.mel_filters(geom))]
    if geom[2] == 128:
        sets.append(("random", fr.random_filters(geom)))
    return sets


@pytest.mark.parametrize("geom", ALL_GEOMETRIES, ids=IDS)
def test_inputs_matrix_dft_agrees_with_rfft_and_float32_tail_stays_inside_the_bar(geom):
    """On every shared input, window and filter set: (a) the DFT by definition and rfft agree within the power bound the GPU is held to;
    (b) the log-mel of the two differs by under a quarter of the feature bar, i.e. no element hangs on fp64 rounding noise of the DFT;
    (c) a numpy float32 emulation of the stages after the DFT stays within a quarter of the bar of the fp64 reference, so the bar
    leaves three quarters to the kernels' own summation order.  An input that fails this is replaced, never the bar."""
    n_fft, hop, n_mels, T, npw = geom
    for wname, window in (("hann", fr.hann(n_fft)), ("asym", fr.asymmetric_window(n_fft))):
        for fname, filters in _filter_sets(geom):
            f32 = fr.pad_filters(filters, npw)
            for name, batch in fr.input_batches(geom):
                assert batch.dtype == np.float32 and batch.shape[0] == 3 and np.abs(batch).max() <= 32768.0
                for r, row in enumerate(batch):
                    a = fr.stages(row, n_fft, hop, T, window, filters)
                    b = fr.stages(row, n_fft, hop, T, window, filters, use_rfft=True)
                    tag = (wname, fname, name, r)
                    assert (np.abs(a.amp - b.amp) <= fr.amp_bound(a)).all(), tag
                    assert np.abs(a.logmel - b.logmel).max() <= fr.FEATURE_ATOL / 4, tag
                    assert np.abs(fr.emulate_f32_tail(a.power, f32) - a.logmel).max() <= fr.FEATURE_ATOL / 4, tag
                    assert np.abs(a.features - b.features).max() <= fr.FEATURE_ATOL / 4, tag


def test_reflect_padding_is_not_symmetric_padding():
    """The edge impulses of the shared inputs are what tells np.pad's "reflect" (edge sample not repeated) from "symmetric"."""
    n_fft, hop, _, T, _ = geom = fr.GEOMETRIES[3]
    batches = dict(fr.input_batches(geom))
    n = T * hop
    for row, at in ((batches["impulses-head"][0], 0), (batches["impulses-head"][1], 1), (batches["impulses-head"][2], n - 2),
                    (batches["impulse-tail-dc"][0], n - 1)):
        assert np.flatnonzero(row).tolist() == [at]
        x = np.zeros(n, np.float32)
        x[:n] = row
        sym = np.pad(x, n_fft // 2, mode="symmetric")
        ref = np.pad(x, n_fft // 2, mode="reflect")
        assert not np.array_equal(sym, ref)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_sample_makes_the_whole_utterance_nan(bad):
    """The reference's semantics the GPU front-end follows: np.maximum and ndarray.max propagate NaN, so one NaN (or Inf: Inf - Inf in
    the DFT, 0 * Inf in the mel projection) sample leaves no finite feature; oracle/cpu_ref agrees."""
    wav = synthetic_waveform(4, 2.0)
    wav[12345] = bad
    n_fft, hop, _, T, _ = fr.WHISPER
    st = fr.stages(wav, n_fft, hop, T, fr.hann(n_fft), fr.mel_filters(fr.WHISPER), use_rfft=True)
    assert np.isnan(st.features).all() and st.features.shape == (80, 3000)
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.isnan(cpu_ref.log_mel_spectrogram(wav)).all()
    small = fr.GEOMETRIES[3]
    x = np.random.default_rng(1).uniform(-1, 1, small[3] * small[1]).astype(np.float32)
    x[777] = bad
    for use_rfft in (False, True):
        assert np.isnan(fr.stages(x, small[0], small[1], small[3], fr.hann(small[0]), fr.mel_filters(small), use_rfft).features).all()


def test_whisper_batch_inputs_have_the_floors_and_lengths_they_are_meant_to():
    """The Whisper-geometry batch of the GPU tests: the loud row's floor is max - 8 with many elements on it, the quiet row's is the
    1e-10 clamp (-1.5), and audio.valid_frames on the reference's own columns gives ceil((n_in + n_fft / 2) / hop)."""
    import torch
    from whisper_trtllm_amd import audio
    n_fft, hop, _, T, _ = fr.WHISPER
    rows, lens = fr.whisper_floor_batch()
    feats = [fr.stages(r, n_fft, hop, T, fr.hann(n_fft), fr.mel_filters(fr.WHISPER), use_rfft=True) for r in rows]
    loud, quiet, clip = feats
    assert loud.logmel.max() - 8.0 > -10.0 + 1.0
    on_floor = loud.features == loud.features.min()
    assert 0.2 < on_floor.mean() < 0.95 and abs(loud.features.min() - (loud.logmel.max() - 8.0 + 4.0) / 4.0) < 1e-6
    assert quiet.logmel.max() - 8.0 < -10.0 and quiet.features.min() == -1.5 and (quiet.features == -1.5).mean() > 0.5
    for geom in (fr.WHISPER, fr.WHISPER_V3):       # the float32 budget of these rows, as for the small geometries' inputs
        f64 = fr.mel_filters(geom)
        for r in rows + [fr.whisper_plain_row()]:
            st = fr.stages(r, n_fft, hop, T, fr.hann(n_fft), f64, use_rfft=True)
            assert np.abs(fr.emulate_f32_tail(st.power, fr.pad_filters(f64, geom[4])) - st.logmel).max() <= fr.FEATURE_ATOL / 4
    # a frame lies wholly in the zero padding from t * hop - n_fft / 2 >= n_in on; the loud row's own floor makes identical columns
    # too, so the full-length count is taken on a row without a floor
    plain = fr.stages(fr.whisper_plain_row(), n_fft, hop, T, fr.hann(n_fft), fr.mel_filters(fr.WHISPER), use_rfft=True)
    expected = [min(T, -(-(n + n_fft // 2) // hop)) for n in [30 * 16000] + lens[1:]]
    assert expected == [3000, 502, 42]
    assert audio.valid_frames(torch.from_numpy(np.stack([plain.features, quiet.features, clip.features]))) == expected
    for f, v in zip((quiet, clip), expected[1:]):
        pad = f.features[:, v:]
        assert (pad == pad[:, :1]).all() and (pad == (max(-10.0, f.logmel.max() - 8.0) + 4.0) / 4.0).all()
        assert not (f.features[:, v - 1] == pad[:, 0]).all()
