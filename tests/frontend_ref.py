"""Plain numpy fp64 reference of the log-mel front-end (csrc/frontend.hip) for ANY geometry, stage by stage, and the inputs the
front-end tests share.  The restatement follows HF WhisperFeatureExtractor._np_extract_fbank_features over audio_utils.spectrogram
like oracle/cpu_ref.log_mel_spectrogram (which is fixed to Whisper's geometry and returns the last stage only); the DFT is the
definition, a matrix product, so that it shares nothing with an FFT's index bookkeeping."""
from collections import namedtuple

import numpy as np

Stages = namedtuple("Stages", "amp power logmel features absum")

# (n_fft, hop, n_mels, n_frames T, npw) -> the kernel paths it runs, derived from n_fft: ksteps = n_fft / 4 k-steps of the MFMA loop,
# n_bins = n_fft / 2 + 1, nbt = ceil(n_bins / 16) bin tiles split (nbt + 1) / 2 | nbt / 2 over the two wave halves; T % 64 is the tail
# of the last 64-frame block, npw % 16 == 0 sends the mel GEMM to the LDS-DMA kernel.
GEOMETRIES = [
    (16, 5, 8, 70, 12),         # ksteps 4; n_bins 9 -> nbt 1: the upper half-waves own no bin tile (nb = 0); second block of 6 frames
    (28, 7, 5, 64, 16),         # ksteps 7 (odd: both `kk + 1 < ksteps` tails); n_bins 15 -> nbt 1; T = 64 exactly; npw 16 -> DMA GEMM
    (36, 12, 128, 130, 20),     # ksteps 9 (odd); n_bins 19 -> nbt 2 (1 | 1); 128 mels = the width of tile[64][129]; blocks 64 + 64 + 2
    (64, 16, 20, 200, 36),      # ksteps 16; n_bins 33 -> nbt 3: unequal halves (2 | 1); last block of 8 frames
    (64, 16, 20, 200, 48),      # the same DFT with npw 48 = 16 * nbt -> DMA GEMM with three K tiles, 15 zero power columns
    (16, 40, 8, 70, 12),        # hop > n_fft: frames do not overlap, samples between them are never read
    (444, 111, 80, 65, 224),    # ksteps 111 (odd); n_bins 223 -> nbt 14 (7 | 7): all 2 * DFT_MAX_BT accumulators; block of 1 frame; DMA GEMM
]
WHISPER = (400, 160, 80, 3000, 204)
WHISPER_V3 = (400, 160, 128, 3000, 204)

FEATURE_ATOL = 2e-5   # tests/test_frontend.py's bar for the features against the oracle (measured ~1e-6); kept for every stage after the DFT


def derived(geom):
    """The kernel-path quantities of a geometry, as csrc/frontend.hip derives them."""
    n_fft, hop, n_mels, T, npw = geom
    n_bins = n_fft // 2 + 1
    nbt = (n_bins + 15) // 16
    return dict(n_bins=n_bins, ksteps=n_fft // 4, nbt=nbt, nb_low=(nbt + 1) // 2, nb_high=nbt - (nbt + 1) // 2, tail=T % 64,
                blocks=(T + 63) // 64, dma_gemm=npw % 16 == 0, n_samples=T * hop)


def hann(n_fft):
    return np.hanning(n_fft + 1)[:-1].astype(np.float64)


def asymmetric_window(n_fft, seed=0):
    """Random positive fp64 window with no symmetry: a frame read backwards under it has another power spectrum (under the symmetric
    Hann window it has the same one, so a k -> n_fft - k slip between samples and window would go unseen)."""
    return np.random.default_rng(1000 + seed).uniform(0.1, 1.0, n_fft)


def mel_filters(geom):
    """[n_mels, n_bins] fp64: the slaney bank of the product at this geometry's sizes."""
    from whisper_trtllm_amd import audio
    return np.ascontiguousarray(audio.mel_filter_bank(derived(geom)["n_bins"], geom[2]).T)


def random_filters(geom, seed=0):
    """[n_mels, n_bins] fp64, dense and non-negative: every mel row and every power column counts (the slaney bank at a small n_bins
    leaves many of 128 rows empty)."""
    return np.random.default_rng(2000 + seed).uniform(0.0, 0.05, (geom[2], derived(geom)["n_bins"]))


def pad_filters(filters, npw):
    """What wt_logmel_create takes: f32 [n_mels][npw], columns >= n_bins zero."""
    out = np.zeros((filters.shape[0], npw), dtype=np.float32)
    out[:, :filters.shape[1]] = filters.astype(np.float32)
    return out


def dft_matrices(n_fft):
    """cos and -sin of 2 pi bin k / n_fft, [n_bins, n_fft] fp64, the argument reduced mod n_fft in integers."""
    n_bins = n_fft // 2 + 1
    ang = 2.0 * np.pi * ((np.arange(n_bins)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    return np.cos(ang), -np.sin(ang)


def frames_of(wave, n_fft, hop, n_frames):
    """[n_frames + 1, n_fft] fp64: zero-pad / trim to n_frames * hop samples, reflect-pad n_fft / 2, frame with the hop."""
    n_samples = n_frames * hop
    x = np.zeros(n_samples, dtype=np.float32)
    w = np.asarray(wave, dtype=np.float32)[:n_samples]
    x[:len(w)] = w
    x = np.pad(x, [(n_fft // 2, n_fft // 2)], mode="reflect").astype(np.float64)
    num = 1 + (x.size - n_fft) // hop
    assert num == n_frames + 1
    return x[np.arange(n_fft)[None, :] + hop * np.arange(num)[:, None]]


def stages(wave, n_fft, hop, n_frames, window, filters, use_rfft=False):
    """wave f32 [n_in], window fp64 [n_fft], filters fp64 [n_mels, n_bins] -> Stages, the last frame dropped in every one:
    amp [T, n_bins] fp64 (|spectrum| after its complex64 rounding), power [T, n_bins] fp64, logmel [T, n_mels] f32 (before the clamp),
    features [n_mels, T] f32, absum [T] = sum_k |x_k w_k| (the scale of the DFT's rounding error)."""
    fw = frames_of(wave, n_fft, hop, n_frames) * np.asarray(window, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        if use_rfft:
            spec = np.fft.rfft(fw, axis=-1)
        else:
            c, s = dft_matrices(n_fft)
            spec = fw @ c.T + 1j * (fw @ s.T)
        spec = spec.astype(np.complex64)
        re, im = spec.real.astype(np.float64), spec.imag.astype(np.float64)
        power = re * re + im * im
        mel = np.maximum(1e-10, power @ np.asarray(filters, dtype=np.float64).T)
        logmel = np.asarray(np.log10(mel), np.float32)[:-1]
        feats = (np.maximum(logmel, logmel.max() - 8.0) + 4.0) / 4.0
    return Stages(np.sqrt(power)[:-1], power[:-1], logmel, np.ascontiguousarray(feats.T), np.abs(fw).sum(axis=1)[:-1])


def amp_bound(ref):
    """Per element bound of |sqrt(pw) - amp| for an fp64 DFT whose spectrum is rounded to complex64 and whose power is stored as
    float32, against `ref` (another such DFT): 2^-22 amp (a float32 ulp of the complex64 rounding on either side plus the float32
    store of the power) + 2 n_fft 2^-53 absum[t] (the fp64 dot-product bound gamma_n sum |x_k w_k| of both DFTs).  [T, n_bins]."""
    n_fft = 2 * (ref.amp.shape[1] - 1)
    return 2.0 ** -22 * ref.amp + 2.0 * n_fft * 2.0 ** -53 * ref.absum[:, None]


def emulate_f32_tail(power, filters32):
    """The stages after the DFT as the GPU runs them, in numpy float32: power stored as float32, float32 mel projection with the
    float32 filter bank, float32 log10.  power [T, n_bins] fp64, filters32 f32 [n_mels, npw] -> logmel f32 [T, n_mels]."""
    p32 = np.zeros((power.shape[0], filters32.shape[1]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p32[:, :power.shape[1]] = power.astype(np.float32)
        mel = p32 @ filters32.T
        return np.log10(np.maximum(np.float32(1e-10), mel)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def input_lengths(geom):
    n_fft, hop, _, T, _ = geom
    n = T * hop
    return [1, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n - 1, n, n + 1, n + 3 * hop]


def _tone(n, cycles_per_sample, phase=0.3):
    return np.cos(2.0 * np.pi * cycles_per_sample * np.arange(n) + phase)


def _impulse(n, at):
    x = np.zeros(n)
    x[at] = 1.0
    return x


def input_batches(geom):
    """[(name, f32 [3, n_in])]: three different rows per batch, |x| <= 1 with one row of each batch rescaled to 32768 (int16 range fed
    unnormalised).  Every n_in of `input_lengths` carries noise, an off-bin tone and an impulse on its last sample (trimmed away
    when n_in > n_samples: that row is silence); the full length also carries a bin-centred tone, DC and single impulses on samples
    0, 1, n_samples - 2 and n_samples - 1, the samples that reflect padding and symmetric padding treat differently."""
    n_fft, hop, _, T, _ = geom
    n_samples = T * hop
    rng = np.random.default_rng(n_fft * 1000 + hop)
    centred, off_bin = (n_fft // 8 + 1) / n_fft, (n_fft // 8 + 1.37) / n_fft
    out = []
    for n_in in input_lengths(geom):
        rows = [rng.uniform(-1.0, 1.0, n_in), 32768.0 * 0.9 * _tone(n_in, off_bin), _impulse(n_in, n_in - 1)]
        out.append((f"n_in={n_in}", np.stack(rows).astype(np.float32)))
    n = n_samples
    out.append(("tones", np.stack([0.8 * _tone(n, centred), 32768.0 * rng.uniform(-1.0, 1.0, n), 0.5 * _tone(n, off_bin, 1.1)]).astype(np.float32)))
    out.append(("impulses-head", np.stack([_impulse(n, 0), 32768.0 * _impulse(n, 1), _impulse(n, n - 2)]).astype(np.float32)))
    out.append(("impulse-tail-dc", np.stack([_impulse(n, n - 1), np.full(n, 0.7), 32768.0 * np.full(n, -1.0)]).astype(np.float32)))
    return out


def whisper_floor_batch():
    """Three utterances at Whisper's geometry with three different floors -> ([loud, quiet, clip], their lengths in samples).
    loud: 30 s, an int16-scale 440 Hz tone for 8 s over noise 50 dB below it for 15 s and 90 dB below it after, so the floor is max - 8
    with the first half of the row above it and the second half on it;
    quiet: 5 s of noise at 1e-3, whose max - 8 lies below the 1e-10 clamp, so the floor is -10 -> -1.5;  clip: 0.4 s at normal level."""
    rng = np.random.default_rng(77)
    sr = 16000
    loud = rng.uniform(-1.0, 1.0, 30 * sr)
    loud[:15 * sr] *= 100.0
    loud[:8 * sr] += 32768.0 * 0.9 * _tone(8 * sr, 440.0 / sr)
    quiet = 1e-3 * rng.uniform(-1.0, 1.0, 5 * sr)
    n = int(0.4 * sr)
    clip = 0.5 * _tone(n, 700.0 / sr) + 0.05 * rng.standard_normal(n)
    rows = [loud.astype(np.float32), quiet.astype(np.float32), clip.astype(np.float32)]
    return rows, [len(r) for r in rows]


def whisper_plain_row():
    """30 s at normal level, noise over a tone: no element on a floor, no two identical columns."""
    rng = np.random.default_rng(78)
    n = 30 * 16000
    return (0.4 * _tone(n, 523.0 / 16000) + 0.1 * rng.standard_normal(n)).astype(np.float32)
