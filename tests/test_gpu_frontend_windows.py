"""GPU: the windowed log-mel front-end (wt_logmel_forward_windows, LogMelFrontend.windows): window b = samples
[offsets[b], offsets[b] + n_valid[b]) of one flat buffer, zero-padded to the handle's window and reflected at the WINDOW's edges.
Pinned bitwise against wt_logmel_forward on a copy of each slice (whose own accuracy tests/test_gpu_frontend_kernels.py holds), at
handles of 192 and 3000 frames; a NaN one sample before and one sample behind a window must not reach it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
HOP = 160


@pytest.fixture(scope="module")
def wt():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    w._lib.load()
    return w


def _windows(n_frames):
    """(offset, n_valid) inside a buffer of 2.5 windows: the head, an offset that is no multiple of the hop, a full window ending with
    the buffer, tails shorter than the window (one of them no multiple of the hop either), and a window of one sample."""
    W = n_frames * HOP
    total = 2 * W + W // 2 + 37
    return total, [(0, W), (HOP * 7 + 53, W), (total - W, W), (total - W // 3, W // 3), (total - 1001, 1001), (total - 1, 1), (W + 11, 1)]


@pytest.mark.parametrize("n_frames", [192, 3000])
def test_windows_are_bitwise_the_forward_of_a_copied_slice(wt, n_frames):
    fe = wt.audio.LogMelFrontend(n_frames=n_frames)
    assert fe.n_frames == n_frames
    total, wins = _windows(n_frames)
    gen = torch.Generator().manual_seed(n_frames)
    flat = (torch.randn(total, generator=gen) * 0.1).cuda()
    got = fe.windows(flat, [o for o, _ in wins], [n for _, n in wins])
    assert got.shape == (len(wins), 80, n_frames) and torch.isfinite(got).all()
    for k, (o, n) in enumerate(wins):
        want = fe(flat[o:o + n].clone()[None])[0]
        assert torch.equal(got[k], want), (n_frames, k, o, n, float((got[k] - want).abs().max()))
    # the windows of one call are independent of their order and of their neighbours in the call
    back = fe.windows(flat, [o for o, _ in wins[::-1]], [n for _, n in wins[::-1]])
    assert torch.equal(back.flip(0), got)
    assert torch.equal(fe.windows(flat, [wins[1][0]], [wins[1][1]])[0], got[1])
    # the window length is the handle's: a longer n_valid is trimmed, as wt_logmel_forward trims
    W = n_frames * HOP
    assert torch.equal(fe.windows(flat, [5], [W + 99])[0], fe(flat[5:5 + W + 99].clone()[None])[0])


@pytest.mark.parametrize("n_frames", [192, 3000])
def test_a_nan_next_to_a_window_does_not_reach_it(wt, n_frames):
    fe = wt.audio.LogMelFrontend(n_frames=n_frames)
    W = n_frames * HOP
    gen = torch.Generator().manual_seed(7)
    flat = (torch.randn(3 * W, generator=gen) * 0.1).cuda()
    wins = [(W + 13, W), (W + 13, W // 2 + 1), (2 * W - 40, 1)]
    clean = fe.windows(flat, [o for o, _ in wins], [n for _, n in wins])
    for k, (o, n) in enumerate(wins):
        dirty = flat.clone()
        dirty[o - 1] = float("nan")            # one sample before the window (where a reflection into the neighbour would look)
        dirty[o + n] = float("nan")            # and the first sample behind it (where zero padding begins)
        got = fe.windows(dirty, [o], [n])[0]
        assert torch.isfinite(got).all() and torch.equal(got, clean[k]), (n_frames, k)
        dirty[o] = float("nan")                # inside: it must show (the reference propagates NaN)
        assert torch.isnan(fe.windows(dirty, [o], [n])[0]).any()


def test_more_windows_than_one_launch_carries_and_the_refusals(wt):
    fe = wt.audio.LogMelFrontend(n_frames=192)
    W = 192 * HOP
    flat = (torch.randn(4 * W, generator=torch.Generator().manual_seed(3)) * 0.1).cuda()
    offs = [(977 * k) % (3 * W) for k in range(19)]          # 19 windows: two launches of the DFT kernel (16 + 3)
    got = fe.windows(flat, offs, [W - k for k in range(19)])
    want = torch.cat([fe(flat[o:o + W - k].clone()[None]) for k, o in enumerate(offs)])
    assert torch.equal(got, want)
    for offsets, n_valid in (([0], [0]), ([-1], [5]), ([4 * W - 4], [5]), ([], []), ([0, 1], [5])):
        with pytest.raises(ValueError):
            fe.windows(flat, offsets, n_valid)
    with pytest.raises(ValueError):
        fe.windows(flat[None], [0], [5])
    lib, L = wt._lib.load(), wt._lib
    off, val = (ctypes.c_int64 * 1)(0), (ctypes.c_int32 * 1)(0)
    out = torch.empty(1, 80, 192, device="cuda")
    assert lib.wt_logmel_forward_windows(fe._handle, flat.data_ptr(), off, val, 1, out.data_ptr(), None) == -22 and "window 0" in L.last_error()
    off[0], val[0] = -3, 5
    assert lib.wt_logmel_forward_windows(fe._handle, flat.data_ptr(), off, val, 1, out.data_ptr(), None) == -22
