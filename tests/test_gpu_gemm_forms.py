"""The addressing forms of the encoder GEMMs that only the engine reached before: the two convolutions (fp32-MFMA, x3 and fp16), the
cross-K/V projection (fp32-MFMA and x3), the producers of bf16 operand planes, and the plane wiring of the x3 GEMM itself.

The hooks build their launches with the engine's own helpers (csrc/wt_common.h: conv_gemm_params, conv_ws_clear, cross_kv_gemm_params,
cross_kv_x3), so what is tested here is what wt_encoder_forward / cross_kv_project launch.  References are float64; the error bars are
per element, normalised by sum_k |a_k||w_k| + |b| of that element, so rows of small magnitude are checked as closely as large ones."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TILES = [0, 128, 192, 256]
# fp32 accumulation (the fp32 MFMA, or the six bf16 partial products of x3) against float64, per element relative to sum |a||w| + |b|:
# about 2^-24 per rounding of a partial sum; measured well below 2^-21.  2^-20 leaves headroom at K = 3 x 1280 and still fails a dropped
# x3 term wherever the term does not cancel (test_gpu_kernels.py::test_gemm_x3_is_an_fp32_gemm shows that margin).
REL = 2.0 ** -20
GELU_SLOPE = 1.13        # max |d gelu / dx|
GELU_APPROX = 2e-7       # |gelu_erf - gelu| <= 1.3e-7 max(|x|, 1) (wt_common.h), plus the rounding of its result


@pytest.fixture(scope="module")
def lib():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    return w._lib.load()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def split3(x):
    """Host form of the kernels' split: b1 = rn(x), b2 = rn(x - b1), b3 = rn(x - b1 - b2), round to nearest even, as [3][...] bf16.
    The two subtractions are exact in fp32."""
    x = x.float()
    b1 = x.to(torch.bfloat16)
    r1 = x - b1.float()
    b2 = r1.to(torch.bfloat16)
    b3 = (r1 - b2.float()).to(torch.bfloat16)
    return torch.stack([b1, b2, b3])


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _nan_bytes(n):
    return torch.full((n,), 255, dtype=torch.uint8, device="cuda")   # all-ones: NaN as float, half and bf16


# ------------------------------------------------------------------------------------------------ x3 GEMM plane wiring, exact
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K", [(128, 128, 16), (200, 136, 48), (257, 300, 64), (390, 520, 144)])
def test_gemm_x3_plane_wiring_is_exact(lib, tile, M, N, K):
    """Planes written directly (flag bit 1): A plane i holds integers in [-3, 3] times 2^-2i, W plane j integers in [-3, 3] times 2^-2j,
    bias integers in [-8, 8].  Every partial product is then a multiple of 2^-8 below 9, and every partial sum of the six kept products
    over K <= 144 stays below 6 x 9 x 144 + 8 < 2^13: 21 significant bits at most, so the fp32 accumulator is exact in any order and the
    output must EQUAL the float64 sum.  Pair (i, j) alone: sum_k A_i W_j^T + bias for the six kept pairs (i + j <= 4, 1-based),
    bias alone for the three dropped ones; all planes together: the six-term sum.  Catches a wrong plane stride, a dropped or duplicated
    product and a transposed fragment map without any tolerance.  One K step to nine (the pipeline has three stages), ragged M / N."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    Ai = [torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** (-2 * i) for i in range(3)]
    Wj = [torch.randint(-3, 4, (N, K), generator=g).double() * 2.0 ** (-2 * j) for j in range(3)]
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    bd = bias.cuda()
    zA, zW = torch.zeros(M, K, dtype=torch.double), torch.zeros(N, K, dtype=torch.double)
    C = torch.empty(M, N, device="cuda")

    def run(Apl, Wpl):
        a_pl = torch.stack(Apl).to(torch.bfloat16).cuda()
        w_pl = torch.stack(Wpl).to(torch.bfloat16).cuda()
        assert torch.equal(a_pl.double().cpu(), torch.stack(Apl)) and torch.equal(w_pl.double().cpu(), torch.stack(Wpl))
        C.fill_(float("nan"))
        assert lib.wt_dbg_gemm_x3_tile(None, None, P(bd), None, P(C), M, N, K, 0, P(a_pl), P(w_pl), 2, tile, _stream()) == 0
        torch.cuda.synchronize()
        return C.cpu()

    full = bias.double().expand(M, N).clone()
    for i in range(3):
        for j in range(3):
            Apl = [Ai[p] if p == i else zA for p in range(3)]
            Wpl = [Wj[p] if p == j else zW for p in range(3)]
            kept = i + j <= 2          # 0-based: i + j <= 4 in 1-based plane numbers
            want = bias.double().expand(M, N) + (Ai[i] @ Wj[j].T if kept else 0.0)
            if kept:
                full += Ai[i] @ Wj[j].T
            got = run(Apl, Wpl)
            assert torch.equal(got, want.float()), f"plane pair A{i + 1}.W{j + 1} (kept={kept}), tile {tile}"
    got = run(Ai, Wj)
    assert torch.equal(got, full.float()), f"all planes, tile {tile}"


# ------------------------------------------------------------------------------------------------ producers of bf16 planes, exact
@pytest.mark.parametrize("rows,d", [(7, 128), (33, 1024), (1502, 384), (6, 1280), (45, 1280)])
def test_layernorm_split_is_the_split_of_layernorm(lib, rows, d):
    """launch_layernorm_split's planes are bitwise the round-to-nearest-even split of launch_layernorm's fp32 row (the same kernel, only
    the stores differ), d up to the kernel's 1280, rows not a multiple of the four rows per workgroup."""
    x, w, b = (_rand(rows, d, seed=5, scale=3.0) + 0.7).cuda(), _rand(d, seed=6).cuda(), _rand(d, seed=7).cuda()
    y = torch.full((rows, d), float("nan"), device="cuda")
    pl = torch.full((3, rows, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib.wt_dbg_layernorm(P(x), P(w), P(b), P(y), rows, d, _stream()) == 0
    assert lib.wt_dbg_layernorm_split(P(x), P(w), P(b), P(pl), rows, d, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert torch.equal(bits(pl), bits(split3(y)))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K,act", [(333, 200, 48, 1), (333, 200, 48, 0), (1500, 1536, 64, 1), (700, 520, 32, 0)])
def test_gemm_x3_three_plane_output_is_the_split_of_the_fp32_output(lib, tile, M, N, K, act):
    """The out_split epilogue (fc1's GELU output, conv1's output) stores bitwise the round-to-nearest-even split of the value the fp32
    epilogue of the same launch stores: interior sub-tiles (fast epilogue) and ragged edges (generic epilogue), every tile form."""
    A, W, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3).cuda()
    a_pl, w_pl = split3(A).cuda(), split3(W).cuda()
    C = torch.full((M, N), float("nan"), device="cuda")
    C3 = torch.full((3, M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib.wt_dbg_gemm_x3_tile(None, None, P(b), None, P(C), M, N, K, act, P(a_pl), P(w_pl), 2, tile, _stream()) == 0
    assert lib.wt_dbg_gemm_x3_tile(None, None, P(b), None, P(C3), M, N, K, act, P(a_pl), P(w_pl), 3, tile, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(C).all()
    assert torch.equal(bits(C3), bits(split3(C)))


# ------------------------------------------------------------------------------------------------ the two convolutions vs float64
def _conv_weights(C, d, seed):
    from whisper_trtllm_amd.builder import Builder
    w1 = _rand(d, C, 1, 3, seed=seed, scale=(3 * C) ** -0.5)
    w2 = _rand(d, d, 1, 3, seed=seed + 1, scale=(3 * d) ** -0.5)
    b1, b2 = _rand(d, seed=seed + 2, scale=0.5), _rand(d, seed=seed + 3, scale=0.5)
    g1 = torch.from_numpy(Builder._conv_as_gemm(w1.numpy()))   # [d][3C], the converter's layout
    g2 = torch.from_numpy(Builder._conv_as_gemm(w2.numpy()))
    return w1[:, :, 0], w2[:, :, 0], b1, b2, g1, g2


def _mel(B, C, S, seed):
    from whisper_trtllm_amd.synthetic import PAD_MEL
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, C, 2 * S, generator=g) * 2 - 1
    for b in range(B):                      # a constant pad tail behind the "audio", of a different length per utterance
        mel[b, :, (2 * S * (b + 2)) // (B + 3):] = PAD_MEL
    return mel


class _Convs:
    """One hook call on fresh (NaN-filled) buffers; reads back conv1's output and the pad rows from the scratch."""

    def __init__(self, lib, mode, tile, B, C, S, d, mel, g1, g2, b1, b2, pos):
        self.B, self.S, self.d, self.mode = B, S, d, mode
        nbytes = lib.wt_dbg_encoder_convs_scratch_bytes(B, C, S, d, mode)
        rows = B * (2 * S + 2)
        self.n_melT, self.n_c1 = rows * C + 4 * C, rows * d + 4 * d
        esz = 6 if mode == 1 else 4
        self.c1_off = (self.n_melT * esz + 255) // 256 * 256
        assert nbytes == self.c1_off + self.n_c1 * esz
        if mode == 1:
            w1, w2 = split3(g1).cuda(), split3(g2).cuda()
        elif mode == 2:
            w1, w2 = g1.half().cuda(), g2.half().cuda()
        else:
            w1, w2 = g1.cuda(), g2.cuda()
        self.scratch = _nan_bytes(nbytes)
        self.out = torch.full((B, S, d), float("nan"), device="cuda")
        mel_d, b1d, b2d, pos_d = mel.cuda(), b1.cuda(), b2.cuda(), pos.cuda()
        assert lib.wt_dbg_encoder_convs(P(mel_d), P(w1), P(b1d), P(w2), P(b2d), P(pos_d), P(self.out), P(self.scratch), B, C, S, d, mode,
                                        tile, _stream()) == 0
        torch.cuda.synchronize()

    def region(self, off, n, C):
        """[B][2S+2][C] rows of a workspace region as float64 (x3: the exact sum of its three planes)"""
        rows = self.B * (2 * self.S + 2)
        raw = self.scratch[off:]
        if self.mode == 1:
            v = raw[: 6 * n].view(torch.bfloat16).view(3, n).double()
            planes = v[:, : rows * C].view(3, self.B, 2 * self.S + 2, C)
            return planes.sum(0), planes
        if self.mode == 2:
            v = raw[: 2 * n].view(torch.float16)[: rows * C].double()
        else:
            v = raw[: 4 * n].view(torch.float32)[: rows * C].double()
        v = v.view(self.B, 2 * self.S + 2, C)
        return v, v[None]

    def c1(self):
        return self.region(self.c1_off, self.n_c1, self.d)

    def melT(self, C):
        return self.region(0, self.n_melT, C)


def _bar(pre, norm, K):
    # plus one rounding of the running sum per 16-deep K step where the sum grows coherently (2^-24 (K / 16) |pre|)
    return GELU_SLOPE * (REL * norm + 2.0 ** -24 * (K / 16) * pre.abs()) + GELU_APPROX * pre.abs().clamp(min=1.0)


CONV_CASES = [
    (1, 80, 40, 128),     # S = 40: conv2's c_rows_per_batch < 64 -> generic epilogue everywhere
    (3, 128, 40, 384),
    (16, 80, 12, 128),    # one tile spans several utterances in both convolutions
    (5, 128, 100, 512),
    (2, 80, 160, 1024),
    (1, 128, 1500, 384),
    (2, 80, 1500, 1280),
]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,C,S,d", CONV_CASES)
def test_encoder_convolutions_vs_fp64(lib, B, C, S, d, mode):
    """Both convolutions as the engine launches them, against F.conv1d in float64: conv1 (k 3, pad 1) + GELU read back from the
    workspace, conv2 (k 3, stride 2, pad 1) + GELU + embed_positions.  conv2's reference is formed from conv1's output as the kernel left
    it (three planes, half or float), so each launch is held to its own bar.  Every row must be written (buffers start as NaN), the pad
    rows of the workspace must be exactly zero, and the melT planes must be the exact split of the mel.  fp16 (mode 2): operands rounded
    to half as the engine rounds them (mel, weights, conv1's output); conv1 is held to the half rounding of its store (2^-11 relative)
    on top of the fp32 accumulation bar."""
    w1, w2, b1, b2, g1, g2 = _conv_weights(C, d, seed=C + d)
    mel = _mel(B, C, S, seed=S + B)
    pos = _rand(S, d, seed=9)
    tiles = TILES if mode == 1 else [0]
    dev = "cuda"
    for tile in tiles:
        r = _Convs(lib, mode, tile, B, C, S, d, mel, g1, g2, b1, b2, pos)
        if mode == 2:
            mel_r, w1r, w2r = mel.half().double(), w1.half().double(), w2.half().double()
        else:
            mel_r, w1r, w2r = mel.double(), w1.double(), w2.double()
        mel_r, w1r, w2r, b1r, b2r = (t.to(dev) for t in (mel_r, w1r, w2r, b1.double(), b2.double()))
        # conv1
        z1 = F.conv1d(mel_r, w1r, b1r, padding=1)                                  # [B][d][2S]
        n1 = F.conv1d(mel_r.abs(), w1r.abs(), b1r.abs(), padding=1)
        c1, c1_planes = r.c1()
        c1 = c1.to(dev)
        got1 = c1[:, 1: 2 * S + 1].transpose(1, 2)                                  # [B][d][2S]
        assert torch.isfinite(got1).all(), f"conv1 rows not written (tile {tile})"
        assert (c1_planes[:, :, 0] == 0).all() and (c1_planes[:, :, 2 * S + 1] == 0).all(), "conv1 pad rows"
        bar1 = _bar(z1, n1, 3 * C) + (2.0 ** -11 * F.gelu(z1).abs() if mode == 2 else 0.0)
        ex1 = ((got1 - F.gelu(z1)).abs() / bar1).max().item()
        assert ex1 <= 1.0, f"conv1: error {ex1:.2f} x its bar (mode {mode}, tile {tile})"
        # melT (x3: the exact split of the mel, bitwise; other modes: the mel / its half rounding)
        mT, mT_planes = r.melT(C)
        assert (mT_planes[:, :, 0] == 0).all() and (mT_planes[:, :, 2 * S + 1] == 0).all(), "melT pad rows"
        if mode == 1:
            want = split3(mel.transpose(1, 2)).cuda()
            assert torch.equal(bits(mT_planes[:, :, 1: 2 * S + 1].to(torch.bfloat16)), bits(want))
        else:
            assert torch.equal(mT[:, 1: 2 * S + 1].cpu(), mel_r.cpu().transpose(1, 2))
        # conv2 from conv1's output as stored
        x2 = got1
        z2 = F.conv1d(x2, w2r, b2r, stride=2, padding=1)                           # [B][d][S]
        n2 = F.conv1d(x2.abs(), w2r.abs(), b2r.abs(), stride=2, padding=1)
        want2 = (F.gelu(z2) + pos.double().to(dev).T[None]).transpose(1, 2)          # [B][S][d]
        bar2 = (_bar(z2, n2, 3 * d) + 2.0 ** -24 * want2.transpose(1, 2).abs()).transpose(1, 2)
        got2 = r.out.double()
        assert torch.isfinite(got2).all(), f"conv2 rows not written (tile {tile})"
        ex2 = ((got2 - want2).abs() / bar2).max().item()
        print(f"convs B={B} C={C} S={S} d={d} mode={mode} tile={tile}: conv1 {ex1:.3f}, conv2 {ex2:.3f} of the bar")
        assert ex2 <= 1.0, f"conv2: error {ex2:.2f} x its bar (mode {mode}, tile {tile})"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_encoder_convolutions_smaller_batch_same_rows(lib, mode):
    """A second call on the same scratch with a smaller batch (other plane strides) gives bitwise the same rows."""
    B, C, S, d = 16, 128, 40, 384
    _, _, b1, b2, g1, g2 = _conv_weights(C, d, seed=11)
    mel, pos = _mel(B, C, S, seed=12), _rand(S, d, seed=13)
    first = _Convs(lib, mode, 0, B, C, S, d, mel, g1, g2, b1, b2, pos)
    out_full = first.out.clone()
    nb = 5
    w1, w2 = (split3(g1).cuda(), split3(g2).cuda()) if mode == 1 else ((g1.half().cuda(), g2.half().cuda()) if mode == 2 else (g1.cuda(), g2.cuda()))
    out = torch.full((nb, S, d), float("nan"), device="cuda")
    mel_d, b1d, b2d, pos_d = mel[:nb].contiguous().cuda(), b1.cuda(), b2.cuda(), pos.cuda()
    assert lib.wt_dbg_encoder_convs(P(mel_d), P(w1), P(b1d), P(w2), P(b2d), P(pos_d), P(out), P(first.scratch), nb, C, S, d, mode, 0,
                                    _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(out_full[:nb]))


# ------------------------------------------------------------------------------------------------ cross-K/V projection vs float64
KV_CASES = [  # B, H, rows_total, rows, cap, seq_off, layer_rows, row0
    (2, 2, 96, 96, 96, 0, 2, 0), (3, 6, 1500, 1500, 1500, 0, 3, 0), (1, 2, 96, 85, 96, 11, 1, 0), (2, 3, 160, 160, 160, 0, 2, 0),
    (1, 16, 1500, 1, 1500, 1499, 1, 0), (8, 16, 1500, 1500, 1500, 0, 8, 0),
    # rows 1 / 11 / 63 / 64: the generic epilogue and the engine's partial cross cache (m_c = 11)
    (2, 6, 1500, 11, 1500, 0, 2, 0), (3, 2, 96, 63, 96, 0, 3, 0), (2, 2, 64, 64, 64, 0, 2, 0), (4, 6, 1500, 1, 1500, 0, 4, 0),
    # row0 > 0 inside a pool of layer_rows utterance rows (continuous mode)
    (3, 6, 1500, 1500, 1500, 0, 8, 4), (2, 2, 96, 64, 96, 32, 5, 2), (2, 6, 1500, 11, 1500, 0, 6, 3),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,H,rows_total,rows,cap,seq_off,layer_rows,row0", KV_CASES)
def test_cross_kv_projection_vs_fp64(lib, B, H, rows_total, rows, cap, seq_off, layer_rows, row0, mode):
    """cross_kv_project's fp32-MFMA and x3 launches (EPI_KV_HEADS): utterance b lands in cache row row0 + b, sequence rows
    [seq_off, seq_off + rows), head-split [h][cap][64]; every other cache element keeps its sentinel.  Per-element bar against float64."""
    d = 64 * H
    A = _rand(B, rows_total, d, seed=51)
    W, bias = _rand(2 * d, d, seed=52, scale=d ** -0.5), _rand(2 * d, seed=53)
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    y = F.linear(Ad[:, :rows].double(), Wd.double(), bd.double())                    # [B][rows][2d]
    ny = F.linear(Ad[:, :rows].double().abs(), Wd.double().abs(), bd.double().abs())
    a_plane = B * rows_total * d
    scratch = torch.empty((a_plane * 6 + 255) // 256 * 256 + 12 * d * d, dtype=torch.uint8, device="cuda") if mode == 1 else None
    for tile in (TILES if mode == 1 else [0]):
        kc = torch.full((layer_rows, H, cap, 64), 7.0, device="cuda")
        vc = torch.full((layer_rows, H, cap, 64), 7.0, device="cuda")
        assert lib.wt_dbg_cross_kv(P(Ad), rows_total, P(Wd), P(bd), P(kc), P(vc), P(scratch), B, rows, H, cap, seq_off, layer_rows, row0,
                                   mode, tile, _stream()) == 0
        torch.cuda.synchronize()
        for which, cache in enumerate((kc, vc)):
            sl = slice(which * d, (which + 1) * d)
            ref = y[..., sl].reshape(B, rows, H, 64).transpose(1, 2)
            nrm = ny[..., sl].reshape(B, rows, H, 64).transpose(1, 2)
            got = cache[row0: row0 + B, :, seq_off: seq_off + rows].double()
            ex = ((got - ref).abs() / (REL * nrm + 2.0 ** -24 * (d / 16) * ref.abs())).max().item()
            assert ex <= 1.0, f"{'kv'[which]} cache: error {ex:.2f} x the bar (mode {mode}, tile {tile})"
            keep = torch.ones(layer_rows, H, cap, dtype=torch.bool, device="cuda")
            keep[row0: row0 + B, :, seq_off: seq_off + rows] = False
            assert (cache[keep] == 7.0).all(), f"{'kv'[which]} cache: a row outside the projected range was written"


# ------------------------------------------------------------------------------------------------ the fp32-MFMA encoder end to end
_CHILD = r"""
import sys
import numpy as np
import torch
import whisper_trtllm_amd as wt
import test_gpu_parity as tp
from conftest import GOLDEN_CASES, load_case
z, cfg, weights, mel = load_case(GOLDEN_CASES[0])
enc, _ = tp._engines(wt, cfg, weights)
print("gemm_mode", wt._lib.load().wt_engine_gemm_mode(enc.session._handle))
np.save(sys.argv[1], enc(torch.from_numpy(mel).cuda()).cpu().numpy())
"""


@pytest.mark.parametrize("switch,gemm_mode", [("WT_GEMM_X3", 0), ("WT_ATTN_X3", 1)])
def test_fp32_mfma_encoder_paths_match_golden(switch, gemm_mode, tmp_path):
    """The encoder with the fp32-MFMA GEMMs (WT_GEMM_X3=0) or the fp32-MFMA attention (WT_ATTN_X3=0) -- the A/B baseline and the fallback.
    The switches are latched once per process, so a fresh child runs the golden encoder cases of test_gpu_parity.py against the
    committed enc_out with that test's own tolerances.  That the switch took effect is observed first: a child with the switch and a
    control child without either switch encode the first golden case; the engine must report the expected GEMM mode, and the two outputs
    must differ bitwise (another kernel ran) while the control equals this process's own default-path output bitwise (so the difference
    is the switch, not run-to-run noise)."""
    import os
    import subprocess
    import sys

    import numpy as np
    import whisper_trtllm_amd as wt
    from conftest import GOLDEN_CASES, load_case
    from test_gpu_parity import _engines
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def child_env(**switches):
        env = {k: v for k, v in os.environ.items() if k not in ("WT_GEMM_X3", "WT_ATTN_X3")}
        env.update(WT_TUNING="1", **switches)
        env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests"), os.path.join(root, "oracle")] +
                                            ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        return env

    def encode(env, path):
        r = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout, np.load(path)

    env = child_env(**{switch: "0"})
    out_sw, got_sw = encode(env, str(tmp_path / "switched.npy"))
    assert f"gemm_mode {gemm_mode}" in out_sw, out_sw
    out_ctl, got_ctl = encode(child_env(), str(tmp_path / "control.npy"))
    assert "gemm_mode 1" in out_ctl, out_ctl
    assert not np.array_equal(got_sw, got_ctl), f"{switch}=0 changed nothing: the fp32-MFMA path did not run"
    z, cfg, weights, mel = load_case(GOLDEN_CASES[0])
    enc, _ = _engines(wt, cfg, weights)
    here = enc(torch.from_numpy(mel).cuda()).cpu().numpy()
    assert np.array_equal(here, got_ctl), "the default path differs between processes"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_parity.py::test_encoder_matches_golden_and_oracle"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
