"""prefill_attn_kernel alone (kernels_prefill.hip, through wt_dbg_prefill_attention), per element against torch fp64.

The kernel attends nq queries of every (utterance, head) over the first nk keys of a head cache [B][H][cap][64] in one launch: the causal
form (the prompt's self attention, query t sees keys 0..t) and the full form (its cross attention).  Shapes: H = 2, B = 3; causal
nq = nk in {1, 2, 33, 65, 130} -- fewer queries than a wave holds, both sides of the 64-key tile, and 130 = two 128-query blocks over three
key tiles --, full (nq, nk) in {(1, 96), (33, 100), (5, 1500)}.  The cache is larger than the key count (160 rows; 1504 for 1500 keys) and
everything behind the valid keys is NaN: the clamped loads of a correct kernel never read it.

Bound per case: max(2e-5, 8 x |att_fp32_cpu - att_fp64|_inf), att_fp32_cpu the same torch attention in float32 on the host -- the
construction of test_gpu_decode_attention_forms.py: a margin of 8 over the float32 reference's own error for the kernel's other
summation order (two interleaved halves of 64-key tiles, fp32 MFMA accumulation) and the hardware exp.  Every test prints err / bound (-s).
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
B, H, D = 3, 2, 128
CAUSAL = [1, 2, 33, 65, 130]
FULL = [(1, 96), (33, 100), (5, 1500)]


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


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def _cap(nk):
    return 160 if nk <= 130 else 1504


def _attention(q, k, v, nk, causal, scale):
    """q [B][nq][H*64], k / v [B][H][cap][64] -> [B][nq][H*64] in the operands' dtype."""
    nq = q.shape[1]
    qh = q.view(B, nq, H, 64).transpose(1, 2)
    s = (qh @ k[:, :, :nk].transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(torch.ones(nq, nk, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v[:, :, :nk]).transpose(1, 2).reshape(B, nq, H * 64)


@functools.lru_cache(maxsize=None)
def _inputs(nq, nk):
    """Shared and never modified: q [B][nq][128], k / v [B][H][cap][64] with NaN behind key nk."""
    cap = _cap(nk)
    q = _rand(B, nq, D, seed=71)
    k, v = _rand(B, H, cap, 64, seed=72), _rand(B, H, cap, 64, seed=73)
    k[:, :, nk:] = float("nan")
    v[:, :, nk:] = float("nan")
    return q, k, v


def _launch(lib, q, k, v, nk, causal, scale, ldc=D, ldq=None):
    """The hook on NaN-sentinel output of B * nq + 4 rows of ldc columns; returns the whole buffer [B * nq + 4][ldc] on the host."""
    nq, cap = q.shape[1], k.shape[2]
    qd = q.cuda()
    if ldq is not None:   # the queries as columns [0, 128) of wider rows
        wide = _nan(B, nq, ldq)
        wide[:, :, :D] = qd
        qd = wide
    out = _nan(B * nq + 4, ldc)
    kd, vd = k.cuda(), v.cuda()
    rc = lib.wt_dbg_prefill_attention(P(qd), P(kd), P(vd), P(out), B, H, nq, nk, cap, qd.shape[2], ldc, int(causal), scale, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu()


def _check(lib, name, q, k, v, nk, causal, scale, ldc=D, ldq=None):
    nq = q.shape[1]
    ref = _attention(q.double(), k.double(), v.double(), nk, causal, scale)
    ref32 = _attention(q, k, v, nk, causal, scale)
    bound = max(2e-5, 8.0 * (ref32.double() - ref).abs().max().item())
    out = _launch(lib, q, k, v, nk, causal, scale, ldc, ldq)
    got = out[:B * nq, :D].reshape(B, nq, D)
    assert torch.isfinite(got).all(), name
    err = (got.double() - ref).abs().max().item()
    print(f"\n{name}: err {err:.2e} bound {bound:.2e} ratio {err / bound:.3f}")
    assert err < bound, (name, err, bound)
    # nothing outside the nq context rows (and, with a wider leading dimension, outside their 128 columns) is written
    assert _untouched(out[B * nq:]) and _untouched(out[:, D:]), name
    return got, ref, bound


@pytest.mark.parametrize("n", CAUSAL)
def test_causal_form_against_fp64(lib, n):
    q, k, v = _inputs(n, n)
    _check(lib, f"causal nq = nk = {n}", q, k, v, n, True, 0.125)


@pytest.mark.parametrize("nq,nk", FULL)
def test_full_form_against_fp64(lib, nq, nk):
    q, k, v = _inputs(nq, nk)
    _check(lib, f"full nq {nq} nk {nk}", q, k, v, nk, False, 1.0 if nk == 1500 else 0.125)


@pytest.mark.parametrize("causal", [True, False])
def test_context_and_query_leading_dimensions(lib, causal):
    """The prefill writes the self-attention context into the left half of a [M][2d] buffer (ldc = 2d), beside the layer input."""
    nq, nk = (65, 65) if causal else (33, 100)
    q, k, v = _inputs(nq, nk)
    a, _, _ = _check(lib, f"ldc 2d causal {causal}", q, k, v, nk, causal, 0.125, ldc=2 * D)
    b, _, _ = _check(lib, f"ldq 3d causal {causal}", q, k, v, nk, causal, 0.125, ldq=3 * D)
    plain = _launch(lib, q, k, v, nk, causal, 0.125)[:B * nq].reshape(B, nq, D)
    assert torch.equal(a, plain) and torch.equal(b, plain)


def _adversarial(kind, nq, nk):
    q = _rand(B, nq, D, seed=81) * 0.5
    k, v = _rand(B, H, 160, 64, seed=82), _rand(B, H, 160, 64, seed=83)
    qh = q.view(B, nq, H, 64)
    if kind == "wide":            # scores within about +-74, the softmax near one-hot
        q = q * 5.0
    elif kind == "wider":         # scores within about +-143
        q = q * 10.0
    elif kind in ("offset+100", "offset-100"):   # every score of query 0 moves by c, the others by c (q_t . q_0) / |q_0|^2
        q0 = qh[:, 0].unsqueeze(2)               # [B][H][1][64]
        k = k + float(kind[6:]) * q0 / q0.norm(dim=-1, keepdim=True) ** 2
    elif kind == "flat":          # all keys equal: uniform weights, the mean of the visible values
        k = k[:, :, :1].expand_as(k).clone()
    elif kind == "dominant":      # one key far above the rest for every query, late in the sequence (the running maximum jumps there)
        u = torch.nn.functional.normalize(_rand(64, seed=84), dim=0)
        q = (qh + u).reshape(B, nq, D)
        k[:, :, 20] = 30.0 * u
    else:
        raise AssertionError(kind)
    k[:, :, nk:] = float("nan")
    v[:, :, nk:] = float("nan")
    return q.contiguous(), k.contiguous(), v.contiguous()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("kind", ["wide", "wider", "offset+100", "offset-100", "flat", "dominant"])
def test_online_softmax_on_adversarial_score_ranges(lib, kind, causal):
    nq, nk = (33, 33) if causal else (33, 100)
    q, k, v = _adversarial(kind, nq, nk)
    got, ref, _ = _check(lib, f"{kind} causal {causal}", q, k, v, nk, causal, 1.0)
    if kind == "flat":
        vv = v.double()[:, :, :nk]
        mean = (vv.cumsum(2)[:, :, :nq] / torch.arange(1, nq + 1).view(1, 1, nq, 1)) if causal else vv.mean(2, keepdim=True).expand(B, H, nq, 64)
        assert (ref - mean.transpose(1, 2).reshape(B, nq, D)).abs().max().item() < 1e-12


@pytest.mark.parametrize("causal", [True, False])
def test_equals_decode_attention_query_by_query(lib, causal):
    """Query t of the prefill against dec_attn_kernel on that query alone (wt_dbg_decode_attention, the query pre-scaled, t + 1 or nk keys):
    what the forced-stepping path computes for the same position."""
    nq, nk = (33, 33) if causal else (33, 100)
    q, k, v = _inputs(nq, nk)
    got, ref, bound = _check(lib, f"vs dec_attn causal {causal}", q, k, v, nk, causal, 0.125)
    kd, vd = k.cuda(), v.cuda()
    qs = (q * 0.125).cuda()   # exact: a power of two
    dec = _nan(nq, B, D)
    cnt, part = torch.zeros(B, H, dtype=torch.int32, device="cuda"), _nan(B, H, 1, 68)
    for t in range(nq):
        qt = qs[:, t].contiguous()
        assert lib.wt_dbg_decode_attention(P(qt), P(kd), P(vd), P(part), P(cnt), P(dec[t]), B, H, k.shape[2], t + 1 if causal else nk, 1, _stream()) == 0
    torch.cuda.synchronize()
    dec = dec.cpu().transpose(0, 1)
    diff = (got - dec).abs().max().item()
    print(f"\nprefill vs dec_attn causal {causal}: max diff {diff:.2e} bound {bound:.2e}")
    assert diff < bound


def test_launcher_refuses_what_it_cannot_launch(lib):
    q, k, v = _inputs(33, 33)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    out = _nan(B * 33, D)

    def call(nq=33, nk=33, cap=160, ldq=D, ldc=D, causal=1):
        return lib.wt_dbg_prefill_attention(P(qd), P(kd), P(vd), P(out), B, H, nq, nk, cap, ldq, ldc, causal, 0.125, _stream())

    assert call(nk=32) != 0            # causal: nk must equal nq
    assert call(nk=161, causal=0) != 0  # more keys than the cache holds
    assert call(nq=0) != 0 and call(nk=0, causal=0) != 0
    assert call(ldq=D - 4) != 0 and call(ldc=D + 2) != 0
    torch.cuda.synchronize()
    assert _untouched(out)


# ---- the prefill's query finish (wt_dbg_prefill_query_finish) ----------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("rows,d", [(5, 128), (7, 384), (1, 1280), (130, 1280)])
def test_query_finish_against_fp64(lib, rows, d, alias):
    """q = (u - mean(h1) . r) * rstd(h1) + t per row, one wave per row and four rows per workgroup: row counts that are no multiple of 4,
    d = 1280 (the last of the five float4 a lane holds), a residual row with a large common offset (two-pass statistics), q aliasing u.
    Bound: max(2e-5, 8 x the same formula in float32 on the host against fp64)."""
    u, h1 = _rand(rows, d, seed=91), _rand(rows, d, seed=92) * 2.0 + 30.0
    r, t = _rand(d, seed=93), _rand(d, seed=94)

    def ref(u, h1, r, t):
        mu = h1.mean(1, keepdim=True)
        return (u - mu * r) * (h1.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() + t

    want = ref(u.double(), h1.double(), r.double(), t.double())
    bound = max(2e-5, 8.0 * (ref(u, h1, r, t).double() - want).abs().max().item())
    buf = _nan(rows + 3, d)
    ud, hd, rd, td = u.cuda(), h1.cuda(), r.cuda(), t.cuda()
    if alias:
        buf[:rows] = ud
        ud = buf
    assert lib.wt_dbg_prefill_query_finish(P(ud), P(hd), P(rd), P(td), P(buf), rows, d, _stream()) == 0
    torch.cuda.synchronize()
    out = buf.cpu()
    err = (out[:rows].double() - want).abs().max().item()
    print(f"\nquery finish rows {rows} d {d} alias {alias}: err {err:.2e} bound {bound:.2e} ratio {err / bound:.3f}")
    assert torch.isfinite(out[:rows]).all() and err < bound
    assert _untouched(out[rows:]) and torch.equal(hd.cpu(), h1)
    assert lib.wt_dbg_prefill_query_finish(P(ud), P(hd), P(rd), P(td), P(buf), rows, 1284, _stream()) != 0   # more than five float4 per lane
