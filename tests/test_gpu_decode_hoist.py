"""The decode step's q|k|v and pair launches with the residual half of the folded cross-attention query hoisted (DESIGN.md section 5;
debug hooks wt_dbg_skinny_qkv_hoist and wt_dbg_skinny_pair_hoisted, which fill their launches through the helpers the engine uses).

u = fold_w . [a ; h] + fold_c is computed as uh = fold_wh . h + fold_c (a passenger range of the q|k|v launch) and u = fold_wa . a + uh
(second half of the pair launch).  What must hold:
  * the q|k|v range of the two-range launch is BITWISE the q|k|v launch on its own (q, the appended k / v rows, every other cache byte);
  * uh against float64 within the bound of test_gpu_kernels.py::test_skinny, 3e-5 * max(1, max |reference|);
  * h1 of the new pair launch is BITWISE that of the pair launch it replaces;
  * u against float64 of fold_w . [a ; h] + fold_c within 1e-5, the bound test_gpu_kernels.py::test_folded_query_adversarial_rows puts on
    the query q = (u - mean . r) . rstd + t: q is linear in u with slope rstd, and the residual rows here have unit variance (rstd = 1
    to a few percent), so a bound on q is the same bound on u.
References are plain torch in float64 on the CPU; half weights are exact in float64.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MAX_ROWS = 16
S_CAP = 8
U_BOUND = 1e-5


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


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@functools.lru_cache(maxsize=None)
def _layer(d, w_half):
    """One decoder layer's operands of the two launches (CPU tensors, never modified): LayerNorm, q|k|v, out-projection, folded query."""
    gen = torch.Generator().manual_seed(77 + d + w_half)
    rn = lambda *s: torch.randn(*s, generator=gen)
    cast = (lambda t: t.half()) if w_half else (lambda t: t)
    L = dict(g=rn(d) + 1.0, be=rn(d), Wqkv=cast(rn(3 * d, d) * d ** -0.5), bqkv=rn(3 * d), Wo=cast(rn(d, d) * d ** -0.5), bo=rn(d),
             Wf=cast(rn(d, 2 * d) * (2 * d) ** -0.5), c=rn(d))
    L["Wa"], L["Wh"] = L["Wf"][:, :d].contiguous(), L["Wf"][:, d:].contiguous()
    return L


def _rows(B, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, d, generator=gen), torch.randn(B, d, generator=gen)   # (a, h): unit variance rows


def _u_ref(L, a64, h):
    return torch.cat([a64, h.double()], 1) @ L["Wf"].double().T + L["c"].double()


@pytest.mark.parametrize("self_len", [0, 5])
@pytest.mark.parametrize("w_half", [0, 1])
@pytest.mark.parametrize("d", [128, 384, 1024])
@pytest.mark.parametrize("B", [1, 3, 8, 16])   # 16: the eight-wave, K-split instantiation of batch 9-16
def test_two_range_qkv_launch(lib, B, d, w_half, self_len):
    H = d // 64
    L = _layer(d, w_half)
    _, h = _rows(B, d, 5 * B + d)
    h = h * 2.0 + 0.3
    ref_uh = h.double() @ L["Wh"].double().T + L["c"].double()
    dev = {k: L[k].cuda() for k in ("g", "be", "Wqkv", "bqkv", "Wh", "c")}
    hd = h.cuda()
    _, sl = _i32([self_len] * B)
    sc = torch.zeros(lib.wt_dbg_skinny_qkv_append_scratch_bytes(), dtype=torch.uint8, device="cuda")
    pat = 0x7fc12345   # the buffers carry the rows of the widest template: rows >= B, and every cache row but self_len, stay untouched

    def buffers():
        return (torch.full((MAX_ROWS, d), pat, dtype=torch.int32, device="cuda"), torch.full((MAX_ROWS, H, S_CAP, 64), pat + 1, dtype=torch.int32, device="cuda"),
                torch.full((MAX_ROWS, H, S_CAP, 64), pat + 2, dtype=torch.int32, device="cuda"))
    for w_nt in (0, 1):
        q0, k0, v0 = buffers()
        q1, k1, v1 = buffers()
        uh = torch.full((MAX_ROWS, d), pat + 3, dtype=torch.int32, device="cuda")
        assert lib.wt_dbg_skinny_qkv_append(P(hd), P(dev["g"]), P(dev["be"]), P(dev["Wqkv"]), P(dev["bqkv"]), P(q0), P(k0), P(v0), sl, B, d, S_CAP,
                                            w_half, 0, w_nt, 0.125, P(sc), _stream()) == 0
        assert lib.wt_dbg_skinny_qkv_hoist(P(hd), P(dev["g"]), P(dev["be"]), P(dev["Wqkv"]), P(dev["bqkv"]), P(q1), P(k1), P(v1), sl, P(dev["Wh"]),
                                           P(dev["c"]), P(uh), B, d, S_CAP, w_half, 0, w_nt, 0.125, P(sc), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(q0, q1) and torch.equal(k0, k1) and torch.equal(v0, v1)
        assert not bool((q1[:B] == pat).any()) and not bool((k1[:B, :, self_len] == pat + 1).any())   # ... and the range did run
        uhh = uh.cpu()
        assert torch.equal(uhh[B:], torch.full_like(uhh[B:], pat + 3))
        err = (uhh[:B].view(torch.float32).double() - ref_uh).abs().max().item()
        print(f"B {B} d {d} half {w_half} nt {w_nt}: uh err {err:.3e}")
        assert err < 3e-5 * max(1.0, ref_uh.abs().max().item()), err
    assert torch.equal(hd.cpu(), h)


def _uh_on_device(lib, L, dev, hd, B, d, w_half):
    """uh by the plain GEMV hook (the passenger range runs the same kernel body over the same staged rows)"""
    uh = torch.full((B, d), float("nan"), device="cuda")
    fn = lib.wt_dbg_skinny_f16 if w_half else lib.wt_dbg_skinny
    assert fn(P(hd), None, None, P(dev["Wh"]), P(dev["c"]), None, P(uh), B, d, d, 4, 0, 1.0, _stream()) == 0
    return uh


@pytest.mark.parametrize("w_half", [0, 1])
@pytest.mark.parametrize("d", [128, 384, 1024])
@pytest.mark.parametrize("B", [1, 3, 8, 16])
def test_pair_launch_with_hoisted_residual_half(lib, B, d, w_half):
    L = _layer(d, w_half)
    a, h = _rows(B, d, 9 * B + d)
    dev = {k: L[k].cuda() for k in ("Wo", "bo", "Wf", "c", "Wa", "Wh")}
    ad, hd = a.cuda(), h.cuda()
    h1_old = torch.full((B, d), float("nan"), device="cuda")
    u_old = torch.full((B, d), float("nan"), device="cuda")
    pair = lib.wt_dbg_skinny_pair_f16 if w_half else lib.wt_dbg_skinny_pair
    assert pair(P(ad), P(dev["Wo"]), P(dev["bo"]), P(hd), P(h1_old), d, d, P(ad), P(hd), P(dev["Wf"]), P(dev["c"]), P(u_old), d, 2 * d, B, _stream()) == 0
    uh = _uh_on_device(lib, L, dev, hd, B, d, w_half)
    ref = _u_ref(L, a.double(), h)
    h1 = torch.full((B, d), float("nan"), device="cuda")
    u = torch.full((B, d), float("nan"), device="cuda")
    assert lib.wt_dbg_skinny_pair_hoisted(P(ad), None, P(dev["Wo"]), P(dev["bo"]), P(hd), P(h1), P(dev["Wa"]), P(uh), P(u), B, d, w_half, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(h1.view(torch.int32), h1_old.view(torch.int32))
    err, err_old = (u.cpu().double() - ref).abs().max().item(), (u_old.cpu().double() - ref).abs().max().item()
    print(f"B {B} d {d} half {w_half}: u err {err:.3e} (single 2d-long dot product: {err_old:.3e})")
    assert err < U_BOUND, err
    assert torch.equal(hd.cpu(), h) and torch.equal(ad.cpu(), a)


@pytest.mark.parametrize("B,H,length", [(8, 16, 447), (3, 6, 1), (8, 16, 130)])
def test_pair_launch_merges_two_split_partials(lib, B, H, length):
    """The context arrives as the two split partials of a self-attention with the merge deferred (length 1: the second split is empty)."""
    d, cap = 64 * H, 448
    L = _layer(d, 0)
    _, h = _rows(B, d, 3 * B + d)
    gen = torch.Generator().manual_seed(900 + B)
    q, k, v = torch.randn(B, d, generator=gen) * 0.5, torch.randn(B, H, cap, 64, generator=gen), torch.randn(B, H, cap, 64, generator=gen)
    dev = {k_: L[k_].cuda() for k_ in ("Wo", "bo", "Wf", "c", "Wa", "Wh")}
    qd, kd, vd, hd = q.cuda(), k.cuda(), v.cuda(), h.cuda()
    part = torch.full((B, H, 2, 68), float("nan"), device="cuda")
    h1_old = torch.full((B, d), float("nan"), device="cuda")
    u_old = torch.full((B, d), float("nan"), device="cuda")
    assert lib.wt_dbg_self_attention_then_pair(P(qd), P(kd), P(vd), P(part), P(dev["Wo"]), P(dev["bo"]), P(hd), P(h1_old), P(dev["Wf"]), P(dev["c"]),
                                               P(u_old), B, H, cap, length, _stream()) == 0
    uh = _uh_on_device(lib, L, dev, hd, B, d, 0)
    h1 = torch.full((B, d), float("nan"), device="cuda")
    u = torch.full((B, d), float("nan"), device="cuda")
    assert lib.wt_dbg_skinny_pair_hoisted(None, P(part), P(dev["Wo"]), P(dev["bo"]), P(hd), P(h1), P(dev["Wa"]), P(uh), P(u), B, d, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(h1.view(torch.int32), h1_old.view(torch.int32))
    # the context the launch staged: the merge of the partials it was given, in float64 (isolates the GEMV from the attention's own error)
    p64 = part.cpu().double()
    o, m, l = p64[..., :64], p64[..., 64], p64[..., 65]
    wgt = torch.exp(m - m.max(-1, keepdim=True).values)
    a64 = ((wgt.unsqueeze(-1) * o).sum(2) / (wgt * l).sum(2, keepdim=True)).reshape(B, d)
    err = (u.cpu().double() - _u_ref(L, a64, h)).abs().max().item()
    print(f"B {B} H {H} length {length}: u err {err:.3e}")
    assert torch.isfinite(u).all() and err < U_BOUND, err


def test_chained_launches_pick_up_new_inputs_at_the_same_addresses(lib):
    """q|k|v (+ uh) then pair at d = 1024, batch 8, twice over the same buffers with the inputs overwritten in place between the runs: the
    second u is that of the second inputs (a uh left over from the first run would miss the bound by orders of magnitude)."""
    B, d, H = 8, 1024, 16
    L = _layer(d, 0)
    dev = {k: L[k].cuda() for k in ("g", "be", "Wqkv", "bqkv", "Wo", "bo", "Wa", "Wh", "c")}
    a1, h1_in = _rows(B, d, 4242)
    a2, h2_in = _rows(B, d, 4343)
    ad, hd = a1.cuda(), h1_in.cuda()
    q = torch.zeros(B, d, device="cuda")
    kc, vc = torch.zeros(B, H, S_CAP, 64, device="cuda"), torch.zeros(B, H, S_CAP, 64, device="cuda")
    uh, hout, u = (torch.full((B, d), float("nan"), device="cuda") for _ in range(3))
    sc = torch.zeros(lib.wt_dbg_skinny_qkv_append_scratch_bytes(), dtype=torch.uint8, device="cuda")
    _, sl = _i32([3] * B)
    results = []
    for a, h in ((a1, h1_in), (a2, h2_in)):
        ad.copy_(a), hd.copy_(h)
        assert lib.wt_dbg_skinny_qkv_hoist(P(hd), P(dev["g"]), P(dev["be"]), P(dev["Wqkv"]), P(dev["bqkv"]), P(q), P(kc), P(vc), sl, P(dev["Wh"]),
                                           P(dev["c"]), P(uh), B, d, S_CAP, 0, 0, 1, 0.125, P(sc), _stream()) == 0
        assert lib.wt_dbg_skinny_pair_hoisted(P(ad), None, P(dev["Wo"]), P(dev["bo"]), P(hd), P(hout), P(dev["Wa"]), P(uh), P(u), B, d, 0,
                                              _stream()) == 0
        torch.cuda.synchronize()
        results.append((u.cpu().double(), hout.cpu().double(), q.cpu().double()))
    for (ug, hg, qg), a, h in zip(results, (a1, a2), (h1_in, h2_in)):
        err = (ug - _u_ref(L, a.double(), h)).abs().max().item()
        print(f"chain: u err {err:.3e}")
        assert err < U_BOUND, err
        ref_h1 = h.double() + a.double() @ L["Wo"].double().T + L["bo"].double()
        assert (hg - ref_h1).abs().max().item() < 2e-5                      # test_skinny_pair's bound
        ref_q = 0.125 * F.linear(F.layer_norm(h.double(), (d,), L["g"].double(), L["be"].double(), 1e-5), L["Wqkv"].double()[:d], L["bqkv"].double()[:d])
        assert (qg - ref_q).abs().max().item() < 3e-5 * max(1.0, ref_q.abs().max().item())
    stale = (results[1][0] - (torch.cat([a2, h1_in], 1).double() @ L["Wf"].double().T + L["c"].double())).abs().max().item()
    assert stale > 1e3 * U_BOUND   # the check above can tell a stale uh from a fresh one
