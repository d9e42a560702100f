"""The greedy step's fused epilogues and token selection, per element (debug hooks wt_dbg_vocab_argmax, wt_dbg_skinny_qkv_append,
wt_dbg_greedy_select, wt_dbg_dec_embed -- each fills its launch through the helper the engine itself uses, csrc/wt_common.h).

References are plain torch in float64 on the CPU.  Tolerances (floating-point checks only; every id / index / bit check is exact):
  * logits, q, appended k / v rows: 3e-5 * max(1, max |reference|), the bound of test_gpu_kernels.py::test_skinny and
    ::test_skinny_half_weights (the same for every K and for both weight types: half weights are exact in float64);
  * half caches: that bound plus the rounding of the reference value to IEEE half (2^-11 relative, 2^-25 absolute below the normal range).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BATCHES = [1, 2, 3, 4, 5, 8, 9, 12, 16]
MAX_ROWS = 16
INT_MAX = 0x7fffffff
NINF = float("-inf")


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


def _scratch(nbytes):
    assert nbytes > 0
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_values(a, b):
    """equal element by element, NaN matching NaN (NaN payloads are not compared)"""
    an, bn = a.isnan(), b.isnan()
    zero = torch.zeros((), dtype=torch.float64)
    return torch.equal(an, bn) and torch.equal(torch.where(an, zero, a.double()), torch.where(bn, zero, b.double()))


# ---- torch.argmax semantics spelled out: NaN counts as the maximum, the lowest index wins ----
def _argmax_rows(v):
    """v [R][n] -> (values [R], indices [R])"""
    nan = v.isnan()
    first_nan = nan.to(torch.int8).argmax(1)                                # first maximal value = first NaN
    first_max = torch.where(nan, torch.full_like(v, NINF), v).argmax(1)     # first maximal value of a NaN-free row
    idx = torch.where(nan.any(1), first_nan, first_max)
    return v.gather(1, idx[:, None])[:, 0], idx


def _masked(logits, mask, at_begin):
    """Suppress (bit 0) and SuppressAtBegin (bit 1, rows with at_begin) as masked_fill(-inf); logits [B][N], mask uint8 [N], at_begin bool [B]"""
    m = mask.to(torch.int32)
    hit = ((m & 1) != 0)[None, :] | (((m & 2) != 0)[None, :] & at_begin[:, None])
    return logits.masked_fill(hit, NINF)


def _partials(masked, per, parts):
    """(max, argmax) of every row over the consecutive ranges [g * per, (g + 1) * per): values [B][parts], indices [B][parts]; a range
    past the end gives (-inf, INT_MAX), what a lane without rows holds"""
    B, N = masked.shape
    pad = parts * per - N
    assert pad >= 0
    x = torch.cat([masked, torch.full((B, pad), NINF, dtype=masked.dtype)], 1).reshape(B * parts, per)
    val, idx = _argmax_rows(x)
    idx = idx.reshape(B, parts) + torch.arange(parts)[None, :] * per
    idx = torch.where(idx < N, idx, torch.full_like(idx, INT_MAX))
    return val.reshape(B, parts), idx


def _merge(val, idx):
    """the argmax over partials: NaN first, then the larger value, then the lower index"""
    B = val.shape[0]
    out = []
    for b in range(B):
        best, bidx = NINF, INT_MAX
        for v, i in zip(val[b].tolist(), idx[b].tolist()):
            vn, bn = v != v, best != best
            better = (not bn or i < bidx) if vn else (not bn and (v > best or (v == best and i < bidx)))
            if better:
                best, bidx = v, i
        out.append(bidx)
    return out


# ---- the vocabulary GEMV's plan (skinny_plan, kernels_decoder.hip): rows per workgroup from B, N, K ----
def _plan(B, N, K):
    NB = 2 if B <= 2 else 4 if B <= 4 else 8 if B <= 8 else 16
    V, NW = (4, 4) if NB <= 8 else (2, 8)
    nsplit = 1
    while K // nsplit > 256 * V or K % nsplit:
        nsplit *= 2
    G = NW // nsplit
    target = (1024 if NB == 8 else 2048) // nsplit
    rpg = max(2, 2 * (-(-N // (2 * target))))
    groups = -(-N // rpg)
    return rpg, G, -(-groups // G)   # rows per row group (a wave, or the waves of a K-split), groups per workgroup, workgroups


def _vocab_configs():
    """Reduced cross product: at every K all nine B (so all four batch-width templates), both weight types in every template, both load
    policies in every template and weight type over the K, and an odd N in every template."""
    Ns = [51865, 51865, 51864, 51865, 1003, 51865, 7, 51865, 51864]
    out = []
    for ik, K in enumerate([384, 512, 768, 1024]):
        for ib, B in enumerate(BATCHES):
            out.append((K, B, Ns[ib], ib % 2, (ib // 2 + ik) % 2))
    return out


VOCAB_CONFIGS = _vocab_configs()
VOCAB_IDS = ["K%d-B%d-N%d-%s-nt%d" % (K, B, N, "f16" if h else "f32", nt) for K, B, N, h, nt in VOCAB_CONFIGS]
N_FULL = 51865


@functools.lru_cache(maxsize=1)
def _random_w(K):
    g = torch.Generator().manual_seed(1000 + K)
    return torch.randn(N_FULL, K, generator=g) * K ** -0.5


@functools.lru_cache(maxsize=1)
def _integer_w(K):
    g = torch.Generator().manual_seed(2000 + K)
    return torch.randint(-1, 2, (N_FULL, K), generator=g).float()


def _run_vocab(lib, X, g, be, W, bias, mask, cur_len, begin_index, xmode, w_nt, fused=1, trace=True):
    """-> (part_val [B][parts], part_idx, logits or None), on the CPU"""
    B, K = X.shape
    N = W.shape[0]
    w_half = int(W.dtype == torch.float16)
    parts = lib.wt_dbg_vocab_argmax_parts(B, N, K, w_half)
    assert parts == _plan(B, N, K)[2]
    pv = torch.full((B, parts), float("nan"), device="cuda")
    pi = torch.full((B, parts), -7, dtype=torch.int32, device="cuda")
    lg = torch.full((B, N), float("nan"), device="cuda") if trace else None
    sc = _scratch(lib.wt_dbg_vocab_argmax_scratch_bytes())
    _, cl = _i32(cur_len)
    rc = lib.wt_dbg_vocab_argmax(P(X), P(g), P(be), P(W), P(bias), P(mask), cl, begin_index, B, N, K, xmode, w_half, w_nt, fused, P(lg),
                                 P(pv), P(pi), P(sc), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return pv.cpu(), pi.cpu(), (lg.cpu() if trace else None)


def _mixed_cur_len(B, begin_index):
    """some rows at begin_index, some not (B == 1: the one row at it)"""
    return np.array([begin_index if b % 3 != 1 else begin_index + 2 for b in range(B)], dtype=np.int32)


def _random_vocab_case(K, B, N, w_half, seed):
    g0 = torch.Generator().manual_seed(seed)
    X = torch.randn(B, K, generator=g0) * 2.0 + 0.3
    g = torch.randn(K, generator=g0) + 1.0
    be = torch.randn(K, generator=g0)
    W = _random_w(K)[:N]
    W = W.half() if w_half else W
    r = torch.rand(N, generator=g0)
    mask = ((r < 0.3).to(torch.uint8) | ((r > 0.2) & (r < 0.45)).to(torch.uint8) * 2)   # bit 0 only, both, bit 1 only
    ref = F.linear(F.layer_norm(X.double(), (K,), g.double(), be.double(), 1e-5), W.double())
    return X, g, be, W, mask, ref


@pytest.mark.parametrize("K,B,N,w_half,w_nt", VOCAB_CONFIGS, ids=VOCAB_IDS)
def test_vocab_argmax_random(lib, K, B, N, w_half, w_nt):
    """Random operands: the traced logits against float64 per element; every workgroup's partial against the argmax of the kernel's own
    traced logits over its rows, bitwise; the merge against the whole row; trace on / off; the token against float64."""
    begin = 4
    X, g, be, W, mask, ref = _random_vocab_case(K, B, N, w_half, 0)   # seed 0 clears the margin below at every configuration
    cur_len = _mixed_cur_len(B, begin)
    at_begin = torch.from_numpy(cur_len == begin)
    bound = 3e-5 * max(1.0, ref.abs().max().item())   # test_skinny / test_skinny_half_weights
    top2 = _masked(ref, mask, at_begin).topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).min().item()
    # (twice the bound: the winner and the runner-up may each move by it)
    assert margin > 2 * bound, f"float64 top-2 margin {margin:.3e} within the logits bound {bound:.3e}: pick another seed"
    dev = [t.cuda() for t in (X, g, be, W, mask)]
    pv, pi, lg = _run_vocab(lib, dev[0], dev[1], dev[2], dev[3], None, dev[4], cur_len, begin, 1, w_nt)
    err = (lg.double() - ref).abs().max().item()
    print(f"logits err {err:.3e} bound {bound:.3e} margin {margin:.3e}")
    assert err < bound, err
    rpg, G, parts = _plan(B, N, K)
    ev, ei = _partials(_masked(lg, mask, at_begin), rpg * G, parts)
    assert torch.equal(pi.long(), ei)
    assert torch.equal(_bits(pv), _bits(ev))
    whole = _argmax_rows(_masked(lg, mask, at_begin))[1].tolist()
    assert _merge(pv, pi) == whole
    assert whole == _argmax_rows(_masked(ref, mask, at_begin))[1].tolist()
    pv2, pi2, _ = _run_vocab(lib, dev[0], dev[1], dev[2], dev[3], None, dev[4], cur_len, begin, 1, w_nt, trace=False)
    assert torch.equal(_bits(pv2), _bits(pv)) and torch.equal(pi2, pi)


def _position_classes(B, N, K):
    """one id per position class the kernel distinguishes, each in a workgroup of its own where N allows: first / second row of a pair,
    first / last pair of a row group, last row of a workgroup, first row of the next one, the last row of N (odd N: a pair of one)"""
    rpg, G, parts = _plan(B, N, K)
    wg = rpg * G
    cls = []
    for i, off in enumerate([0, 1, rpg - 2, rpg - 1, wg - 1, wg, rpg, rpg + 1]):
        base = (1 + 2 * i) * wg if parts > 20 else 0
        cls.append(base + off)
    cls.append(N - 1)
    return sorted({c for c in cls if 0 <= c < N})


@pytest.mark.parametrize("K,B,N,w_half,w_nt", VOCAB_CONFIGS, ids=VOCAB_IDS)
def test_vocab_argmax_exact(lib, K, B, N, w_half, w_nt):
    """Small-integer X, W and bias: every logit is exact in fp32 in any summation order, so the expected partials do not need the trace."""
    begin = 3
    gen = torch.Generator().manual_seed(77 + K + B)
    X = torch.randint(-1, 2, (B, K), generator=gen).float()
    W = _integer_w(K)[:N].clone()
    rpg, G, parts = _plan(B, N, K)
    wg = rpg * G
    cur_len = _mixed_cur_len(B, begin)
    at_begin = torch.from_numpy(cur_len == begin)
    base = F.linear(X.double(), W.double())   # [B][N], integers
    assert base.abs().max().item() <= K
    Wd = (W.half() if w_half else W).cuda()
    Xd = X.cuda()
    cls = _position_classes(B, N, K)

    def run(bias, mask, Xr=Xd, Wr=Wd, expect=None):
        pv, pi, lg = _run_vocab(lib, Xr, None, None, Wr, bias.float().cuda(), mask.cuda(), cur_len, begin, 0, w_nt)
        masked = _masked(expect, mask, at_begin)
        ev, ei = _partials(masked, wg, parts)
        assert torch.equal(pi.long(), ei)
        assert _same_values(pv, ev)
        tok = _merge(pv, pi)
        assert tok == _argmax_rows(masked)[1].tolist()
        assert _same_values(lg, expect)
        return tok

    # the row maximum on a masked id at every position class: bit 0 on the even classes and bit 1 on the odd ones, then swapped
    for flip in (0, 1):
        bias, mask = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.uint8)
        for i, c in enumerate(cls):
            bias[c] = 4000 + 2000 * i   # (steps above the spread of the unplanted logits, |.| <= K)
            mask[c] = 1 + (i + flip) % 2
        tok = run(bias, mask, expect=base + bias)
        for b in range(B):   # the last class is the global maximum: taken unless its mask applies to the row
            top = cls[-1]
            assert (tok[b] == top) == (int(mask[top]) == 2 and not bool(at_begin[b]))
    # exact duplicates of the winning row in the second row of its pair, a later pair, a later wave and a later workgroup
    p = cls[0] if cls[0] + wg < N else 0
    dups = sorted({q for q in (p + 1, p + 2, p + rpg, p + wg, N - 1) if p < q < N})
    W2 = Wd.clone()
    bias = torch.zeros(N, dtype=torch.float64)
    bias[p] = 5000
    exp = base.clone()
    for q in dups:
        W2[q] = W2[p]
        bias[q] = 5000
        exp[:, q] = exp[:, p]
    tok = run(bias, torch.zeros(N, dtype=torch.uint8), Wr=W2, expect=exp + bias)
    assert tok == [p] * B
    # a NaN in one X row: that row's logits are all NaN, its token is the first unmasked id; the other rows are unaffected
    mask = torch.zeros(N, dtype=torch.uint8)
    mask[0] = 1
    if N > 2:
        mask[1] = 2
    for r in sorted({0, B - 1, min(1, B - 1)}):
        X2 = Xd.clone()
        X2[r, K // 2 + 1] = float("nan")
        exp = base.clone()
        exp[r] = float("nan")
        tok = run(torch.zeros(N, dtype=torch.float64), mask, Xr=X2, expect=exp)
        assert tok[r] == (2 if (at_begin[r] and N > 2) else 1)
    # a NaN in one W row under a mask (no effect) and in a later one not under a mask (every row's token)
    c1, c2 = cls[len(cls) // 2], cls[-1]
    if c1 != c2:
        W2 = Wd.clone()
        W2[c1, 3] = float("nan")
        W2[c2, K - 1] = float("nan")
        mask = torch.zeros(N, dtype=torch.uint8)
        mask[c1] = 1
        exp = base.clone()
        exp[:, c1] = float("nan")
        exp[:, c2] = float("nan")
        tok = run(torch.zeros(N, dtype=torch.float64), mask, Wr=W2, expect=exp)
        assert tok == [c2] * B
    # every id masked: index 0, in range
    tok = run(torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.uint8), expect=base)
    assert tok == [0] * B


# ---- q|k|v projection with the in-place cache append ----
@pytest.mark.parametrize("s_cap", [448, 40])
@pytest.mark.parametrize("w_half,kv_half", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("d", [384, 512, 768, 1024])
@pytest.mark.parametrize("B", BATCHES)
def test_qkv_append(lib, B, d, w_half, kv_half, s_cap):
    H = d // 64
    gen = torch.Generator().manual_seed(31 * B + d + s_cap)
    X = torch.randn(B, d, generator=gen) * 2.0 + 0.3
    W = torch.randn(3 * d, d, generator=gen) * d ** -0.5
    W = W.half() if w_half else W
    b = torch.randn(3 * d, generator=gen)
    g, be = torch.randn(d, generator=gen) + 1.0, torch.randn(d, generator=gen)
    # a different position per row, with 0 and s_cap - 1 among them
    self_len = np.array([0, s_cap - 1, 7, s_cap // 2, 1, s_cap - 2, 3, s_cap - 4, 11, s_cap // 2 + 5, 2, s_cap - 7, 5, s_cap - 9, 13,
                         s_cap // 2 - 6][:B], dtype=np.int32)
    if B == 1:
        self_len[0] = s_cap - 1 if (d // 128) % 2 else 0
    assert len(set(self_len.tolist())) == B and self_len.min() >= 0 and self_len.max() < s_cap
    scale = 0.125
    ref = F.linear(F.layer_norm(X.double(), (d,), g.double(), be.double(), 1e-5), W.double(), b.double())
    ref_q = ref[:, :d] * scale
    bound_q = 3e-5 * max(1.0, ref_q.abs().max().item())        # test_skinny / test_skinny_half_weights
    bound = 3e-5 * max(1.0, ref[:, d:].abs().max().item())     # the same for the k / v thirds (scale 1)
    # the buffers carry the rows of the widest template (16): rows >= B must stay untouched
    cdt, pat = (torch.int16, 0x7e11) if kv_half else (torch.int32, 0x7fc12345)
    kc = torch.full((MAX_ROWS, H, s_cap, 64), pat, dtype=cdt, device="cuda")
    vc = torch.full((MAX_ROWS, H, s_cap, 64), pat + 1, dtype=cdt, device="cuda")
    q = torch.full((MAX_ROWS, d), 0x7fc54321, dtype=torch.int32, device="cuda")
    sc = _scratch(lib.wt_dbg_skinny_qkv_append_scratch_bytes())
    dev = [t.cuda() for t in (X, g, be, W, b)]
    _, sl = _i32(self_len)
    for w_nt in (0, 1):
        kc.fill_(pat), vc.fill_(pat + 1), q.fill_(0x7fc54321)
        rc = lib.wt_dbg_skinny_qkv_append(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), P(q), P(kc), P(vc), sl, B, d, s_cap, w_half,
                                          kv_half, w_nt, scale, P(sc), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        qh = q.cpu()
        assert torch.equal(qh[B:], torch.full_like(qh[B:], 0x7fc54321))
        err = (qh[:B].view(torch.float32).double() - ref_q).abs().max().item()
        assert err < bound_q, err
        for third, (cache, fill) in enumerate([(kc, pat), (vc, pat + 1)], start=1):
            want = ref[:, third * d:(third + 1) * d].reshape(B, H, 64)
            rows = torch.stack([cache[r, :, int(self_len[r]), :] for r in range(B)]).cpu()
            got = rows.view(torch.float16 if kv_half else torch.float32).double()
            tol = bound + (want.abs() * 2.0 ** -11 + 2.0 ** -25 if kv_half else 0.0)
            assert bool(((got - want).abs() < tol).all()), (third, (got - want).abs().max().item())
            # every element outside row self_len[b] of each (b, h) is bitwise unchanged
            rest = cache.clone()
            for r in range(B):
                rest[r, :, int(self_len[r]), :] = fill
            assert bool((rest == fill).all()), third


# ---- greedy_select_kernel + greedy_finish_kernel<false> on crafted rows ----
def _chunk_len(V):
    """ids per chunk of greedy_select_kernel's eight chunks (16-byte path when V % 4 == 0)"""
    return 4 * (-(-(V // 4) // 8)) if V % 4 == 0 else -(-V // 8)


def _state(B, cur_len, pos, self_len, step, done=0, seq=5):
    st = np.zeros(4 + 3 * MAX_ROWS, dtype=np.int32)
    st[0], st[1], st[2], st[3] = done, B, step, seq
    st[4:4 + MAX_ROWS] = 900          # rows >= B: must come back unchanged
    st[4 + MAX_ROWS:4 + 2 * MAX_ROWS] = 901
    st[4 + 2 * MAX_ROWS:] = 902
    st[4:4 + B], st[4 + MAX_ROWS:4 + MAX_ROWS + B], st[4 + 2 * MAX_ROWS:4 + 2 * MAX_ROWS + B] = cur_len, pos, self_len
    return st


def _reference_step(logits, mask, forced, ids, unf, st, force_eos_step, force_rows, tok_emb, pos_emb, next_x, B, max_length, begin, eos, pad):
    """run.py's greedy step (Suppress -> SuppressAtBegin -> Force, forced EOS, pad after EOS, stop test) on the crafted rows"""
    st, ids, unf, next_x = st.copy(), ids.clone(), unf.clone(), next_x.clone()
    st[3] += 1
    if st[0]:
        return ids, unf, st, next_x
    cur, step, pos = int(st[4]), int(st[2]), int(st[4 + MAX_ROWS])
    at_begin = torch.from_numpy(st[4:4 + B] == begin)
    arg = _argmax_rows(_masked(logits, mask, at_begin))[1].tolist()
    alive = 0
    toks = []
    for b in range(B):
        tok = arg[b]
        if forced[cur] >= 0:
            tok = int(forced[cur])
        if force_eos_step >= 0 and step == force_eos_step:
            tok = eos
        if force_rows is not None and force_rows[b] >= 0 and step == force_rows[b]:
            tok = eos
        if not unf[b]:
            tok = pad
        ids[b, cur] = tok
        if tok == eos:
            unf[b] = 0
        alive += int(unf[b] != 0)
        toks.append(tok)
    st[4:4 + B] += 1
    st[4 + MAX_ROWS:4 + MAX_ROWS + B] += 1
    st[4 + 2 * MAX_ROWS:4 + 2 * MAX_ROWS + B] += 1
    st[1], st[2] = alive, step + 1
    if alive == 0 or cur + 1 >= max_length:
        st[0] = 1
    if cur + 1 < max_length:
        next_x[:B] = tok_emb[toks].float() + pos_emb[pos + 1]   # one fp32 add of the widened table row
    return ids, unf, st, next_x


def _crafted_logits(B, V, borders, eos, nan_masked, eos_row):
    """rows by role (b % 6): 0 a tie across a chunk border and on the last element, 1 the maximum on the last element, 2 NaNs (the first
    one under a mask), 3 all -inf, 4 the maximum under the begin mask (id 2), 5 random.  eos_row: that row's maximum is EOS instead."""
    gen = torch.Generator().manual_seed(V + 17 * B)
    lg = torch.randn(B, V, generator=gen)
    for b in range(B):
        role = b % 6
        if role == 0:
            for k in borders:
                lg[b, k - 1] = lg[b, k] = 9.0
            lg[b, V - 1] = 9.0
        elif role == 1:
            lg[b, V - 1] = 11.0
        elif role == 2:
            lg[b, nan_masked] = float("nan")
            lg[b, V - 2] = float("nan")
            lg[b, V - 1] = float("nan")
        elif role == 3:
            lg[b] = NINF
        elif role == 4:
            lg[b, 2] = 12.0
            lg[b, V // 2] = 10.0
    if eos_row is not None:
        lg[eos_row] = torch.randn(V, generator=gen)
        lg[eos_row, eos] = 20.0
    return lg


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("V", [51864, 51865, 1003, 5])
def test_greedy_select_and_finish(lib, V, B):
    d, max_length, begin, pos_rows = 64 if V > 2000 else 128, 12, 4, 16
    eos, pad = (V - 3, V - 4) if V > 5 else (3, 4)
    gen = torch.Generator().manual_seed(5 * V + B)
    tok_emb32 = torch.randn(V, d, generator=gen)
    pos_emb = torch.randn(pos_rows, d, generator=gen)
    nan_masked = 1
    mask0 = torch.zeros(V, dtype=torch.uint8)
    mask0[nan_masked] = 1   # bit 0 on the NaN row's first NaN
    mask0[2] = 2            # bit 1 on role 4's maximum
    if V > 5:
        mask0[7] = 3
    sc = _scratch(lib.wt_dbg_greedy_select_scratch_bytes(max_length))
    tables = {False: (tok_emb32, tok_emb32.cuda()), True: (tok_emb32.half(), tok_emb32.half().cuda())}
    pe_d = pos_emb.cuda()
    sources = [("chunks", 0)] + [("fused", n) for n in (1, 9, 130, 300)]
    per8 = _chunk_len(V)
    forced_tok = 6 if V > 6 else 0
    # role 0's ties sit across chunk borders of EVERY partial layout, so that all of them see the same logits
    pers = [per8] + [-(-V // n) for _, n in sources[1:]]
    borders = sorted({k for per in pers for k in (3 * per, 5 * per) if 0 < k < V - 1})
    # (name, cur_len, step, forced at cur_len, force_eos_step, force_eos_rows, rows finished on entry, EOS row, done on entry, full mask, half table)
    scenes = [
        ("at-begin", begin, 0, -1, -1, None, [1], None, 0, False, False),
        ("later", begin + 2, 2, -1, -1, None, [], None, 0, False, True),
        ("forced", begin + 1, 1, forced_tok, -1, None, [B - 1] if B > 2 else [], None, 0, False, False),
        ("forced+eos-step", begin + 1, 1, forced_tok, 1, None, [0] if B > 1 else [], None, 0, False, True),
        ("forced+eos-rows", begin + 1, 1, forced_tok, -1, [1 if b % 2 == 0 else (-1 if b % 4 == 1 else 3) for b in range(B)], [], None, 0, False, False),
        ("natural-eos", begin + 3, 3, -1, -1, None, list(range(1, B)), 0, 0, False, False),   # the last live row ends: done
        ("eos-one-row", begin + 3, 3, -1, -1, None, [], B - 1, 0, False, True),
        ("max-length", max_length - 1, 7, -1, -1, None, [], None, 0, False, False),
        ("done", begin + 3, 3, forced_tok, 3, None, [], None, 1, False, False),
        ("all-masked", begin, 0, -1, -1, None, [], None, 0, True, False),
    ]
    for name, cur, step, ftok, fstep, frows, fin, eos_row, done, full, half in scenes:
        mask = torch.ones(V, dtype=torch.uint8) if full else mask0
        tok_emb, te_d = tables[half]
        forced = np.full(max_length, -1, dtype=np.int32)
        forced[cur] = ftok
        got_ids = {}
        for src, n_parts in sources:
            per = per8 if src == "chunks" else -(-V // n_parts)
            n = 8 if src == "chunks" else n_parts
            lg = _crafted_logits(B, V, borders, eos, nan_masked, eos_row)
            ids = torch.full((MAX_ROWS, max_length), -3, dtype=torch.int32)
            ids[:, :cur] = 1
            unf = torch.ones(MAX_ROWS, dtype=torch.int32)
            unf[fin] = 0
            st = _state(B, cur, cur - 1, cur - 1, step, done=done)
            next_x = torch.full((MAX_ROWS, d), 123.25)
            want = _reference_step(lg, mask, forced, ids, unf, st, fstep, frows, tok_emb, pos_emb, next_x, B, max_length, begin, eos, pad)
            at_begin = torch.full((B,), cur == begin)
            ids_d, unf_d, nx_d, mask_d = ids.cuda(), unf.cuda(), next_x.cuda(), mask.cuda()
            lg_d = pv_d = pi_d = None
            if src == "chunks":
                lg_d = lg.cuda()
            else:   # what the vocabulary GEMV leaves: masked partials over consecutive id ranges
                pv, pi = _partials(_masked(lg, mask, at_begin), per, n)
                pv_d, pi_d = pv.float().cuda(), pi.to(torch.int32).cuda()
            _, fp = _i32(forced)
            rows_io, rp = _i32(frows) if frows is not None else (None, None)
            st_io, sp = _i32(st)
            rc = lib.wt_dbg_greedy_select(P(lg_d), P(pv_d), P(pi_d), n, P(mask_d), fp, P(ids_d), P(unf_d), sp, fstep, rp, P(te_d), P(pe_d), pos_rows,
                                          int(half), P(nx_d), B, V, d, max_length, begin, eos, pad, P(sc), _stream())
            assert rc == 0, (name, src, n)
            torch.cuda.synchronize()
            what = (name, src, n)
            assert torch.equal(ids_d.cpu(), want[0]), what
            assert torch.equal(unf_d.cpu(), want[1]), what
            assert st_io.tolist() == want[2].tolist(), what
            assert torch.equal(_bits(nx_d.cpu()), _bits(want[3])), what
            got_ids[(src, n)] = ids_d.cpu()
            # what the scene is there to show
            new = want[0][:B, cur].tolist()
            if name == "done":
                assert want[0][:B, cur].tolist() == [-3] * B and st_io[3] == 6 and st_io[0] == 1
            elif name == "max-length":
                assert st_io[0] == 1 and bool((nx_d.cpu() == 123.25).all())
            elif name == "natural-eos":
                assert new[0] == eos and st_io[0] == 1 and st_io[1] == 0
            elif name == "eos-one-row":
                assert new[B - 1] == eos
                if V > 5:   # (V = 5: other roles' maxima fall on EOS too)
                    assert st_io[1] == B - 1 and st_io[0] == (1 if B == 1 else 0)
            elif name == "forced+eos-step":
                assert new == [pad if b in fin else eos for b in range(B)] and st_io[0] == 1
            elif name == "forced+eos-rows":
                assert new == [eos if frows[b] == step else forced_tok for b in range(B)]
            elif name == "forced":
                assert new == [pad if b in fin else forced_tok for b in range(B)]
            elif name == "all-masked":
                assert new == [0] * B
            elif name in ("at-begin", "later"):
                for b in range(B if V > 5 else 0):   # (V = 5: the roles' ids collide; the reference above still holds)
                    role = b % 6
                    exp = {0: borders[0] - 1 if borders else V - 1, 1: V - 1, 2: V - 2, 3: 0, 4: V // 2 if cur == begin else 2}.get(role)
                    if b in fin:
                        exp = pad
                    if exp is not None:
                        assert new[b] == exp, (what, b)
        first = got_ids[("chunks", 8)]
        assert all(torch.equal(first, v) for v in got_ids.values()), name


# ---- dec_embed_kernel ----
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("d", [384, 1024])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_dec_embed(lib, B, d, half):
    V, pos_rows, ld = 301, 24, 10
    gen = torch.Generator().manual_seed(d + B)
    tok_emb = torch.randn(V, d, generator=gen)
    tok_emb = tok_emb.half() if half else tok_emb
    pos_emb = torch.randn(pos_rows, d, generator=gen)
    ids = torch.randint(0, V, (B, ld), generator=gen).to(torch.int32)
    ids[0, 0], ids[B - 1, ld - 1] = V - 1, 0
    cur_len = np.array([1 + (3 * b) % ld for b in range(B)], dtype=np.int32)   # rows at different lengths and positions
    cur_len[B - 1] = ld
    pos = np.array([(5 * b + 2) % pos_rows for b in range(B)], dtype=np.int32)
    pos[0] = pos_rows - 1
    x = torch.full((MAX_ROWS, d), 123.25, device="cuda")
    sc = _scratch(lib.wt_dbg_dec_embed_scratch_bytes(B, ld))
    te_d, pe_d = tok_emb.cuda(), pos_emb.cuda()
    rc = lib.wt_dbg_dec_embed(_i32(ids.numpy())[1], ld, _i32(cur_len)[1], _i32(pos)[1], P(te_d), V, P(pe_d), pos_rows, half, P(x), B, d, P(sc), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    toks = [int(ids[b, cur_len[b] - 1]) for b in range(B)]
    want = torch.full((MAX_ROWS, d), 123.25)
    want[:B] = tok_emb[toks].float() + pos_emb[pos.tolist()]   # one fp32 add of the widened table row
    assert torch.equal(_bits(x.cpu()), _bits(want))


# ---- the fused and the unfused tail on the same inputs ----
@pytest.mark.parametrize("w_half", [0, 1])
@pytest.mark.parametrize("K", [384, 1024])
@pytest.mark.parametrize("B", [3, 8, 16])
def test_fused_tail_equals_unfused_tail(lib, B, K, w_half):
    N, begin, max_length, pos_rows = 51864, 4, 12, 16
    X, g, be, W, mask, _ = _random_vocab_case(K, B, N, w_half, 3)
    eos, pad = N - 3, N - 4
    gen = torch.Generator().manual_seed(K + B)
    tok_emb = W if w_half else torch.randn(N, K, generator=gen)   # fp16 engines: the tied table
    pos_emb = torch.randn(pos_rows, K, generator=gen)
    dev = [t.cuda() for t in (X, g, be, W, mask)]
    te_d, pe_d = tok_emb.cuda(), pos_emb.cuda()
    sc = _scratch(lib.wt_dbg_greedy_select_scratch_bytes(max_length))
    forced = np.full(max_length, -1, dtype=np.int32)
    for cur in (begin, begin + 1):   # with and without the begin mask
        cur_len = np.full(B, cur, dtype=np.int32)
        pv, pi, trace = _run_vocab(lib, dev[0], dev[1], dev[2], dev[3], None, dev[4], cur_len, begin, 1, 1)
        _, _, logits = _run_vocab(lib, dev[0], dev[1], dev[2], dev[3], None, dev[4], cur_len, begin, 1, 1, fused=0)
        assert torch.equal(_bits(trace), _bits(logits))
        out = []
        for fused in (1, 0):
            ids = torch.full((MAX_ROWS, max_length), -3, dtype=torch.int32, device="cuda")
            unf = torch.ones(MAX_ROWS, dtype=torch.int32, device="cuda")
            nx = torch.full((MAX_ROWS, K), 123.25, device="cuda")
            st, sp = _i32(_state(B, cur, cur - 1, cur - 1, cur - begin))
            lg_d = None if fused else logits.cuda()
            pv_d, pi_d = (pv.cuda(), pi.cuda()) if fused else (None, None)
            rc = lib.wt_dbg_greedy_select(P(lg_d), P(pv_d), P(pi_d), pv.shape[1] if fused else 8, P(dev[4]), _i32(forced)[1], P(ids), P(unf), sp, -1,
                                          None, P(te_d), P(pe_d), pos_rows, w_half, P(nx), B, N, K, max_length, begin, eos, pad, P(sc), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            out.append((ids.cpu(), unf.cpu(), st.tolist(), _bits(nx.cpu())))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] and torch.equal(out[0][3], out[1][3])
        at_begin = torch.full((B,), cur == begin)
        assert out[0][0][:B, cur].tolist() == _argmax_rows(_masked(logits, mask, at_begin))[1].tolist()
