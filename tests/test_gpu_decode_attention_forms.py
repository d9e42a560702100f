"""dec_attn_kernel in the forms the decode step really launches (engine.hip, enqueue_layer_part), per element against fp64.

The other kernel-level tests reach the kernel with fixed_len = len and nt = 1.  Here, through wt_dbg_decode_attention_state and
wt_dbg_self_attention_then_pair_state: the length per row from a device DecState (one launch mixes a row of 1 key with one of 448), the
skip-finished-rows forms (alive), default-policy loads (nt = 0), idle slots (slot_row = -1), the two-split deferred merge with per-row
lengths, and score ranges that punish a wrong online softmax (wide, a common offset of +-100, a late jump of the running maximum, flat).

Reference: torch softmax attention in fp64, per row over that row's own first len_b keys (half caches: rounded to half, then widened).
Bounds: the existing ones for N(0, 1) inputs (2e-5 fp32 caches, 3e-5 half caches / folded query / the pair's GEMV outputs).  Adversarial
inputs: max(2e-5, 8 x |att_fp32_cpu - att_fp64|_inf), att_fp32_cpu the same torch attention in float32 on the host -- a margin of 8 over
the float32 reference's own error for the kernel's other summation order (16 / 32 interleaved streams, then splits) and the hardware exp.
Every test prints err / bound (-s).

Measured on an MI355X: the largest err / bound of the adversarial cases is 0.21 (err 7.3e-6 at the widest scores, bound 7.0e-5 there,
the hooks and load policies agreeing to the printed digits); on N(0, 1) inputs the largest error of any per-row / alive / slot_row case is
2.5e-6 against the 2e-5 bound, of the pair's h1 / u 9.8e-7 against 3e-5.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000   # torch.full(..., nan) in float32
LENS = [1, 2, 16, 17, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 447, 448]
CAP = 448


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


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _dev_i32(vals):
    return None if vals is None else torch.tensor(vals, dtype=torch.int32, device="cuda")


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def _attention(q, k, v, lens, rows=None):
    """Plain softmax attention in the dtype of the operands: row b of q [B][H*64] over the first lens[b] keys of cache row rows[b]
    (default b) of k / v [R][H][cap][64] -> [B][H*64]."""
    B, H = q.shape[0], k.shape[1]
    out = []
    for b in range(B):
        r = b if rows is None else rows[b]
        qb = q[b].view(H, 1, 64)
        att = torch.softmax(qb @ k[r, :, :lens[b]].transpose(-1, -2), -1)
        out.append((att @ v[r, :, :lens[b]]).reshape(H * 64))
    return torch.stack(out)


def _fold(u, h1, r, t):
    mu = h1.mean(1, keepdim=True)
    rstd = (h1.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    return (u - mu * r) * rstd + t


def _launch_state(lib, q, k, v, *, lens=None, fixed_len=0, alive=None, slot=None, rows=None, ln=None, n_split=1, nt=1, defer=0, launches=1):
    """wt_dbg_decode_attention_state on NaN-sentinel outputs; k / v float or half host tensors [R][H][cap][64].  Returns (out, part, cnt)."""
    B, H, cap = q.shape[0], k.shape[1], k.shape[2]
    kv_half = int(k.dtype == torch.float16)
    out, part = _nan(B, H * 64), _nan(B, H, n_split, 68)
    cnt = torch.zeros(B, H, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(int(lib.wt_dbg_decode_attention_state_scratch_bytes()), dtype=torch.uint8, device="cuda")
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    ad, sd = _dev_i32(alive), _dev_i32(slot)
    lnd = [x.cuda() for x in ln] if ln else [None, None, None]
    sl = _i32([n - 1 for n in lens]) if lens is not None else None
    for _ in range(launches):   # the arrival tickets must re-arm themselves between launches
        rc = lib.wt_dbg_decode_attention_state(P(qd), P(kd), P(vd), P(part), P(cnt), P(out), sl, fixed_len, P(ad), P(sd),
                                               k.shape[0] if rows is None else rows, P(lnd[0]), P(lnd[1]), P(lnd[2]), B, H, cap, n_split,
                                               kv_half, nt, defer, P(scratch), _stream())
        assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu(), part.cpu(), cnt.cpu()


@functools.lru_cache(maxsize=None)
def _core_inputs(kv_half):
    """q [16][128], k / v [16][2][448][64] (half caches: rounded) and their fp64 widening; shared and never modified."""
    q = _rand(16, 128, seed=15) * 0.5
    k, v = _rand(16, 2, CAP, 64, seed=16), _rand(16, 2, CAP, 64, seed=17)
    if kv_half:
        k, v = k.half(), v.half()
    return q, k, v, q.double(), k.double(), v.double()


@functools.lru_cache(maxsize=None)
def _core_ref(kv_half, lens):
    _, _, _, q64, k64, v64 = _core_inputs(kv_half)
    return _attention(q64[:len(lens)], k64, v64, list(lens))


def _bound(kv_half):
    return 3e-5 if kv_half else 2e-5


# ------------------------------------------------------------------------------------------------------------- per-row lengths
SUBSETS = {1: (129,), 3: (448, 1, 128), 5: (2, 257, 33, 127, 447), 8: (1, 448, 17, 128, 256, 65, 2, 129)}


@pytest.mark.parametrize("nan_tail", [False, True])
@pytest.mark.parametrize("n_split", [1, 2, 4])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kv_half", [0, 1])
@pytest.mark.parametrize("lens", [tuple(LENS), tuple(reversed(LENS))] + list(SUBSETS.values()), ids=lambda l: f"B{len(l)}first{l[0]}")
def test_self_attention_length_per_row_from_device_state(lib, lens, kv_half, nt, n_split, nan_tail):
    """LP_SELF_ATTN: len = st->self_len[b] + 1 per block.  One grid holds rows with fewer keys than streams, one key per stream, both
    sides of the 128-key switch of the eight-wave form, the cache's last row, and (four splits, 1 or 2 keys) empty splits.  With
    nan_tail every key past a row's length is NaN: the clamped loads of a correct kernel never read one."""
    q, k, v, _, _, _ = _core_inputs(kv_half)
    B = len(lens)
    ref = _core_ref(kv_half, lens)
    if nan_tail:
        k, v = k.clone(), v.clone()
        for b, n in enumerate(lens):
            k[b, :, n:] = float("nan")
            v[b, :, n:] = float("nan")
    out, _, cnt = _launch_state(lib, q[:B], k[:B], v[:B], lens=list(lens), n_split=n_split, nt=nt, launches=3)
    assert int(cnt.abs().sum()) == 0
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs().max(1).values
    print(f"\nlens {lens[0]}..{lens[-1]} half {kv_half} nt {nt} splits {n_split}: err {err.max().item():.2e} bound {_bound(kv_half):.0e}")
    assert err.max().item() < _bound(kv_half), [(n, f"{e:.2e}") for n, e in zip(lens, err.tolist())]


# ------------------------------------------------------------------------------------------------------------- skip-finished rows
ALIVE = {"all": [1] * 16, "alternating": [1, 0] * 8, "first": [1] + [0] * 15, "last": [0] * 15 + [1]}
PERM = [5, 0, 11, 3, 15, 8, 1, 13, 2, 10, 7, 14, 4, 9, 12, 6]   # cache row of slot b


@pytest.mark.parametrize("n_split", [1, 2])
@pytest.mark.parametrize("with_slot", [False, True])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kv_half", [0, 1])
@pytest.mark.parametrize("pattern", list(ALIVE))
def test_finished_rows_are_skipped_and_live_rows_unaffected(lib, pattern, kv_half, nt, with_slot, n_split):
    """The ALIVE forms (nt = 1): a row with alive[b] == 0 leaves after the query prologue -- out, part and the tickets stay as they were
    -- and the live rows beside it are exact.  nt = 0 has no such form: the plain kernel runs, a dead row is untouched or attended."""
    q, k, v, q64, k64, v64 = _core_inputs(kv_half)
    alive, lens = ALIVE[pattern], LENS
    slot = PERM if with_slot else None
    ref = _attention(q64, k64, v64, lens, slot) if with_slot else _core_ref(kv_half, tuple(lens))
    out, part, cnt = _launch_state(lib, q, k, v, lens=lens, alive=alive, slot=slot, n_split=n_split, nt=nt, launches=3)
    assert int(cnt.abs().sum()) == 0
    err = (out.double() - ref).abs().max(1).values
    bound = _bound(kv_half)
    live_err = max(err[b].item() for b in range(16) if alive[b])
    print(f"\nalive {pattern} half {kv_half} nt {nt} slot {with_slot} splits {n_split}: live err {live_err:.2e} bound {bound:.0e}")
    for b in range(16):
        if alive[b]:
            assert torch.isfinite(out[b]).all() and err[b].item() < bound, (b, err[b].item())
        elif nt == 1:
            assert _untouched(out[b]) and _untouched(part[b]), b
        else:
            assert _untouched(out[b]) or err[b].item() < bound, (b, err[b].item())


# ------------------------------------------------------------------------------------------------------------- cross attention, slot_row
SLOTS = [3, -1, 0, 3, -1, 4, 1, 0]   # 8 slots over a pool of 5 cache rows: repeats, two idle slots


@pytest.mark.parametrize("dead", [False, True])
@pytest.mark.parametrize("n_split", [1, 2])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kv_half", [0, 1])
@pytest.mark.parametrize("H", [2, 6])
def test_cross_attention_through_slot_rows_with_idle_slots(lib, H, kv_half, nt, n_split, dead):
    """LP_CROSS_ATTN of the continuous mode: folded query, every slot over the 160 keys of pool row slot_row[b]; an idle slot (-1) reads
    row 0 (DecAttnParams.slot_row).  dead: the idle slots and one mapped slot are finished rows."""
    B, S, pool, d = 8, 160, 5, 64 * H
    u, h1 = _rand(B, d, seed=21) * 0.5, _rand(B, d, seed=22) * 2.0 + 0.7
    r, t = _rand(d, seed=23), _rand(d, seed=24) * 0.3
    k, v = _rand(pool, H, S, 64, seed=25), _rand(pool, H, S, 64, seed=26)
    if kv_half:
        k, v = k.half(), v.half()
    alive = [1, 0, 1, 1, 0, 1, 0, 1] if dead else None
    out, part, cnt = _launch_state(lib, u, k, v, fixed_len=S, alive=alive, slot=SLOTS, rows=pool, ln=(h1, r, t), n_split=n_split, nt=nt, launches=3)
    assert int(cnt.abs().sum()) == 0
    q64 = _fold(u.double(), h1.double(), r.double(), t.double())
    ref = _attention(q64, k.double(), v.double(), [S] * B, [max(s, 0) for s in SLOTS])
    err = (out.double() - ref).abs().max(1).values
    bound = 3e-5
    print(f"\nH {H} half {kv_half} nt {nt} splits {n_split} dead {dead}: err {err[torch.isfinite(err)].max().item():.2e} bound {bound:.0e}")
    for b in range(B):
        if alive is None or alive[b]:
            assert torch.isfinite(out[b]).all() and err[b].item() < bound, (b, SLOTS[b], err[b].item())
        elif nt == 1:
            assert _untouched(out[b]) and _untouched(part[b]), b
        else:
            assert _untouched(out[b]) or err[b].item() < bound, (b, err[b].item())


# ------------------------------------------------------------------------------------------------------------- two splits into the pair
PAIR_LENS = [1, 2, 3, 33, 128, 257, 447, 448]


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("half", [0, 1])
def test_two_split_self_attention_into_the_pair_with_per_row_lengths(lib, half, nt):
    """LP_SELF_ATTN with two splits and the merge deferred, then LP_PAIR: split 1 of a short row is empty (m = -inf, l = 0, o = 0) in the
    launch where a long row's split 1 holds 224 keys.  h1 and u against fp64, and bitwise against each row run alone at its own length.
    At batch 8, and at batch 9: the smallest batch of the 16-row shape, whose pair kernel (half-staged second GEMV) needs more than 48 KiB
    of dynamic LDS."""
    for lens in (PAIR_LENS, PAIR_LENS + [200]):
        _two_split_pair_per_row_lengths(lib, half, nt, lens)


def _two_split_pair_per_row_lengths(lib, half, nt, lens):
    B, H = len(lens), 6
    d = 64 * H
    q = _rand(B, d, seed=51) * 0.5
    k, v = _rand(B, H, CAP, 64, seed=52), _rand(B, H, CAP, 64, seed=53)
    Wo, bo = _rand(d, d, seed=54, scale=d ** -0.5), _rand(d, seed=55)
    Wf, c = _rand(d, 2 * d, seed=56, scale=(2 * d) ** -0.5), _rand(d, seed=57)
    h = _rand(B, d, seed=58)
    if half:
        k, v, Wo, Wf = k.half(), v.half(), Wo.half(), Wf.half()
    qd, kd, vd, Wod, bod, Wfd, cd, hd = (x.cuda() for x in (q, k, v, Wo, bo, Wf, c, h))
    scratch = torch.zeros(int(lib.wt_dbg_self_attention_then_pair_state_scratch_bytes()), dtype=torch.uint8, device="cuda")
    part, h1, u = _nan(B, H, 2, 68), _nan(B, d), _nan(B, d)
    assert lib.wt_dbg_self_attention_then_pair_state(P(qd), P(kd), P(vd), P(part), P(Wod), P(bod), P(hd), P(h1), P(Wfd), P(cd), P(u),
                                                     _i32([n - 1 for n in lens]), 0, B, H, CAP, half, nt, P(scratch), _stream()) == 0
    # every row alone, at its own fixed length (fp32: the fixed-length hook the other tests use, nt = 1 -- the load policy does not change
    # the arithmetic there; half caches: the same nt, which selects the pipelined form with its own order of operations)
    h1_1, u_1 = _nan(B, d), _nan(B, d)
    for b, n in enumerate(lens):
        part1 = _nan(1, H, 2, 68)
        if half:
            rc = lib.wt_dbg_self_attention_then_pair_state(P(qd[b]), P(kd[b]), P(vd[b]), P(part1), P(Wod), P(bod), P(hd[b]), P(h1_1[b]), P(Wfd), P(cd),
                                                           P(u_1[b]), None, n, 1, H, CAP, 1, nt, None, _stream())
        else:
            rc = lib.wt_dbg_self_attention_then_pair(P(qd[b]), P(kd[b]), P(vd[b]), P(part1), P(Wod), P(bod), P(hd[b]), P(h1_1[b]), P(Wfd), P(cd),
                                                     P(u_1[b]), 1, H, CAP, n, _stream())
        assert rc == 0
    torch.cuda.synchronize()
    a = _attention(q.double(), k.double(), v.double(), lens)
    ref1 = h.double() + a @ Wo.double().T + bo.double()
    ref2 = torch.cat([a, h.double()], 1) @ Wf.double().T + c.double()
    assert torch.isfinite(h1).all() and torch.isfinite(u).all()
    e1, e2 = (h1.cpu().double() - ref1).abs().max().item(), (u.cpu().double() - ref2).abs().max().item()
    print(f"\nB {B} half {half} nt {nt}: h1 err {e1:.2e} u err {e2:.2e} bound 3e-05")
    assert e1 < 3e-5 and e2 < 3e-5
    assert torch.equal(h1.cpu(), h1_1.cpu()) and torch.equal(u.cpu(), u_1.cpu())
    assert torch.equal(hd.cpu(), h)   # the residual input is read-only


# ------------------------------------------------------------------------------------------------------------- refusals
def test_state_hooks_refuse_what_they_cannot_launch(lib):
    B, H, cap = 4, 2, 16
    d = 64 * H
    q, k, v = torch.zeros(16, d, device="cuda"), torch.zeros(16, H, cap, 64, device="cuda"), torch.zeros(16, H, cap, 64, device="cuda")
    out, part = _nan(16, d), _nan(16, H, 2, 68)
    cnt = torch.zeros(16, H, dtype=torch.int32, device="cuda")
    ln = torch.ones(16, d, device="cuda")
    scratch = torch.zeros(int(lib.wt_dbg_decode_attention_state_scratch_bytes()), dtype=torch.uint8, device="cuda")

    def call(self_len=(3, 3, 3, 3), fixed_len=0, slot=None, rows=16, lns=(None, None, None), B=B, n_split=2, nt=1, kv_half=0):
        sd = _dev_i32(slot)
        return lib.wt_dbg_decode_attention_state(P(q), P(k), P(v), P(part), P(cnt), P(out), _i32(list(self_len)) if self_len is not None else None,
                                                 fixed_len, None, P(sd), rows, P(lns[0]), P(lns[1]), P(lns[2]), B, H, cap, n_split, kv_half, nt,
                                                 0, P(scratch), _stream())

    assert call() == 0   # the arguments the refusals below vary are launchable as they stand
    assert call(self_len=None, fixed_len=cap, slot=[0, -1, 3, 2], rows=4, lns=(ln, ln, ln)) == 0
    assert call(self_len=(3, -1, 3, 3)) == -22
    assert call(self_len=(3, 3, 3, cap)) == -22
    assert call(self_len=(3,) * 17, B=17) == -22
    assert call(lns=(ln, None, None)) == -22
    assert call(lns=(ln, ln, None)) == -22
    assert call(lns=(None, ln, ln)) == -22
    assert call(slot=[0, 1, 2, 4], rows=4) == -22
    assert call(slot=[0, -2, 2, 3], rows=4) == -22
    assert call(self_len=None, fixed_len=0) == -22          # no length at all
    assert call(fixed_len=cap) == -22                       # two lengths
    assert call(self_len=None, fixed_len=cap + 1) == -22
    assert call(n_split=0) == -22 and call(n_split=17) == -22
    assert call(nt=2) == -22
    torch.cuda.synchronize()
    assert _untouched(out[B:]) and _untouched(part[B:])   # the two accepted calls wrote rows < B; no refused call launched anything wider
    sl = _i32([3, 3, 3, cap])
    W, Wf = _nan(d, d), _nan(d, 2 * d)
    assert lib.wt_dbg_self_attention_then_pair_state(P(q), P(k), P(v), P(part), P(W), P(ln), P(ln), P(out), P(Wf), P(ln), P(out), sl, 0, B, H, cap,
                                                     0, 1, P(scratch), _stream()) == -22
    assert lib.wt_dbg_self_attention_then_pair_state(P(q), P(k), P(v), P(part), P(W), P(ln), P(ln), P(out), P(Wf), P(ln), P(out), None, 0, B, H, cap,
                                                     0, 1, P(scratch), _stream()) == -22
    assert lib.wt_dbg_self_attention_then_pair_state(P(q), P(k), P(v), P(part), P(W), P(ln), P(ln), P(out), P(Wf), P(ln), P(out), _i32([3] * 17), 0,
                                                     17, H, cap, 0, 1, P(scratch), _stream()) == -22


# ------------------------------------------------------------------------------------------------------------- adversarial score ranges
def _adversarial(kind, length, n_split, kv_half):
    B, H = 3, 2
    q = _rand(B, H * 64, seed=61) * 0.5
    k, v = _rand(B, H, CAP, 64, seed=62), _rand(B, H, CAP, 64, seed=63)
    qh = q.view(B, H, 1, 64)
    qn = qh.norm(dim=-1, keepdim=True)
    if kind == "wide":          # scores within about +-74, the softmax near one-hot
        q = q * 5.0
    elif kind == "wider":       # q = 5 N(0, 1): scores within about +-143
        q = q * 10.0
    elif kind in ("offset+100", "offset-100"):
        k = k + float(kind[6:]) * qh / qn ** 2        # every score of the head moves by c
    elif kind == "late-jump":
        chunk = (length + n_split - 1) // n_split
        keys = {length - 1, (chunk + length) // 2 if n_split > 1 else length // 2}
        if n_split > 1:
            keys.add(chunk)                            # the first key of split 1; split 0 holds none of them
        for s in keys:
            k[:, :, s] = (6.0 * qh / qn)[:, :, 0]
    elif kind == "flat":
        k = k[:, :, :1].expand_as(k).clone()
    else:
        raise AssertionError(kind)
    if kv_half:
        k, v = k.half(), v.half()
    return q.contiguous(), k.contiguous(), v.contiguous()


@pytest.mark.parametrize("kv_half", [0, 1])
@pytest.mark.parametrize("n_split", [1, 2, 3])
@pytest.mark.parametrize("length", [447, 129])
@pytest.mark.parametrize("kind", ["wide", "wider", "offset+100", "offset-100", "late-jump", "flat"])
def test_online_softmax_on_adversarial_score_ranges(lib, kind, length, n_split, kv_half):
    """Stream merge through LDS, split merge by ticket or by the consumer GEMV, the branch-free consume of the pipelined form and __expf,
    on scores N(0, 1) inputs never produce.  Through the fixed-length hooks (nt = 1), the state hook (per-row length, nt = 0 and 1) and,
    at two splits, the deferred merge inside a GEMV with W = I (y = the merged context, exactly)."""
    q, k, v = _adversarial(kind, length, n_split, kv_half)
    B, H, d = q.shape[0], 2, 128
    lens = [length] * B
    ref = _attention(q.double(), k.double(), v.double(), lens)
    ref32 = _attention(q, k.float(), v.float(), lens)
    bound = max(2e-5, 8.0 * (ref32.double() - ref).abs().max().item())
    if kind == "flat":   # uniform weights: the mean of the values
        assert (ref - v.double()[:, :, :length].mean(2).reshape(B, d)).abs().max().item() < 1e-12
    got = {}
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    part, out = _nan(B, H, n_split, 68), _nan(B, d)
    cnt = torch.zeros(B, H, dtype=torch.int32, device="cuda")
    if kv_half:
        rc = lib.wt_dbg_decode_attention_f16(P(qd), P(kd), P(vd), P(part), P(cnt), P(out), None, None, None, B, H, CAP, length, n_split, _stream())
    else:
        rc = lib.wt_dbg_decode_attention(P(qd), P(kd), P(vd), P(part), P(cnt), P(out), B, H, CAP, length, n_split, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0
    got["fixed"] = out.cpu()
    for nt in (0, 1):
        got[f"state nt{nt}"], _, c2 = _launch_state(lib, q, k, v, lens=lens, n_split=n_split, nt=nt, launches=2)
        assert int(c2.abs().sum()) == 0
    if n_split == 2:
        eye = torch.eye(d, dtype=torch.float16 if kv_half else torch.float32, device="cuda")
        zero, zrow = torch.zeros(d, device="cuda"), torch.zeros(B, d, device="cuda")
        part2, y = _nan(B, H, 2, 68), _nan(B, d)
        if kv_half:
            rc = lib.wt_dbg_attention_then_projection_f16(P(qd), P(kd), P(vd), P(part2), P(eye), P(zero), P(zrow), P(y), B, H, CAP, length, _stream())
        else:
            rc = lib.wt_dbg_attention_then_projection(P(qd), P(kd), P(vd), P(part2), P(eye), P(zero), P(zrow), P(y), B, H, CAP, length, 2, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        got["deferred"] = y.cpu()
    errs = {name: (o.double() - ref).abs().max().item() if torch.isfinite(o).all() else float("inf") for name, o in got.items()}
    worst = max(errs.values())
    print(f"\n{kind} len {length} splits {n_split} half {kv_half}: bound {bound:.2e} ratio {worst / bound:.3f} " +
          " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for name, e in errs.items():
        assert e < bound, (name, e, bound)
