"""Decode self-attention as the step graph launches it (length per row from a device DecState; hook wt_dbg_decode_attention_state) over
caches whose rows at or beyond a row's length hold NaN bit patterns: nothing of such a tail may reach the result (a score of -inf alone
would not do: 0 x NaN is NaN).  Lengths around every path of dec_attn_kernel -- fewer keys than streams, the 16 / 32-stream switch at
128 keys, a full cache -- mixed within a batch; both load policies; the skip-finished-rows (ALIVE) form with finished rows.
Against float64 within 2e-5, the bound of tests/test_gpu_decode_attention_forms.py for fp32 caches.  Any form of the kernel that
requests keys before it knows the length (DESIGN.md section 9.1 (2) records one that was measured and retired) has to keep this.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, CAP = 2, 448
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 447, 448)
BATCHES = {"a": (1, 128, 2, 447, 15, 129, 16, 448), "b": (17, 127, 31, 128, 32, 33, 448, 129)}
# (name, keys per row, nt, alive flags or None)
CASES = [(f"b1_len{n}_nt{nt}", (n,), nt, None) for n in LENGTHS for nt in (0, 1)]
CASES += [(f"b8_{k}_nt{nt}", v, nt, None) for k, v in BATCHES.items() for nt in (0, 1)]
CASES += [(f"b8_{k}_alive", v, 1, (1, 1, 0, 1, 1, 1, 1, 0)) for k, v in BATCHES.items()]
PREFILL = 0.25   # what `out` holds before the launch: a finished row keeps it


@pytest.fixture(scope="module")
def lib():
    import whisper_trtllm_amd as w
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    return w._lib.load()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(B):
    """q and NaN-free caches (CPU, float32); the same for every case of a batch width"""
    gen = torch.Generator().manual_seed(4100 + B)
    q = torch.randn(B, H * 64, generator=gen) * 0.5
    k, v = torch.randn(B, H, CAP, 64, generator=gen), torch.randn(B, H, CAP, 64, generator=gen)
    return q, k, v


@pytest.mark.parametrize("name,lens,nt,alive", CASES, ids=[c[0] for c in CASES])
def test_nan_tails_never_reach_the_result(lib, name, lens, nt, alive):
    B = len(lens)
    q, k, v = _inputs(B)
    kn, vn = k.clone(), v.clone()
    for b, n in enumerate(lens):   # rows at or beyond the length: NaN bit patterns (quiet, both signs)
        kn[b, :, n:] = float("nan")
        vn[b, :, n:] = -torch.tensor(float("nan"))
    qd, kd, vd = q.cuda(), kn.cuda(), vn.cuda()
    out = torch.full((B, H * 64), PREFILL, device="cuda")
    scratch = torch.zeros(lib.wt_dbg_decode_attention_state_scratch_bytes(), dtype=torch.uint8, device="cuda")
    sl = np.ascontiguousarray(np.array(lens, dtype=np.int32) - 1)
    al = torch.tensor(alive, dtype=torch.int32, device="cuda") if alive else None
    rc = lib.wt_dbg_decode_attention_state(P(qd), P(kd), P(vd), None, None, P(out), sl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0, P(al), None,
                                           B, None, None, None, B, H, CAP, 1, 0, nt, 0, P(scratch),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    qh = q.double().view(B, H, 1, 64)
    ref = torch.empty(B, H * 64, dtype=torch.float64)
    for b, n in enumerate(lens):
        att = torch.softmax(qh[b] @ k[b, :, :n].double().transpose(-1, -2), -1)
        ref[b] = (att @ v[b, :, :n].double()).reshape(H * 64)
        if alive and not alive[b]:
            ref[b] = PREFILL   # a finished row streams nothing and keeps what the buffer held
    err = (got - ref).abs().max().item()
    print(f"{name}: max err {err:.3e}")
    assert err < 2e-5, err
