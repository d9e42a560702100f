"""Host side of temperature sampling: the reference sampler (tests/sampling_ref.py) against the Philox known answers and against
softmax(s / T), the whole-decode reference against the reference-recorded goldens, the header / binding / exports, the fallback loop
against a scripted engine, and the Python refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

import sampling_ref as ref
import whisper_trtllm_amd  # noqa: F401
from conftest import load_case
from whisper_trtllm_amd import _lib, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SM_CASES = ["sm-tiny_b2", "sm-toy-short_b3", "sm-ts-toy_b3"]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        out = ref.philox4x32_10([np.array([c]) for c in counter], key)
        assert " ".join(f"{int(x[0]):08x}" for x in out) == want


def test_uniform_is_strictly_inside_the_unit_interval():
    """u = ((x >> 9) + 0.5) 2^-23 in fp32 arithmetic: 23 bits, because (x >> 8) + 0.5 needs 25 significand bits from x = 2^31 on and
    would round to 2^24 -- u = 1, g = +inf -- at x = 0xffffffff."""
    u = ref.uniform_of(np.array([0, 0xff, 0xffffffff], dtype=np.uint32))
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    assert u[0] == np.float32(2.0 ** -24) and u[2] == np.float32(1.0 - 2.0 ** -24)
    assert np.isfinite(-np.log(-np.log(u))).all()


def _chi2_quantile(p, k):
    """Wilson-Hilferty: the p-quantile of chi-square with k degrees of freedom (z = the normal quantile, by bisection on erf)."""
    lo, hi = 0.0, 10.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if 0.5 * (1 + math.erf(mid / math.sqrt(2))) < p else (lo, mid)
    return k * (1 - 2 / (9 * k) + lo * math.sqrt(2 / (9 * k))) ** 3


def test_reference_sampler_draws_from_softmax():
    V, T, N = 50, 0.7, 20000
    s = np.random.default_rng(0).standard_normal(V) * 3
    p = np.exp(s / T - (s / T).max())
    p /= p.sum()
    count = np.zeros(V)
    for t in range(N):
        count[ref.nan_argmax(ref.keys(s, T, 1234, t))] += 1
    e = p * N
    small = e < 5                                   # cells with expectation below 5 are pooled into one
    obs, exp = np.append(count[~small], count[small].sum()), np.append(e[~small], e[small].sum())
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    bound = _chi2_quantile(0.999, len(exp) - 1)
    print(f"chi-square {chi2:.1f} on {len(exp)} cells, 0.999 quantile {bound:.1f}")
    assert chi2 <= bound


@pytest.mark.parametrize("case", SM_CASES)
def test_decode_reference_matches_golden(case):
    """The CPU whole-decode reference (cpu_ref's decoder + the fp32 key) reproduces the goldens the reference's own loop recorded: ids
    equal, log-probabilities within 2e-3 through each row's EOS (tests/test_logprobs_host.py's bound)."""
    z, cfg, weights, mel = load_case(case)
    ids, lp = ref.sample_decode(cfg, weights, mel, float(z["temperature"]), [int(s) for s in z["sampler_seeds"]],
                                timestamp_mode=bool(int(z["timestamp_mode"])))
    np.testing.assert_array_equal(ids, z["ids"])
    eos = cfg["eos_token_id"]
    want = z["token_logprobs"]
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, 1:] == eos)[0]
        last = int(hit[0]) + 1 if hit.size else ids.shape[1] - 1
        assert np.abs(lp[b, 1:last + 1] - want[b, :last]).max() <= 2e-3
    live = np.ones(z["top2_margin"].shape, dtype=bool)
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, 1:] == eos)[0]
        if hit.size:
            live[b, hit[0] + 1:] = False
    assert z["top2_margin"][live].min() >= 1e-3


def test_goldens_differ_from_the_greedy_ones():
    for case in SM_CASES:
        z = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
        g = np.load(os.path.join(ROOT, "tests", "golden", "lp-" + case[3:] + ".npz"))["ids"]
        n = min(z["ids"].shape[1], g.shape[1])
        assert (z["ids"][:, :n] != g[:, :n]).any() or z["ids"].shape != g.shape


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "whisper_trtllm_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "whisper_trtllm_amd_debug.h")).read()
    assert re.search(r"#define\s+WT_ABI_VERSION\s+3\b", hdr) and _lib.ABI_VERSION == 3
    body = re.search(r"typedef struct \{([^}]*)\} wt_sampling_params;", hdr).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.SamplingParams._fields_] == ["temperature", "seeds", "n_seeds", "seed"]
    for sym, text, table in (("wt_decoder_set_sampling", hdr, _lib.EXPORTS), ("wt_dbg_sample_select", dbg, _lib.DEBUG_EXPORTS),
                             ("wt_dbg_sample_select_scratch_bytes", dbg, _lib.DEBUG_EXPORTS)):
        assert re.search(r"\b" + sym + r"\(", text) and sym in table
    lib = _lib.load()
    assert lib.wt_abi_version() == 3
    for sym in ("wt_decoder_set_sampling", "wt_dbg_sample_select", "wt_dbg_sample_select_scratch_bytes"):
        assert hasattr(lib, sym)


class FakeEngine:
    """generate() returns scripted scores per (original row, temperature); records every call."""
    generate_with_fallback = runtime.WhisperDecoderEngine.generate_with_fallback

    def __init__(self, script, nsp=None, texts=None):
        self.config = {"eos_token_id": 9, "pad_token_id": 0}
        self.script, self.nsp, self.texts, self.calls = script, nsp, texts or {}, []

    def generate(self, hidden, return_logprobs, no_speech_token_id, temperature, seeds, **kw):
        rows = [int(x) for x in hidden[:, 0].tolist()]            # the encoder rows carry their original index
        self.calls.append((temperature, rows, list(seeds)))
        ids = torch.tensor([[1, 100 + r, int(temperature * 10), 9] if r != 2 else [1, 100 + r, 9, 0] for r in rows], dtype=torch.int32)
        avg = torch.tensor([self.script[r].get(temperature, -0.1) for r in rows], dtype=torch.float32)
        n = torch.tensor([3.0 if r != 2 else 2.0 for r in rows])
        sc = runtime.DecodeScores(ids, torch.zeros(ids.shape), avg * n,
                                  torch.tensor([self.nsp[r] for r in rows]) if no_speech_token_id is not None else None, 9)
        return ids, sc


def test_fallback_loop_against_a_scripted_engine():
    hidden = torch.arange(4, dtype=torch.float32)[:, None]
    # row 0 passes at once; row 1 fails at 0 and 0.2, passes at 0.4; row 2 fails everywhere; row 3 fails but is silence
    script = {0: {}, 1: {0.0: -2.0, 0.2: -1.5}, 2: {0.0: -3.0, 0.2: -3.0, 0.4: -3.0}, 3: {0.0: -5.0}}
    eng = FakeEngine(script, nsp=[0.1, 0.1, 0.1, 0.9])
    ids, sc, used = eng.generate_with_fallback(hidden, temperatures=(0.0, 0.2, 0.4), no_speech_token_id=7, seed=50)
    assert [c[0] for c in eng.calls] == [0.0, 0.2, 0.4]
    assert [c[1] for c in eng.calls] == [[0, 1, 2, 3], [1, 2], [1, 2]]                  # only failing rows; no_speech overrides fallback
    assert [c[2] for c in eng.calls] == [[50, 51, 52, 53], [51, 52], [51, 52]]          # seeds follow the original row index
    assert used.tolist() == pytest.approx([0.0, 0.4, 0.4, 0.0])                        # the last temperature is kept (row 2 never passes)
    assert ids[:, 2].tolist() == [0, 4, 9, 0] and ids.shape == (4, 4)
    assert sc.avg_logprob.tolist() == pytest.approx([-0.1, -0.1, -3.0, -5.0])
    assert sc.no_speech_prob.tolist() == pytest.approx([0.1, 0.1, 0.1, 0.9])
    # a None threshold is skipped: nothing fails on avg_logprob, nothing is decoded again
    eng = FakeEngine(script, nsp=[0.1] * 4)
    _ids, _sc, used = eng.generate_with_fallback(hidden, temperatures=(0.0, 0.2), logprob_threshold=None, no_speech_token_id=7)
    assert len(eng.calls) == 1 and used.tolist() == [0.0] * 4
    # no_speech_threshold None: the silent row falls back like the others
    eng = FakeEngine(script, nsp=[0.1, 0.1, 0.1, 0.9])
    eng.generate_with_fallback(hidden, temperatures=(0.0, 0.2), no_speech_threshold=None, no_speech_token_id=7)
    assert eng.calls[1][1] == [1, 2, 3]
    # the compression ratio: a repetitive text fails, through text_of
    eng = FakeEngine({r: {} for r in range(4)}, nsp=[0.1] * 4)
    text_of = lambda row: "ab " * 200 if row[1] == 101 and row[2] == 0 else "a plain sentence"
    _ids, _sc, used = eng.generate_with_fallback(hidden, temperatures=(0.0, 0.2), text_of=text_of)
    assert used.tolist() == pytest.approx([0.0, 0.2, 0.0, 0.0]) and eng.calls[1][1] == [1]
    # without a vocabulary the default text is the ids in decimal
    assert runtime._default_text_of({})([1, 22, 333]) == "1 22 333"


def test_python_refusals():
    for bad in (float("nan"), float("inf"), "hot"):
        with pytest.raises(ValueError):
            runtime._check_sampling_args(bad, 0, None, 2, 1)
    with pytest.raises(ValueError):
        runtime._check_sampling_args(0.5, 0, None, 2, 2)             # beams
    with pytest.raises(ValueError):
        runtime._check_sampling_args(0.5, 0, [1], 2, 1)              # too few seeds
    assert runtime._check_sampling_args(0.0, 3, None, 2, 4) == []     # off: nothing to refuse
    assert runtime._check_sampling_args(0.5, 3, None, 2, 1) == [3, 4]
    assert runtime._check_sampling_args(0.5, 0, [7, 8, 9], 2, 1) == [7, 8]
