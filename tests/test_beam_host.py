"""CPU: beam search (include/whisper_trtllm_amd.h (9c)).  A float64 restatement of select + process + finalize (the semantics of
transformers' beam_search with BeamSearchScorer / BeamHypotheses), fed the candidates the reference recorded
(tests/golden/make_golden_beam.py), reproduces the recorded beam_idx, tokens, beam scores, done flags, final ids and scores; the header
declares and the library exports the new symbols; the Python layer refuses what the engine refuses."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["beam-toy_b3x2", "beam-toy_b2x4", "beam-tiny_b2x4"]


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------
def rank_key(score, flat):
    """Sort key of a candidate: NaN first, then descending score, lowest flat index (beam * V + id) first among equals."""
    return (0, 0.0, flat) if score != score else (1, -score, flat)


def ref_candidates(logits, beam_scores, mask, at_begin, forced, K):
    """One utterance.  logits [nb, V] (any float dtype), beam_scores [nb], mask uint8 [V] (bit 0: suppressed, bit 1: suppressed at
    begin), forced token or -1.  Returns the K best (score, token, beam), sorted: log_softmax over ALL ids first (a NaN logit ranks first
    and is left out of the log-sum-exp), then the masks / the forced id on the log-probabilities, plus the beam score."""
    nb, V = logits.shape
    x = logits.astype(np.float64)
    cands = []
    for j in range(nb):
        if forced >= 0:
            cands.append((0.0 + float(beam_scores[j]), forced, j))
            continue
        row = x[j]
        ok = ~np.isnan(row) & ~np.isneginf(row)
        m = row[ok].max() if ok.any() else -np.inf
        lse = m + np.log(np.exp(row[ok] - m).sum()) if ok.any() else np.nan
        sc = row - lse + float(beam_scores[j])
        dead = ((mask & 1) != 0) | (((mask & 2) != 0) & at_begin)
        sc = np.where(dead, -np.inf, sc)
        # only the K best of a row can be among the utterance's K best
        order = sorted(range(V), key=lambda v: rank_key(sc[v], v))[:K]
        cands += [(float(sc[v]), v, j) for v in order]
    cands.sort(key=lambda c: rank_key(c[0], c[2] * V + c[1]))
    return cands[:K]


class Hyps:
    """BeamHypotheses of one utterance."""

    def __init__(self, nb, lp, early):
        self.nb, self.lp, self.early, self.beams, self.worst = nb, lp, early, [], 1e9

    def add(self, ids, sum_logprobs):
        score = sum_logprobs / (len(ids) ** self.lp)
        if len(self.beams) < self.nb or score > self.worst:
            self.beams.append((score, list(ids)))
            if len(self.beams) > self.nb:
                order = sorted((s, i) for i, (s, _h) in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum, cur_len):
        if len(self.beams) < self.nb:
            return False
        return True if self.early else self.worst >= best_sum / cur_len ** self.lp


class RefBeam:
    """process + finalize for U utterances x nb beams; `ids` are the rows' histories (lists)."""

    def __init__(self, U, nb, lp, early, eos, pad, start):
        self.U, self.nb, self.eos, self.pad = U, nb, eos, pad
        self.hyps = [Hyps(nb, lp, early) for _ in range(U)]
        self.done = [False] * U
        self.ids = [[start] for _ in range(U * nb)]
        self.scores = [0.0 if j == 0 else -1e9 for _u in range(U) for j in range(nb)]

    def process(self, cands):
        """cands[u]: sorted (score, token, beam) of utterance u (ignored when it is done).  Returns per row (token, source beam)."""
        nb, cur_len = self.nb, len(self.ids[0])
        out, new_ids, new_scores = [], [], []
        for u in range(self.U):
            if self.done[u]:
                for j in range(nb):
                    out.append((self.pad, j))
                    new_ids.append(self.ids[u * nb + j] + [self.pad])
                    new_scores.append(0.0)
                continue
            n = 0
            for rank, (sc, tok, j) in enumerate(cands[u]):
                if tok == self.eos:
                    if rank < nb:
                        self.hyps[u].add(self.ids[u * nb + j], sc)
                    continue
                out.append((tok, j))
                new_ids.append(self.ids[u * nb + j] + [tok])
                new_scores.append(sc)
                n += 1
                if n == nb:
                    break
            assert n == nb, "fewer than num_beams continuations"
            self.done[u] = self.hyps[u].is_done(cands[u][0][0], cur_len + 1)
        self.ids, self.scores = new_ids, new_scores
        return out

    def finalize(self, max_length):
        nb = self.nb
        rows, scores = [], []
        for u in range(self.U):
            h = self.hyps[u]
            if not self.done[u]:
                for j in range(nb):
                    h.add(self.ids[u * nb + j], self.scores[u * nb + j])
            score, best = sorted(h.beams, key=lambda x: x[0])[-1]
            rows.append(best)
            scores.append(score)
        width = min(max(len(r) for r in rows) + 1, max_length)
        out = np.full((self.U, width), self.pad, dtype=np.int64)
        for u, r in enumerate(rows):
            out[u, :len(r)] = r
            if len(r) < width:
                out[u, len(r)] = self.eos
        return out, np.array(scores)


def load_beam_case(case):
    z = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    import whisper_trtllm_amd as w
    cfg = w.synthetic.get_config(str(z["config_name"]))
    cfg.update(json.loads(str(z["overrides_json"])))
    return z, cfg


def live_rows(z, t):
    """Rows of step t whose utterance was not done before it and whose recorded beam score is above the -1e9 start scores (the order the
    reference gives bit-equal start-score candidates is torch.topk's choice: make_golden_beam.py)."""
    nb = int(z["num_beams"])
    return np.repeat(~z["done_before"][t], nb) & (z["beam_scores"][t] > -1e8)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_recorded_decode(case):
    z, cfg = load_beam_case(case)
    U, nb = int(z["batch"]), int(z["num_beams"])
    # min_gap: every decision of the recorded decode, see make_golden_beam.py -- it leaves out pairs of candidates both at -inf and pairs
    # of beams both still at their -1e9 start score (bit-equal on both sides, never a decision about a token); beam_idx is compared
    # below only for rows above -1e8 for the same reason (live_rows)
    assert float(z["min_gap"]) >= 1e-3
    ref = RefBeam(U, nb, float(z["length_penalty"]), bool(z["early_stopping"]), cfg["eos_token_id"], cfg["pad_token_id"], cfg["decoder_start_token_id"])
    steps = z["tokens"].shape[0]
    saw_reorder = False
    for t in range(steps):
        K = 2 * nb
        cands = [[(float(z["cand_scores"][t, u, r]), int(z["cand_tokens"][t, u, r]), int(z["cand_beams"][t, u, r])) for r in range(K)] for u in range(U)]
        out = ref.process(cands)
        live = live_rows(z, t)
        tok = np.array([o[0] for o in out])
        src = np.array([o[1] for o in out]) + np.repeat(np.arange(U), nb) * nb
        alive = np.repeat(~z["done_before"][t], nb)
        np.testing.assert_array_equal(tok[alive], z["tokens"][t][alive])
        np.testing.assert_array_equal(src[live], z["beam_idx"][t][live])
        np.testing.assert_allclose(np.array(ref.scores)[alive], z["beam_scores"][t][alive], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(np.array(ref.done), z["done"][t])
        saw_reorder |= bool((z["beam_idx"][t][live] != np.arange(U * nb)[live]).any())
    ids, scores = ref.finalize(cfg["max_length"])
    np.testing.assert_array_equal(ids, z["ids"])
    np.testing.assert_allclose(scores, z["scores"], rtol=0, atol=1e-6)
    assert saw_reorder, "the case never reorders its beams"
    g = z["greedy_ids"]
    assert ids.shape != g.shape or not np.array_equal(ids, g), "the beam result equals the greedy ids"


def test_candidate_order_of_the_restatement():
    """ties go to the lowest flat index, NaN ranks first, masked ids are -inf, a forced step keeps one id per beam"""
    V = 11
    x = np.zeros((2, V), dtype=np.float32)
    mask = np.zeros(V, dtype=np.uint8)
    c = ref_candidates(x, np.array([0.0, 0.0]), mask, False, -1, 4)
    assert [(t, j) for _s, t, j in c] == [(0, 0), (1, 0), (2, 0), (3, 0)]
    x[1, 5] = np.nan
    mask[0] = 1
    c = ref_candidates(x, np.array([0.0, 0.0]), mask, False, -1, 4)
    # (beam 1's log-sum-exp runs over 10 ids instead of 11: its ids score higher; id 0 is masked)
    assert (c[0][1], c[0][2]) == (5, 1) and (c[1][1], c[1][2]) == (1, 1)
    c = ref_candidates(x, np.array([0.0, -1e9]), mask, False, 7, 4)
    assert c == [(0.0, 7, 0), (-1e9, 7, 1)]


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_declares_and_library_exports_the_beam_symbols():
    import whisper_trtllm_amd as w
    h, hd = _header("whisper_trtllm_amd.h"), _header("whisper_trtllm_amd_debug.h")
    assert re.search(r"typedef struct \{\s*int32_t num_beams;\s*float length_penalty;\s*int32_t early_stopping;[^}]*\} wt_beam_params;", h)
    for sym in ("wt_decoder_set_beam_search", "wt_decoder_read_beam_scores"):
        assert re.search(r"\bint " + sym + r"\(", h), sym
        assert sym in w._lib.EXPORTS
    for sym in ("wt_dbg_beam_select", "wt_dbg_beam_select_scratch_bytes", "wt_dbg_decode_attention_beam", "wt_dbg_decode_attention_rows", "wt_dbg_beam_trace"):
        assert re.search(r"\b" + sym + r"\(", hd), sym
        assert sym in w._lib.DEBUG_EXPORTS
    lib = w._lib.load()   # loads without a GPU and resolves every symbol it binds
    for sym in ("wt_decoder_set_beam_search", "wt_decoder_read_beam_scores", "wt_dbg_beam_select", "wt_dbg_beam_trace"):
        assert getattr(lib, sym) is not None
    assert ctypes_sizeof_beam_params(w) == 12


def ctypes_sizeof_beam_params(w):
    import ctypes
    return ctypes.sizeof(w._lib.BeamParams)


def test_python_refuses_beam_search_where_the_engine_does():
    import whisper_trtllm_amd as w
    from whisper_trtllm_amd import runtime
    dec = object.__new__(w.WhisperDecoderEngine)   # the refusals come before anything touches the handle
    with pytest.raises(ValueError, match="beam search"):
        dec.stream(slots=2, num_beams=2)
    with pytest.raises(ValueError, match="beam search"):
        runtime.transcribe_continuous(None, dec, [], num_beams=4)
    with pytest.raises(ValueError, match="timestamp"):
        dec.generate(None, num_beams=2, return_timestamps=True)
    with pytest.raises(ValueError, match="timestamp"):
        dec.begin(None, num_beams=2, return_timestamps=True)
    with pytest.raises(ValueError, match="force_eos"):
        dec.generate(None, num_beams=2, force_eos_step=3)
    with pytest.raises(ValueError, match="num_beams"):
        dec.generate(None, num_beams=9)
    with pytest.raises(ValueError, match="return_scores"):
        dec.generate(None, return_scores=True)
