#!/usr/bin/env python3
"""Golden vectors of beam search from the REFERENCE's bundled HuggingFace Whisper (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_beam.py [case ...]   (no case = all)
      ... make_golden_beam.py --scan case [first_seed n_seeds]    (prints the seeds / EOS ids that pass the conditions below)
The reference model's `beam_search` is called directly with a BeamSearchScorer and the processor list generate() would build
(SuppressTokens, SuppressTokensAtBegin, ForceTokens).  Recorded per case (tests/golden/<case>.npz): final ids and sequence scores, the
greedy ids of the same weights, and per step the sorted top 2 * num_beams + 1 candidate scores (float64) with their tokens and source
beams, the chosen beam_idx / tokens / beam scores and the done flags.

A case is kept only if every decision is at least 1e-3 wide (tests/golden/find_healthy_seeds.py's criterion): all adjacent gaps among the
recorded candidates, every comparison BeamHypotheses makes (add against the worst kept score, is_done) and the best against the second
hypothesis at the end.  Two kinds of pairs are not decisions and are left out: two candidates at -inf (masked or not forced: both sides
compute exactly -inf and the walk never reaches them, which is asserted), and two candidates of beams still at their -1e9 start score
(float32 spacing 64 there: bit-equal sums on both sides; such beams share one history, so their order cannot change a token -- they only
occur at the forced first step with more than two beams; the reference's order among them is torch.topk's choice, not the flat index,
so a test compares beam_idx only for rows whose recorded beam score is above -1e8).  The tiny.en case shares weights and mels with
tiny_b2, so it has one seed: --scan shortens it (max_length 17, 15, ...) until it is healthy.
Every case must also contain a step whose beam_idx is not the identity and an utterance whose beam result differs from its greedy ids."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import build_hf, import_reference_hf  # noqa: E402

GAP = 1e-3
CASES = {  # case: (config, weight seed, utterances, beams, length_penalty, early_stopping, overrides, needs an early and a full-length utterance)
    "beam-toy_b3x2": ("toy-short", 0, 3, 2, 1.0, False, {}, True),
    "beam-toy_b2x4": ("toy-short", 0, 2, 4, 0.8, True, {}, True),
    # shares weights and mels with tiny_b2
    "beam-tiny_b2x4": ("whisper-tiny.en", 14, 2, 4, 1.0, False, {"max_length": 17}, False),
}
CHOSEN = os.path.join(HERE, "beam_cases.json")   # seeds / EOS ids found by --scan


def processors(cfg):
    from transformers.generation.logits_process import (ForceTokensLogitsProcessor, LogitsProcessorList,
                                                        SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)
    forced = cfg.get("forced_decoder_ids") or []
    begin_index = 1 + (forced[-1][0] if forced else 0)
    procs = [SuppressTokensLogitsProcessor(cfg["suppress_tokens"]), SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], begin_index)]
    if forced:
        procs.append(ForceTokensLogitsProcessor(forced))
    return LogitsProcessorList(procs)


def record(model, cfg, enc_out, U, nb, lp, early, BaseModelOutput):
    from transformers.generation import beam_search as bs_mod
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList
    K = 2 * nb
    max_length = cfg["max_length"]
    steps, margins = [], []
    state = {"beam_scores": torch.tensor([0.0] + [-1e9] * (nb - 1)).repeat(U)}

    class Tap:   # last in the list: the processed log-probabilities of the step
        def __call__(self, input_ids, scores):
            full = (scores + state["beam_scores"][:, None]).view(U, -1)
            v, i = torch.topk(full, K + 1, dim=1, largest=True, sorted=True)
            state["cand"] = (v.double().numpy(), (i % scores.shape[-1]).numpy(), (i // scores.shape[-1]).numpy())
            return scores

    scorer = bs_mod.BeamSearchScorer(batch_size=U, num_beams=nb, device="cpu", length_penalty=lp, do_early_stopping=early)
    process = scorer.process

    def spy_process(input_ids, next_scores, next_tokens, next_indices, **kw):
        was_done = scorer._done.clone().numpy()
        out = process(input_ids, next_scores, next_tokens, next_indices, **kw)
        cv, ct, cs = state["cand"]
        # the first K are the reference's own top-k (the order of exactly equal scores is topk's choice), the last one the tap's
        assert np.array_equal(cv[:, :K], next_scores.double().numpy())
        ct, cs = ct.copy(), cs.copy()
        ct[:, :K], cs[:, :K] = next_tokens.numpy(), next_indices.numpy()
        state["beam_scores"] = out["next_beam_scores"].clone()
        steps.append(dict(cand_scores=cv, cand_tokens=ct, cand_beams=cs, tokens=out["next_beam_tokens"].numpy().copy(),
                          beam_idx=out["next_beam_indices"].numpy().copy(), beam_scores=out["next_beam_scores"].numpy().copy(),
                          done_before=was_done, done=scorer._done.clone().numpy()))
        return out
    scorer.process = spy_process
    add, is_done = bs_mod.BeamHypotheses.add, bs_mod.BeamHypotheses.is_done

    def spy_add(self, hyp, sum_logprobs, beam_indices=None):
        if len(self) >= self.num_beams:
            margins.append(abs(sum_logprobs / (hyp.shape[-1] ** self.length_penalty) - self.worst_score))
        return add(self, hyp, sum_logprobs, beam_indices=beam_indices)

    def spy_is_done(self, best_sum_logprobs, cur_len):
        if len(self) >= self.num_beams and self.early_stopping is False:
            margins.append(abs(self.worst_score - best_sum_logprobs / cur_len ** self.length_penalty))
        return is_done(self, best_sum_logprobs, cur_len)
    bs_mod.BeamHypotheses.add, bs_mod.BeamHypotheses.is_done = spy_add, spy_is_done
    procs = processors(cfg)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            greedy = model.greedy_search(torch.full((U, 1), cfg["decoder_start_token_id"], dtype=torch.long), logits_processor=procs,
                                         stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]), pad_token_id=cfg["pad_token_id"],
                                         eos_token_id=cfg["eos_token_id"], encoder_outputs=BaseModelOutput(last_hidden_state=enc_out), use_cache=True)
            procs.append(Tap())
            out = model.beam_search(torch.full((U * nb, 1), cfg["decoder_start_token_id"], dtype=torch.long), scorer, logits_processor=procs,
                                    stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length)]), pad_token_id=cfg["pad_token_id"],
                                    eos_token_id=cfg["eos_token_id"], output_scores=True, return_dict_in_generate=True,
                                    encoder_outputs=BaseModelOutput(last_hidden_state=enc_out.repeat_interleave(nb, dim=0)), use_cache=True)
    finally:
        bs_mod.BeamHypotheses.add, bs_mod.BeamHypotheses.is_done = add, is_done
    for hyps in scorer._beam_hyps:   # best against second at the end
        sc = sorted(s for s, _h, _b in hyps.beams)
        if len(sc) > 1:
            margins.append(sc[-1] - sc[-2])
    return out.sequences.numpy().astype(np.int64), out.sequences_scores.numpy().astype(np.float64), greedy.numpy().astype(np.int64), steps, margins


def health(steps, nb, V, eos):
    """(smallest decision gap, problems) of a recorded decode."""
    K, lo, bad = 2 * nb, np.inf, []
    for t, s in enumerate(steps):
        for u in range(s["cand_scores"].shape[0]):
            if s["done_before"][u]:
                continue
            v, tk, bm = s["cand_scores"][u], s["cand_tokens"][u], s["cand_beams"][u]
            used, kept = 0, 0
            for r in range(K):   # the candidates the walk consumes
                used = r + 1
                kept += tk[r] != eos
                if kept == nb:
                    break
            if not np.isfinite(v[:used]).all():
                bad.append(f"step {t} utterance {u}: the walk reaches a -inf candidate")
            for r in range(K):
                a, b = v[r], v[r + 1]
                if np.isinf(a) and np.isinf(b):
                    continue
                if a <= -1e8 and b <= -1e8:
                    continue
                lo = min(lo, a - b)
    return lo, bad


def run_case(case, seed, eos, models, max_length=None):
    cname, _seed, U, nb, lp, early, overrides, want_mix = CASES[case]
    if max_length is not None:
        overrides = dict(overrides, max_length=max_length)
    from whisper_trtllm_amd import synthetic
    WhisperConfig, Model, BaseModelOutput = models
    cfg = synthetic.get_config(cname)
    cfg.update(overrides)
    if eos is not None:
        cfg.update(eos_token_id=int(eos), pad_token_id=int(eos))
    weights = synthetic.make_weights(cfg, seed)
    mel = synthetic.make_mel(cfg, index=7 * seed, batch=U)
    model = build_hf(cfg, weights, WhisperConfig, Model)
    with torch.no_grad():
        enc_out = model.model.encoder(torch.from_numpy(mel)).last_hidden_state
        ids, scores, greedy, steps, margins = record(model, cfg, enc_out, U, nb, lp, early, BaseModelOutput)
    lo, bad = health(steps, nb, cfg["vocab_size"], cfg["eos_token_id"])
    lo = min([lo] + margins)
    ident = np.tile(np.arange(nb), U) + np.repeat(np.arange(U), nb) * nb
    if not any((s["beam_idx"] != ident)[np.repeat(~s["done_before"], nb)].any() for s in steps):
        bad.append("beam_idx is the identity at every step")
    w = min(ids.shape[1], greedy.shape[1])
    if ids.shape[1] == greedy.shape[1] and np.array_equal(ids, greedy):
        bad.append("the beam result equals the greedy ids")
    elif all(np.array_equal(ids[u, :w], greedy[u, :w]) for u in range(U)) and ids.shape[1] == greedy.shape[1]:
        bad.append("the beam result equals the greedy ids")
    done_at = [next((t for t, s in enumerate(steps) if s["done"][u]), None) for u in range(U)]
    if want_mix and not (any(d is not None and d < len(steps) - 1 for d in done_at) and any(d is None for d in done_at)):
        bad.append(f"needs an utterance done early and one running to max_length (done at {done_at} of {len(steps)} steps)")
    if lo < GAP:
        bad.append(f"smallest decision gap {lo:.3e} < {GAP}")
    return cfg, ids, scores, greedy, steps, lo, bad, done_at


def main():
    sys.path.insert(0, ROOT)
    import whisper_trtllm_amd  # noqa: F401  (alias loader for the hyphenated package dir)
    models = import_reference_hf()
    chosen = json.load(open(CHOSEN)) if os.path.exists(CHOSEN) else {}
    if len(sys.argv) > 2 and sys.argv[1] == "--scan":
        case = sys.argv[2]
        first, n = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, 40)
        remap = CASES[case][7]
        if not remap:
            for ml in range(CASES[case][6]["max_length"], 5, -2):
                *_x, lo, bad, done_at = run_case(case, CASES[case][1], None, models, ml)
                print(f"[{case}] max_length {ml}: gap {lo:.3e} {'OK' if not bad else '; '.join(bad)}", flush=True)
                if not bad:
                    chosen[case] = {"seed": CASES[case][1], "eos": None, "max_length": ml}
                    json.dump(chosen, open(CHOSEN, "w"), indent=1, sort_keys=True)
                    return
            return
        for seed in ([CASES[case][1]] if not remap else range(first, first + n)):
            eos_ids = [None]
            if remap:   # EOS candidates: the text tokens the decode emits with the default EOS
                _cfg, ids, _s, greedy, steps, *_ = run_case(case, seed, None, models)
                toks = np.concatenate([s["tokens"] for s in steps])
                eos_ids = [int(t) for t in np.unique(toks) if t < 500][:24]
            for eos in eos_ids:
                _cfg, ids, _s, _g, steps, lo, bad, done_at = run_case(case, seed, eos, models)
                print(f"[{case}] seed {seed} eos {eos}: gap {lo:.3e} done_at {done_at} {'OK' if not bad else '; '.join(bad)}", flush=True)
                if not bad:
                    chosen[case] = {"seed": seed, "eos": eos}
                    json.dump(chosen, open(CHOSEN, "w"), indent=1, sort_keys=True)
                    return
        return
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case not in only:
            continue
        cname, seed, U, nb, lp, early, overrides, _mix = CASES[case]
        pick = chosen.get(case, {"seed": seed, "eos": None})
        cfg, ids, scores, greedy, steps, lo, bad, done_at = run_case(case, pick["seed"], pick["eos"], models, pick.get("max_length"))
        if pick.get("max_length"):
            overrides = dict(overrides, max_length=pick["max_length"])
        print(f"[{case}] seed {pick['seed']} eos {pick['eos']} ids {ids.shape} steps {len(steps)} done_at {done_at} | min decision gap {lo:.3e}")
        for r, g in zip(ids, greedy):
            print("    beam  ", r.tolist(), "\n    greedy", g.tolist())
        assert not bad, "unhealthy case: " + "; ".join(bad)
        if pick["eos"] is not None:
            overrides = dict(overrides, eos_token_id=pick["eos"], pad_token_id=pick["eos"])
        out = {"config_name": cname, "seed": pick["seed"], "batch": U, "num_beams": nb, "length_penalty": lp, "early_stopping": int(early),
               "mel_index": 7 * pick["seed"], "overrides_json": json.dumps(overrides), "ids": ids, "scores": scores, "greedy_ids": greedy,
               "min_gap": lo}
        for k in steps[0]:
            out[k] = np.stack([s[k] for s in steps])
        path = os.path.join(HERE, case + ".npz")
        np.savez_compressed(path, **out)
        print("   wrote", case + ".npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
