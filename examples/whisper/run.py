#!/usr/bin/env python3
"""Run the engines built by build_encoder.py / build_decoder.py — the reference's examples/whisper/run.py flow.

Two decode paths over the same C-ABI:
  * Session path (default with --session): `WhisperEncoder` / `WhisperDecoder` wrappers + `greedy_search`, i.e. the
    reference's per-token `Session.run` protocol with by-value caches (run.py:57-227), batch 1;
  * fast path (default): resident in-place KV cache, on-device greedy loop, utterance batches of 8
    (`WhisperEncoderEngine` / `WhisperDecoderEngine`).
Inputs: `--audio a.wav ...` (16 kHz mono; log-mel on the GPU front-end, transcripts printed when `--whisper` is a checkpoint
directory with vocab.json) or, without audio on the box, `--synthetic N` seeded synthetic 80x3000 log-mels (outputs are token ids).
Multi-GPU: under `python -m torch.distributed.run --nproc-per-node N ...` the fast path shards the utterances over the ranks
(one process per GPU, full weight replica each, no data-path collective); ids are gathered on the host and rank 0 reports."""
import argparse
import os
import pickle
import time

import torch

from _common import ROOT  # noqa: F401

import whisper_trtllm_amd as tensorrt_llm
from whisper_trtllm_amd import trt
from whisper_trtllm_amd.generation import get_logits_processor, get_stopping_criteria, greedy_search
from whisper_trtllm_amd.runtime import Session, TensorInfo, _scoped_stream

_trt_to_torch_dtype_dict = {trt.float16: torch.float16, trt.float32: torch.float32, trt.int32: torch.int32, trt.int8: torch.int8}
_torch_to_trt_dtype_dict = {v: k for k, v in _trt_to_torch_dtype_dict.items()}


def parse_arguments():
    parser = argparse.ArgumentParser()
    parser.add_argument("--whisper", type=str, default="synthetic:whisper-tiny.en")
    parser.add_argument("--engine_precision", type=str, default="float32")
    parser.add_argument("--log_level", type=str, default="error")
    parser.add_argument("--engine_dir", type=str, default="whisper_outputs")
    parser.add_argument("--compare", action="store_true", help="also decode through the Session path and compare ids")
    parser.add_argument("--session", action="store_true", help="decode through the per-token Session protocol only")
    parser.add_argument("--synthetic", type=int, default=8, help="number of synthetic utterances")
    parser.add_argument("--synthetic_start", type=int, default=0, help="index of the first synthetic utterance (synthetic.make_mel)")
    parser.add_argument("--audio", nargs="+", default=None, help="16 kHz mono audio files to transcribe instead (log-mel by the GPU "
                        "front-end, i.e. what hf_processor does in the reference, run.py:267); with --whisper <checkpoint dir> the ids "
                        "are also decoded to text (vocab.json)")
    parser.add_argument("--max_length", type=int, default=None)
    parser.add_argument("--batching", choices=["continuous", "sorted", "dataset"], default="sorted",
                        help="fast path: continuous (arrival order, 8 decode slots refilled on the device the step an utterance stops -- every "
                             "utterance ends at its own EOS like the reference's batch-1 loop, run.py:219-226), length-aware batches (by the audio "
                             "duration recovered from the log-mel's trailing padding) or dataset-order batches")
    parser.add_argument("--workers", type=int, default=2, help="fast path: engine pairs per GPU, each on its own stream and host thread")
    parser.add_argument("--dist-backend", type=str, default=None, help="nccl (= RCCL) | gloo; default: nccl when every rank has its own GPU")
    parser.add_argument("--dump_ids", type=str, default=None, help="rank 0 writes the fast-path token ids as JSON (tests)")
    parser.add_argument("--return_timestamps", action="store_true", help="Whisper's timestamp mode: <|t|> tokens (t x 0.02 s) between "
                        "segments; printed as [start --> end] text segments with a tokenizer, as ids with <|t|> marks otherwise")
    parser.add_argument("--return_token_timestamps", action="store_true", help="fast path: per-token times by cross-attention DTW on the "
                        "device, printed as words with [start --> end] (with a tokenizer) or as ids with their times; needs a batch plan, no beams")
    parser.add_argument("--alignment_heads", nargs="+", default=None, metavar="LAYER,HEAD", help="alignment heads for "
                        "--return_token_timestamps, e.g. 2,1 3,0 (default: the checkpoint's generation_config.json; synthetic models have none)")
    parser.add_argument("--median_filter_width", type=int, default=None, help="default: the config's median_filter_width, else 7")
    parser.add_argument("--num_beams", type=int, default=1, help="fast path: beam search on the device with this many beams (<= 8; batches are "
                        "sized so that utterances x beams <= 16 rows); needs a batch plan and no --return_timestamps")
    parser.add_argument("--return_logprobs", action="store_true", help="fast path: token log-probabilities from the device; prints avg_logprob, "
                        "no_speech_prob (with --no_speech_token_id) and the compression ratio per utterance, and each word's mean token "
                        "log-probability with --return_token_timestamps; needs a batch plan, no beams")
    parser.add_argument("--no_speech_token_id", type=int, default=None, help="the <|nospeech|> (<|nocaptions|>) id whose first-step probability "
                        "--return_logprobs reports as no_speech_prob")
    parser.add_argument("--temperature", type=float, default=0.0, help="fast path: sample every token from softmax(scores / T) on the device "
                        "instead of the argmax (utterance i draws with seed --seed + i); implies --return_logprobs; needs a batch plan, no beams")
    parser.add_argument("--seed", type=int, default=0, help="base seed of --temperature / --temperature_fallback")
    parser.add_argument("--temperature_fallback", action="store_true", help="fast path: openai-whisper's quality loop -- decode greedily, "
                        "then decode the utterances whose transcript is repetitive (compression ratio > 2.4) or unlikely (avg_logprob < -1) "
                        "again at temperature 0.2, 0.4 .. 1.0 (not those whose no_speech_prob > 0.6, with --no_speech_token_id); implies "
                        "--return_logprobs; prints the temperature used per utterance")
    parser.add_argument("--prompt_ids", type=int, nargs="+", default=None, metavar="N", help="fast path: a decoder prompt in front of the "
                        "transcript, shared by every utterance -- token ids, the first of them <|startofprev|> (previous text / "
                        "initial_prompt; text -> ids is the caller's: there is no BPE encoder here); needs a batch plan, an fp32 decoder "
                        "engine, no beams and no --return_token_timestamps")
    parser.add_argument("--long_form", action="store_true", help="transcribe recordings of any length (--audio files whole, or --synthetic "
                        "noise recordings of 2.5 windows): openai-whisper's seek loop with the temperature fallback, batched over the files "
                        "(runtime.transcribe_long); prints [start --> end] text per file; single rank, fp32 decoder engine, no beams")
    parser.add_argument("--no_condition_on_previous_text", action="store_true", help="--long_form: do not prompt a window with the text before it")
    parser.add_argument("--max_rows", type=int, default=8, help="--long_form: recordings decoded side by side (<= 16)")
    parser.add_argument("--language", type=str, default=None, help="fast path, multilingual checkpoints: auto (detect every utterance's "
                        "language in the first step of its decode), a code (en), a token (<|en|>) or a token id; prints the language per "
                        "utterance; needs a batch plan, no beams, no --return_token_timestamps; with --long_form a recording keeps the "
                        "language of its first window")
    parser.add_argument("--task", type=str, default=None, help="transcribe | translate (the checkpoint's task_to_id) or a token id: "
                        "replaces the task token of the forced list")
    parser.add_argument("--detect_language", action="store_true", help="fast path: only detect and print every utterance's language "
                        "(one decoder step per batch)")
    parser.add_argument("--length_penalty", type=float, default=1.0)
    parser.add_argument("--early_stopping", action="store_true")
    args = parser.parse_args()
    if args.num_beams < 1 or args.num_beams > 8:
        parser.error("--num_beams must be in [1, 8]")
    if args.num_beams > 1 and (args.batching == "continuous" or args.return_timestamps or args.session or args.compare):
        parser.error("--num_beams needs the fast path with a batch plan (--batching sorted | dataset): no --return_timestamps, --session or "
                     "--compare (the Session path decodes greedily)")
    if args.return_token_timestamps and (args.batching == "continuous" or args.num_beams > 1 or args.session):
        parser.error("--return_token_timestamps needs the fast path with a batch plan (--batching sorted | dataset) and no beams: the "
                     "continuous mode keeps no query history, beam search no beam_indices, the Session path no cross attentions")
    if args.temperature_fallback and (args.temperature > 0 or args.return_token_timestamps):
        parser.error("--temperature_fallback takes no --temperature (it walks 0, 0.2 .. 1.0) and no --return_token_timestamps")
    if not (args.temperature >= 0 and args.temperature < float("inf")):
        parser.error("--temperature must be a finite number >= 0")
    if args.temperature > 0 or args.temperature_fallback:
        args.return_logprobs = True
    if args.return_logprobs and (args.batching == "continuous" or args.num_beams > 1 or args.session):
        parser.error("--return_logprobs needs the fast path with a batch plan (--batching sorted | dataset) and no beams")
    if args.no_speech_token_id is not None and not args.return_logprobs:
        parser.error("--no_speech_token_id needs --return_logprobs")
    if args.prompt_ids is not None and (args.batching == "continuous" or args.num_beams > 1 or args.return_token_timestamps or args.session
                                        or args.compare or args.engine_precision != "float32"):
        parser.error("--prompt_ids needs the fast path with a batch plan (--batching sorted | dataset) and an fp32 decoder engine: no beams, "
                     "no --return_token_timestamps, no --session / --compare (the Session path takes no prompt)")
    if args.long_form and (args.session or args.compare or args.num_beams > 1 or args.return_token_timestamps or args.prompt_ids is not None
                           or args.batching == "continuous" or args.engine_precision != "float32" or args.temperature > 0):
        parser.error("--long_form runs the batched seek loop on an fp32 decoder engine: no --session / --compare, beams, "
                     "--return_token_timestamps, --prompt_ids, --temperature (it walks the fallback's list) or --batching continuous")
    if args.long_form and not 1 <= args.max_rows <= 16:
        parser.error("--max_rows must be in [1, 16]")
    if args.detect_language and args.language is None:
        args.language = "auto"
    for key in ("language", "task"):     # ids may be given as numbers
        v = getattr(args, key)
        if v is not None and v.lstrip("-").isdigit():
            setattr(args, key, int(v))
    if (args.language is not None or args.task is not None) and (args.session or args.compare or args.batching == "continuous"):
        parser.error("--language / --task / --detect_language need the fast path with a batch plan (--batching sorted | dataset): no --session / --compare")
    if args.language is not None and (args.num_beams > 1 or args.return_token_timestamps):
        parser.error("--language takes no beams and no --return_token_timestamps")
    if args.alignment_heads is not None:
        try:
            args.alignment_heads = [tuple(int(x) for x in pair.split(",")) for pair in args.alignment_heads]
            assert all(len(p) == 2 for p in args.alignment_heads)
        except (ValueError, AssertionError):
            parser.error("--alignment_heads takes LAYER,HEAD pairs, e.g. 2,1 3,0")
    if args.return_timestamps and args.batching == "continuous":
        parser.error("--return_timestamps needs a batch plan (--batching sorted | dataset): the continuous mode predicts no timestamps")
    return args


def trim_after_eos(row, eos, pad):
    """A batched fast-path row is padded with `pad` up to the longest row of its batch; a batch-1 Session row stops at its own EOS
    (run.py:219-226).  Cut a row behind its first EOS so the two are comparable (pad == eos for the .en checkpoints)."""
    row = list(row)
    if eos in row[1:]:
        row = row[:row.index(eos, 1) + 1]
    while len(row) > 1 and row[-1] == pad and pad != eos:
        row.pop()
    return row


class WhisperEncoder:
    """Engine wrapper with the reference's call signature (run.py:57-93): mel [1,80,3000] -> hidden [1,1500,d]."""

    def __init__(self, args=None, config=None):
        with open(os.path.join(args.engine_dir, "WhisperEncoder.engine"), "rb") as f:
            self.session = Session.from_serialized_engine(f.read())
        frames = 2 * config["max_source_positions"]
        outputs_shape = self.session.infer_shapes([TensorInfo("data", trt.float32, (1, config["num_mel_bins"], frames)),
                                                   TensorInfo("length", trt.float32, (1,))])
        self.inputs = {"data": torch.rand(1, config["num_mel_bins"], frames).cuda(), "length": torch.Tensor([1.0]).cuda()}
        self.outputs = {o.name: torch.zeros(*o.shape, dtype=_trt_to_torch_dtype_dict[o.dtype]).cuda() for o in outputs_shape}

    def __call__(self, input):
        self.inputs["data"] = input
        with _scoped_stream() as stream:
            ok = self.session.run(self.inputs, self.outputs, stream)
        assert ok
        return self.outputs["hidden_states"].clone()


class WhisperDecoder:
    """Per-token decoder wrapper with the by-value cache protocol of run.py:95-148 (masks carry lengths only)."""

    def __init__(self, args=None, config=None):
        self.config = config
        with open(os.path.join(args.engine_dir, "WhisperDecoder.engine"), "rb") as f:
            self.session = Session.from_serialized_engine(f.read())

    def __call__(self, decoder_input_ids, encoder_outputs, past_key_values):
        config = self.config
        S = config["max_source_positions"]
        inputs = {"data": decoder_input_ids.to(dtype=torch.int32, device="cuda"),
                  "length": torch.Tensor([1.0]).to(dtype=torch.int32).cuda(),
                  "encoder_hidden_states": encoder_outputs.to(dtype=torch.float32, device="cuda")}
        if past_key_values is None:
            L, H = config["decoder_layers"], config["decoder_attention_heads"]
            dh = config["d_model"] // H
            inputs["self_past_key"] = torch.rand(L, H, 1, dh).cuda()
            inputs["self_past_value"] = torch.rand(L, H, 1, dh).cuda()
            inputs["cross_past_key"] = torch.rand(L, H, S, dh).cuda()
            inputs["cross_past_value"] = torch.rand(L, H, S, dh).cuda()
            inputs["past_self_cache_mask"] = torch.rand(1).cuda()
            inputs["past_cross_cache_mask"] = torch.rand(1).cuda()
        else:
            for name, t in zip(("self_past_key", "self_past_value", "cross_past_key", "cross_past_value"), past_key_values):
                inputs[name] = t.to(dtype=torch.float32, device="cuda")
            inputs["past_self_cache_mask"] = torch.rand(int(1 + past_key_values[0].shape[2]), dtype=torch.float32).cuda()
            inputs["past_cross_cache_mask"] = torch.rand(int(1 + S), dtype=torch.float32).cuda()
        outputs_shape = self.session.infer_shapes([TensorInfo(k, _torch_to_trt_dtype_dict[v.dtype], tuple(v.shape)) for k, v in inputs.items()])
        outputs = {o.name: torch.zeros(*o.shape, dtype=_trt_to_torch_dtype_dict[o.dtype]).cuda() for o in outputs_shape}
        with _scoped_stream() as stream:
            ok = self.session.run(inputs, outputs, stream)
        assert ok
        return outputs["hidden_states"], (outputs["next_self_keys"], outputs["next_self_values"],
                                          outputs["next_cross_keys"], outputs["next_cross_values"])


def decode_with_sessions(whisperencoder, whisperdecoder, config, mel, return_timestamps=False):
    """One utterance through the reference's loop (run.py:266-284)."""
    encoder_outputs = whisperencoder(mel)
    input_ids = torch.Tensor([[config["decoder_start_token_id"]]]).to(dtype=torch.int32).cuda()
    return greedy_search(model=whisperdecoder, encoder_outputs=encoder_outputs, input_ids=input_ids,
                         logits_processor=get_logits_processor(config, input_ids.shape[-1], return_timestamps),
                         stopping_criteria=get_stopping_criteria(config),
                         pad_token_id=config["pad_token_id"], eos_token_id=config["eos_token_id"])


if __name__ == "__main__":
    args = parse_arguments()
    tensorrt_llm.logger.set_level(args.log_level)
    rank, world, device, dist = tensorrt_llm.sharding.init_from_env(args.dist_backend)
    torch.cuda.set_device(device)
    if world > 1 and (args.session or args.compare):
        raise SystemExit("the Session path is the reference's batch-1 single-GPU protocol: run --session / --compare without torchrun")
    with open(os.path.join(args.engine_dir, "config.pkl"), "rb") as f:
        config = pickle.load(f)
    if args.max_length:
        config["max_length"] = args.max_length
    name = config.get("name", "whisper-tiny.en")
    lang_name = {v: k for k, v in (config.get("lang_to_id") or {}).items()}
    show_lang = lambda tok, p: f"language {lang_name.get(tok, tok)}" + ("" if p is None else f"  probability {p:.4f}")
    if args.long_form:
        if world > 1:
            raise SystemExit("--long_form runs on one rank")
        window = 2 * config["max_source_positions"]
        if args.audio:
            from get_LibriSpeech import read_audio
            audios = [torch.from_numpy(read_audio(path)).float().cuda() for path in args.audio]
            names = [os.path.basename(path) for path in args.audio]
        else:   # noise recordings of 2.5 windows
            gen = torch.Generator().manual_seed(args.synthetic_start)
            audios = [(torch.randn(window * tensorrt_llm.audio.HOP * 5 // 2, generator=gen) * 0.1).cuda() for _ in range(args.synthetic)]
            names = [f"recording {i}" for i in range(args.synthetic)]
        enc = tensorrt_llm.WhisperEncoderEngine(open(os.path.join(args.engine_dir, "WhisperEncoder.engine"), "rb").read())
        dec = tensorrt_llm.WhisperDecoderEngine(open(os.path.join(args.engine_dir, "WhisperDecoder.engine"), "rb").read(), config)
        frontend = tensorrt_llm.audio.LogMelFrontend(n_frames=window)
        tok = tensorrt_llm.text.WhisperTokenDecoder.from_dir(args.whisper) if os.path.isdir(args.whisper) else None
        for _ in range(2):  # the first pass is the warm-up, as in run.py:260
            torch.cuda.synchronize()
            t0 = time.time()
            files = tensorrt_llm.runtime.transcribe_long(enc, dec, frontend, audios, condition_on_previous_text=not args.no_condition_on_previous_text,
                                                         no_speech_token_id=args.no_speech_token_id, max_rows=args.max_rows, seed=args.seed,
                                                         **({"language": args.language} if args.language is not None else {}),
                                                         **({"task": args.task} if args.task is not None else {}),
                                                         **({"text_of": lambda ids: tok.decode(ids, skip_special_tokens=True)} if tok else {}))
            torch.cuda.synchronize()
            elapsed = time.time() - t0
        file_langs = [None] * len(audios)
        if args.language is not None:        # (segments per file, dict(language, language_prob) per file)
            files, file_langs = files
        seconds = sum(a.numel() for a in audios) / tensorrt_llm.audio.SAMPLING_RATE
        print(f"long form   : {elapsed:.3f} s for {seconds:.1f} s of audio in {len(audios)} file(s)  ({seconds / elapsed:.1f} audio-s/s)")
        tb = tensorrt_llm.runtime.timestamp_rules(config)[1]
        for fname, segments, lang in zip(names, files, file_langs):
            print(f"{fname}:" + (f"  {show_lang(lang['language'], lang['language_prob'])}" if lang else ""))
            for seg in segments:
                if tok:
                    text = tok.decode_with_timestamps(seg["ids"])
                else:
                    text = " ".join(str(t) for t in seg["ids"] if t < tb)
                print(f"  [{seg['start']:7.2f} --> {seg['end']:7.2f}] {text}")
        if args.dump_ids:
            import json
            json.dump([[dict(start=s["start"], end=s["end"], ids=s["ids"], temperature=s["temperature"], seek=s["seek"]) for s in segs] for segs in files],
                      open(args.dump_ids, "w"))
        raise SystemExit(0)
    if args.audio:
        import numpy as np
        from get_LibriSpeech import N_SAMPLES, read_audio
        frontend = tensorrt_llm.audio.LogMelFrontend()
        wav = np.zeros((len(args.audio), N_SAMPLES), dtype=np.float32)
        for j, path in enumerate(args.audio):
            a = read_audio(path)[:N_SAMPLES]
            wav[j, :len(a)] = a
        mels = list(frontend(torch.from_numpy(wav).cuda()).split(1))
    else:
        mels = [torch.from_numpy(tensorrt_llm.synthetic.make_mel(config, index=args.synthetic_start + i, batch=1)).cuda() for i in range(args.synthetic)]
    results = {}
    if not args.session:
        pipe = tensorrt_llm.WhisperPipeline(open(os.path.join(args.engine_dir, "WhisperEncoder.engine"), "rb").read(),
                                            open(os.path.join(args.engine_dir, "WhisperDecoder.engine"), "rb").read(), config, workers=max(1, args.workers))
        begin, end = tensorrt_llm.sharding.utterance_shard(len(mels), world, rank)       # this rank's contiguous shard
        per_batch = 8 if args.num_beams <= 1 else max(1, min(8, 16 // args.num_beams))   # rows = utterances x beams <= 16
        if args.batching == "continuous":
            groups = None
        elif args.batching == "sorted":
            lengths = [tensorrt_llm.audio.valid_frames(m)[0] for m in mels]
            groups = tensorrt_llm.sharding.length_sorted_batches(lengths, per_batch, world, rank)
        else:
            begin, end = tensorrt_llm.sharding.utterance_shard(len(mels), world, rank)   # this rank's contiguous shard
            groups = [list(range(b0, b1)) for b0, b1 in tensorrt_llm.sharding.batches(begin, end, per_batch)]
        if args.detect_language:
            if rank == 0:
                dec = pipe.engines[0][1]
                enc = pipe.engines[0][0]
                for g in groups:
                    toks, probs = dec.detect_language(enc(torch.cat([mels[i] for i in g])))
                    for i, t, p in zip(g, toks.cpu().tolist(), probs.max(1).values.cpu().tolist()):
                        print(f"utterance {i}: {show_lang(t, p)}")
            raise SystemExit(0)
        for _ in range(2):  # the first pass is the warm-up, as in run.py:260
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.time()
            indexed, score_rows, lang_rows = [], [], []
            if groups is None:
                rows = pipe.transcribe_continuous(torch.cat(mels[begin:end]), slots=8, chunk=8) if end > begin else []
                indexed = list(zip(range(begin, end), [r.tolist() for r in rows]))
            else:
                kw = [{"return_timestamps": True}] * len(groups) if args.return_timestamps else None
                if args.return_token_timestamps:
                    one = {"return_token_timestamps": True, "alignment_heads": args.alignment_heads, "return_timestamps": args.return_timestamps,
                           "median_filter_width": args.median_filter_width or int(config.get("median_filter_width", 7))}
                    kw = [one] * len(groups)
                if args.return_logprobs:
                    lp = {"return_logprobs": True, "no_speech_token_id": args.no_speech_token_id}
                    kw = [dict(k, **lp) for k in (kw or [{}] * len(groups))]
                if args.temperature > 0:             # utterance i draws with seed + i, whichever batch it lands in
                    kw = [dict(k, temperature=args.temperature, seeds=[args.seed + i for i in g]) for k, g in zip(kw, groups)]
                if args.temperature_fallback:
                    kw = [{"return_timestamps": args.return_timestamps, "no_speech_token_id": args.no_speech_token_id,
                           "temperature_fallback": {"seeds": [args.seed + i for i in g]}} for g in groups]
                if args.prompt_ids is not None:      # generate / generate_with_fallback(prompt_ids=...): one prompt for every utterance
                    kw = [dict(k, prompt_ids=args.prompt_ids) for k in (kw or [{}] * len(groups))]
                if args.num_beams > 1:
                    kw = [{"num_beams": args.num_beams, "length_penalty": args.length_penalty, "early_stopping": args.early_stopping}] * len(groups)
                lt = dict(**({"language": args.language} if args.language is not None else {}), **({"task": args.task} if args.task is not None else {}))
                if lt:
                    kw = [dict(k, **lt) for k in (kw or [{}] * len(groups))]
                for g, ids in zip(groups, pipe.transcribe([torch.cat([mels[i] for i in g]) for g in groups], kw)):
                    used = [args.temperature] * len(g)
                    if args.language is not None:        # the result's last element: DecodeLanguages of the batch
                        langs, ids = ids[-1], (ids[:-1] if len(ids) > 2 else ids[0])
                        lang_rows += list(zip(g, zip(langs.ids.cpu().tolist(), langs.prob_of_ids().cpu().tolist())))
                    if args.temperature_fallback:        # (ids, DecodeScores, temperature used per row)
                        used = ids[2].cpu().tolist()
                        ids = ids[:2]
                    if args.return_logprobs:             # (ids, [seconds per token,] DecodeScores) of the batch
                        sc = ids[-1]
                        nsp = sc.no_speech_prob.cpu().tolist() if sc.no_speech_prob is not None else [None] * len(g)
                        score_rows += list(zip(g, zip(sc.token_logprobs.cpu().tolist(), sc.avg_logprob.cpu().tolist(), nsp, used)))
                        ids = ids[:-1] if args.return_token_timestamps else ids[0]
                    if args.return_token_timestamps:     # (ids, seconds per token) of the batch
                        indexed += list(zip(g, zip(ids[0].cpu().tolist(), ids[1].cpu().tolist())))
                    else:
                        indexed += list(zip(g, ids.cpu().tolist()))
            torch.cuda.synchronize()
            elapsed = tensorrt_llm.sharding.max_over_ranks(time.time() - t0, dist)
            ids = [row for _, row in sorted(tensorrt_llm.sharding.gather_objects(indexed, dist))]   # dataset order, on the host
            if args.return_token_timestamps:
                results["token_timestamps"] = [row[1] for row in ids]
                ids = [row[0] for row in ids]
            results["fast"] = (elapsed, ids)
            if args.return_logprobs:
                results["scores"] = [row for _, row in sorted(tensorrt_llm.sharding.gather_objects(score_rows, dist))]
            if args.language is not None:
                results["languages"] = [row for _, row in sorted(tensorrt_llm.sharding.gather_objects(lang_rows, dist))]
        if rank == 0:
            print(f"fast path   : {results['fast'][0]:.3f} s for {len(mels)} x 30 s on {world} rank(s)  ({30 * len(mels) / results['fast'][0]:.1f} audio-s/s)")
            if args.dump_ids:
                import json
                json.dump(results["fast"][1], open(args.dump_ids, "w"))
    if args.session or args.compare:
        whisperencoder, whisperdecoder = WhisperEncoder(args, config), WhisperDecoder(args, config)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.time()
            ids = [decode_with_sessions(whisperencoder, whisperdecoder, config, m, args.return_timestamps)[0].cpu().tolist() for m in mels]
            torch.cuda.synchronize()
            results["session"] = (time.time() - t0, ids)
        print(f"Session path: {results['session'][0]:.3f} s for {len(mels)} x 30 s  ({30 * len(mels) / results['session'][0]:.1f} audio-s/s)")
    if args.compare:
        eos, pad = config["eos_token_id"], config["pad_token_id"]
        a = [trim_after_eos(r, eos, pad) for r in results["fast"][1]]
        b = [trim_after_eos(r, eos, pad) for r in results["session"][1]]
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        print(f"Compare Result: same [{len(a) - len(diff)}], diff [{len(diff)}]")
    token_times = results.pop("token_timestamps", None)
    scores = results.pop("scores", None)
    languages = results.pop("languages", None)
    if rank == 0 and languages is not None:
        for i, (t, p) in enumerate(languages):
            print(f"utterance {i}: {show_lang(t, p if args.language == 'auto' else None)}")
    if rank == 0:
        for key in results:
            print(key, "ids[0][:16] =", results[key][1][0][:16])
    if rank == 0 and args.audio and os.path.isdir(args.whisper):   # batch_decode(predicted_ids, skip_special_tokens=True) of run.py:287
        tok = tensorrt_llm.text.WhisperTokenDecoder.from_dir(args.whisper)
        for path, ids in zip(args.audio, next(iter(results.values()))[1]):
            print(f"{os.path.basename(path)}: {tok.decode(ids, skip_special_tokens=True)!r}")
            if args.return_timestamps:
                for seg in tok.offsets(ids):
                    print(f"  [{seg['timestamp'][0]:6.2f} --> {seg['timestamp'][1]:6.2f}] {seg['text']}")
            if token_times is not None:
                word_lp = [None] * len(ids)
                if scores is not None:      # each word's mean token log-probability
                    lps = scores[args.audio.index(path)][0]
                    word_lp = [sum(lps[k] for k in idx) / len(idx) for idx in tok.combine_tokens_into_words([int(i) for i in ids])[2]]
                for w, lp in zip(tok.words(ids, token_times[args.audio.index(path)]), word_lp):
                    print(f"  [{w['timestamp'][0]:6.2f} --> {w['timestamp'][1]:6.2f}] {w['text']!r}" + (f"  logprob {lp:.3f}" if lp is not None else ""))
    elif rank == 0 and token_times is not None:      # no tokenizer: every token as its own word
        eos, pad = config["eos_token_id"], config["pad_token_id"]
        for i, (ids, ts) in enumerate(list(zip(results["fast"][1], token_times))[:4]):
            n = len(trim_after_eos(ids, eos, pad))
            ends = list(ts[1:]) + [ts[-1]]
            print(f"utterance {i} token times:", " ".join(f"{t}[{a:.2f}-->{b:.2f}]" for t, a, b in zip(ids[:n], ts[:n], ends[:n])))
    elif rank == 0 and args.return_timestamps:       # no tokenizer: ids with the timestamps written out
        tb = tensorrt_llm.runtime.timestamp_rules(config)[1]
        for i, ids in enumerate(next(iter(results.values()))[1][:4]):
            print(f"utterance {i}:", " ".join(f"<|{(t - tb) * 0.02:.2f}|>" if t >= tb else str(t) for t in ids))
    if rank == 0 and scores is not None:             # confidence per utterance (openai-whisper's segment fields)
        tok = tensorrt_llm.text.WhisperTokenDecoder.from_dir(args.whisper) if os.path.isdir(args.whisper) else None
        eos, pad = config["eos_token_id"], config["pad_token_id"]
        sampled = args.temperature > 0 or args.temperature_fallback
        for i, (ids, (_lps, avg, nsp, used)) in enumerate(zip(results["fast"][1], scores)):
            # without a tokenizer the ratio is taken over the ids written out: repetition still shows
            text = tok.decode(ids, skip_special_tokens=True) if tok else " ".join(str(t) for t in trim_after_eos(ids, eos, pad))
            ratio = tensorrt_llm.text.compression_ratio(text) if text else 0.0
            print(f"utterance {i}: avg_logprob {avg:.6f}  no_speech_prob {'n/a' if nsp is None else format(nsp, '.6f')}  compression_ratio {ratio:.3f}"
                  + (f"  temperature {used:.1f}" if sampled else ""))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
