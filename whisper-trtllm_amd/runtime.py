"""Runtime boundary: `Session` / `TensorInfo` with the reference's surface (tensorrt_llm/runtime/session.py:28-207),
plus the batched resident-KV fast path (`WhisperEncoderEngine`, `WhisperDecoderEngine`) behind the same C-ABI.
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

from . import _dtypes as trt
from . import _lib
from .logger import logger


def under_rocprof() -> bool:
    """True when rocprofv3's tool library is loaded into this process (it is LD_PRELOADed by the `rocprofv3` launcher and intercepts every
    HIP / HSA call, incl. the AQL packets of a hipGraph replay).  A 4-worker `WhisperPipeline` run under `rocprofv3 --kernel-trace`
    aborted with SIGSEGV in round 3: the faulting frame lies in a module mapped at process start (where the preloaded profiler
    libraries live), below hipGraphLaunch <- enqueue_steps <- wt_decoder_run of a worker thread; the frames could not be symbolised
    (DESIGN.md "The four-worker abort under rocprofv3").  The same runs without the profiler are clean (soak, test suite, driver bench),
    so the hazard is several host threads replaying graphs at once UNDER THE PROFILER -- `WhisperPipeline` therefore runs one worker then."""
    import os
    env = os.environ
    if "rocprofiler" in env.get("LD_PRELOAD", "") or env.get("ROCP_TOOL_LIBRARIES") or any(k.startswith("ROCPROF_") for k in env):
        return True
    try:
        with open("/proc/self/maps") as f:
            return any("rocprofiler-sdk-tool" in line for line in f)
    except OSError:
        return False


@contextlib.contextmanager
def _scoped_stream():
    """Current torch stream handle; synchronised when the scope ends (session.py:14-25)."""
    import torch
    stream = torch.cuda.current_stream()
    try:
        yield stream.cuda_stream
    finally:
        stream.synchronize()


@dataclass
class TensorInfo:
    name: str
    dtype: trt.DataType
    shape: tuple


def _desc(info: TensorInfo) -> _lib.TensorDesc:
    d = _lib.TensorDesc()
    d.name = info.name.encode()
    d.dtype = info.dtype.code
    shape = tuple(int(s) for s in info.shape)
    if len(shape) > _lib.WT_MAX_DIMS:
        raise ValueError(f"{info.name}: rank {len(shape)} too large")
    d.ndim = len(shape)
    for i, s in enumerate(shape):
        d.shape[i] = s
    return d


class Session:
    """`Session.from_serialized_engine(bytes)` -> `infer_shapes` -> `run` (async) like session.py:36-178."""

    def __init__(self, **kwargs):
        self._handle = None
        self._lib = None

    def _init(self, engine_buffer, device: Optional[int] = None):
        import torch
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("whisper-trtllm_amd needs a ROCm GPU (MI355X); there is no CPU execution path")
        dev = torch.cuda.current_device() if device is None else device
        buf = bytes(engine_buffer)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.wt_engine_open(buf, len(buf), dev, ctypes.byref(handle)), "wt_engine_open")
        self._handle = handle
        info = _lib.EngineInfo()
        _lib.check(self._lib.wt_engine_get_info(self._handle, ctypes.byref(info)), "wt_engine_get_info")
        self.info = info
        return self

    @staticmethod
    def from_serialized_engine(engine, device: Optional[int] = None) -> "Session":
        return Session()._init(engine, device)

    def clone(self) -> "Session":
        """A second execution context on the same weights (wt_engine_clone): own workspace / caches / graphs, shared read-only payload."""
        other = Session()
        other._lib = self._lib
        handle = ctypes.c_void_p()
        _lib.check(self._lib.wt_engine_clone(self._handle, ctypes.byref(handle)), "wt_engine_clone")
        other._handle = handle
        other.info = self.info
        return other

    def __del__(self):
        try:
            if self._handle is not None and self._lib is not None:
                self._lib.wt_engine_close(self._handle)
                self._handle = None
        except Exception:
            pass

    @property
    def handle(self):
        return self._handle

    def infer_shapes(self, inputs: List[TensorInfo], context=None) -> Optional[List[TensorInfo]]:
        """Returns the output TensorInfos, or None (after logging) on a name/dtype/shape mismatch — session.py:131-136."""
        n = len(inputs)
        arr = (_lib.TensorDesc * max(n, 1))(*[_desc(i) for i in inputs])
        out = (_lib.TensorDesc * 8)()
        n_out = ctypes.c_int(8)
        rc = self._lib.wt_engine_infer_shapes(self._handle, arr, n, out, ctypes.byref(n_out))
        if rc != 0:
            logger.error(_lib.last_error())
            return None
        return [TensorInfo(out[i].name.decode(), trt.from_code(out[i].dtype), tuple(out[i].shape[k] for k in range(out[i].ndim)))
                for i in range(n_out.value)]

    def run(self, inputs: Dict[str, Any], outputs: Dict[str, Any], stream, context=None) -> bool:
        """Enqueue on `stream` (raw hipStream_t handle as int).  True means enqueued, not finished (session.py:159-160)."""
        def bind(d):
            arr = (_lib.Binding * max(len(d), 1))()
            keep = []
            for i, (name, t) in enumerate(d.items()):
                ptr = t.data_ptr() if hasattr(t, "data_ptr") else int(t)
                nm = name.encode()
                keep.append(nm)
                arr[i].name, arr[i].ptr = nm, ptr
            return arr, keep
        a_in, k1 = bind(inputs)
        a_out, k2 = bind(outputs)
        rc = self._lib.wt_engine_run(self._handle, a_in, len(inputs), a_out, len(outputs), ctypes.c_void_p(stream or 0))
        if rc != 0:
            logger.error(_lib.last_error())
            return False
        return True

    def _debug_run(self, inputs: Dict[str, "torch.Tensor"], context=None) -> Dict[str, "torch.Tensor"]:
        """Synchronous convenience run with freshly allocated outputs (session.py:180-207)."""
        import torch
        infos = [TensorInfo(n, trt.from_torch(t.dtype), tuple(t.shape)) for n, t in inputs.items()]
        outs = self.infer_shapes(infos)
        if outs is None:
            raise RuntimeError(_lib.last_error())
        outputs = {o.name: torch.empty(tuple(o.shape), dtype=trt.torch_dtype(o.dtype), device="cuda") for o in outs}
        with _scoped_stream() as stream:
            if not self.run(inputs, outputs, stream):
                raise RuntimeError(_lib.last_error())
        return outputs


# ----------------------------------------------------------------------------------------------- batched fast path
class WhisperEncoderEngine:
    """mel f32 [B, n_mels, 2*S] on the GPU -> hidden f32 [B, S, d]; asynchronous on the current torch stream."""

    def __init__(self, engine_buffer, device: Optional[int] = None, _session: Optional[Session] = None):
        self.session = _session if _session is not None else Session.from_serialized_engine(engine_buffer, device)
        if self.session.info.kind != 1:
            raise ValueError("not a WhisperEncoder engine")

    def clone(self) -> "WhisperEncoderEngine":
        """Another engine on the same device weights (own workspace): for a second host thread / stream."""
        return WhisperEncoderEngine(None, _session=self.session.clone())

    def __call__(self, mel):
        import torch
        i = self.session.info
        if mel.dtype != torch.float32 or mel.dim() != 3 or mel.shape[1] != i.n_mels or mel.shape[2] != 2 * i.max_source_positions:
            raise ValueError(f"mel must be float32 [B,{i.n_mels},{2 * i.max_source_positions}], got {tuple(mel.shape)} {mel.dtype}")
        if not mel.is_cuda:   # the C-ABI takes DEVICE pointers: a host pointer would fault on the GPU
            raise ValueError("mel must be a CUDA (ROCm) tensor: move it to the GPU first (there is no CPU execution path)")
        mel = mel.contiguous()
        out = torch.empty(mel.shape[0], i.max_source_positions, i.d_model, dtype=torch.float32, device=mel.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_encoder_forward(self.session.handle, mel.data_ptr(), mel.shape[0], out.data_ptr(),
                                                         ctypes.c_void_p(stream)), "wt_encoder_forward")
        return out


def _i32_array(values: Sequence[int]):
    vals = [int(v) for v in values]
    return (ctypes.c_int32 * max(len(vals), 1))(*vals), len(vals)


def timestamp_rules(config: dict):
    """Timestamp mode of a config (WhisperTimeStampLogitsProcessor's constants, logits_process.py:1350-1357): returns
    (no_timestamps_token_id, timestamp_begin, ts_begin_index, max_initial_timestamp_index, forced list without <|notimestamps|>).
    `ts_begin_index` is what the reference computes from the model's own forced list (.en: [[1, no_ts]] -> 2).  Raises ValueError for a
    forced list the timestamp rule would fight with: a forced position >= ts_begin_index - 1 (the forced <|0.00|> step or later)."""
    forced = [list(x) for x in (config.get("forced_decoder_ids") or [])]
    no_ts = config.get("no_timestamps_token_id")
    if no_ts is None:
        if not forced:
            raise ValueError("timestamp mode needs no_timestamps_token_id (or forced_decoder_ids ending in <|notimestamps|>)")
        no_ts = forced[-1][1]
    ts_begin = len(forced) + 2 - (1 if forced and forced[-1][1] == no_ts else 0)
    kept = [pair for pair in forced if pair[1] != no_ts]
    bad = [pair for pair in kept if pair[0] >= ts_begin - 1]
    if bad:
        raise ValueError(f"timestamp mode: forced ids {bad} at or after the forced <|0.00|> position {ts_begin - 1}")
    max_init = config.get("max_initial_timestamp_index", 1)
    return int(no_ts), int(no_ts) + 1, ts_begin, -1 if max_init is None else int(max_init), kept


def _check_beam_args(num_beams, return_timestamps, logits_trace, force_eos_step, force_eos_steps):
    """The combinations the engine refuses (wt_decoder_begin: WT_E_UNSUPPORTED), refused before anything is enqueued."""
    if not isinstance(num_beams, int) or num_beams < 1 or num_beams > 8:
        raise ValueError(f"num_beams must be an integer in [1, 8], got {num_beams!r}")
    if num_beams > 1 and return_timestamps:
        raise ValueError("beam search and timestamp mode cannot be combined (num_beams > 1 with return_timestamps=True)")
    if num_beams > 1 and (logits_trace is not None or force_eos_step is not None or force_eos_steps is not None):
        raise ValueError("beam search does not take logits_trace / force_eos_step(s)")


def prompt_rows(prompt_ids, batch: int, max_target_positions: int):
    """The decoder prompt of a batch as the engine takes it (wt_decoder_set_prompt): `prompt_ids` is a 1-D sequence shared by the batch or a
    2-D [batch, n] sequence with per-row contents of equal length; the first entry is <|startofprev|>.  The text part is cut to its last
    max_target_positions // 2 - 1 tokens, as openai-whisper's _get_initial_tokens does.  Returns a list of 1 or `batch` rows."""
    if hasattr(prompt_ids, "tolist"):
        prompt_ids = prompt_ids.tolist()
    rows = list(prompt_ids)
    if not rows:
        raise ValueError("prompt_ids is empty (pass None for no prompt)")
    if not isinstance(rows[0], (list, tuple)):
        rows = [rows]
    rows = [[int(t) for t in r] for r in rows]
    n = len(rows[0])
    if n < 1 or any(len(r) != n for r in rows):
        raise ValueError("prompt_ids rows must have one length >= 1 (per-row prompt lengths are not supported)")
    if len(rows) != 1 and len(rows) != batch:
        raise ValueError(f"prompt_ids has {len(rows)} rows for a batch of {batch} (one shared row, or one per utterance)")
    keep = max_target_positions // 2 - 1
    return [r[:1] + r[1:][-keep:] for r in rows]


def ragged_prompt_rows(prompts, batch: int, max_target_positions: int):
    """Per-utterance decoder prompts as the engine takes them (wt_decoder_set_prompt_rows): `prompts` holds one sequence per utterance, each
    empty (no prompt for that row) or starting with <|startofprev|>; the text part of each is cut to its last max_target_positions // 2 - 1
    tokens.  Returns `batch` lists of unequal lengths."""
    if hasattr(prompts, "tolist"):
        prompts = prompts.tolist()
    rows = [r.tolist() if hasattr(r, "tolist") else list(r) for r in prompts]
    if len(rows) != batch:
        raise ValueError(f"prompts has {len(rows)} rows for a batch of {batch} (one sequence per utterance, empty for none)")
    keep = max_target_positions // 2 - 1
    return [[int(t) for t in r[:1] + r[1:][-keep:]] for r in rows]


def strip_prompts(ids, prompt_len: int, eos_token_id=None):
    """The rows of a decode behind decoder prompts (`prompt_ids`, or `prompts` whose rows are left-padded to the longest) without the pad
    and the prompt: per row the list of ids from the start token on, cut behind the row's first EOS when `eos_token_id` is given."""
    out = []
    for row in (ids.tolist() if hasattr(ids, "tolist") else ids):
        row = [int(t) for t in row[prompt_len:]]
        if eos_token_id is not None and eos_token_id in row[1:]:
            row = row[:row.index(eos_token_id, 1) + 1]
        out.append(row)
    return out


def _check_prompt_args(rows, vocab_size, max_length, num_beams, return_token_timestamps, half_engine):
    """What the engine refuses (wt_decoder_set_prompt / wt_decoder_set_prompt_rows / wt_decoder_begin: WT_E_INVALID, WT_E_UNSUPPORTED), refused
    before anything is enqueued.  `rows` may be of unequal lengths (`prompts`): the longest counts."""
    if half_engine:
        raise ValueError("prompt_ids needs an fp32 decoder engine (the prefill is fp32)")
    if num_beams > 1:
        raise ValueError("prompt_ids and beam search cannot be combined")
    if return_token_timestamps:
        raise ValueError("prompt_ids and return_token_timestamps cannot be combined")
    bad = [t for r in rows for t in r if not 0 <= t < vocab_size]
    if bad:
        raise ValueError(f"prompt_ids holds ids outside the vocabulary [0, {vocab_size}): {bad[:4]}")
    longest = max(len(r) for r in rows)
    if longest + 2 > max_length:
        raise ValueError(f"a prompt of {longest} tokens, the start token and one generated token exceed max_length {max_length}")


def language_ids_of(config: dict):
    """The language token ids of a config: `language_ids` (synthetic models), else the values of `lang_to_id` (generation_config.json, which
    examples/whisper/_common.py copies into the config), in ascending order.  [] when the config names none."""
    ids = config.get("language_ids")
    if ids is None and isinstance(config.get("lang_to_id"), dict):
        ids = sorted(config["lang_to_id"].values())
    return [int(t) for t in (ids or [])]


def resolve_languages(config: dict, language, batch: int):
    """`language=` of generate / begin as the engine takes it (wt_decoder_set_languages): returns (language_ids, rows) with rows[b] the
    language token id of utterance b, or -1 where it is to be detected.  `language`: "auto", an id, a code ("en") or token ("<|en|>")
    looked up in the config's `lang_to_id`, or a list of `batch` of those.  Raises ValueError for a config without language ids or
    without a language slot at forced position 1 (a `.en` checkpoint), for a name without a map, and for an id that is not listed."""
    ids = language_ids_of(config)
    if not ids:
        raise ValueError("language= needs the config's language ids (`language_ids`, or generation_config.json's `lang_to_id`)")
    if len(ids) > 128 or len(set(ids)) != len(ids):
        raise ValueError(f"language ids must be at most 128 distinct ids, got {len(ids)}")
    forced = config.get("forced_decoder_ids") or []
    if not forced or forced[0][0] != 1 or forced[0][1] not in ids:
        raise ValueError("language= needs a forced_decoder_ids list whose position 1 is a language token (a multilingual checkpoint)")
    entries = list(language) if isinstance(language, (list, tuple)) else [language] * batch
    if len(entries) != batch:
        raise ValueError(f"language has {len(entries)} entries for a batch of {batch} (one for all, or one per utterance)")
    rows = []
    for entry in entries:
        if hasattr(entry, "item"):
            entry = entry.item()
        if entry is None or entry == "auto":
            rows.append(-1)
            continue
        if isinstance(entry, str):
            names = config.get("lang_to_id")
            if not isinstance(names, dict):
                raise ValueError(f"language {entry!r}: the config has no `lang_to_id` map (pass a token id)")
            key = entry if entry.startswith("<|") else f"<|{entry}|>"
            if key not in names:
                raise ValueError(f"language {entry!r} is not in the config's `lang_to_id`")
            entry = names[key]
        if isinstance(entry, bool) or not isinstance(entry, int) or entry not in ids:
            raise ValueError(f"language token {entry!r} is not one of the config's language ids")
        rows.append(int(entry))
    return ids, rows


def resolve_task(config: dict, task):
    """`task=` as a token id: "transcribe" / "translate" through the config's `task_to_id`, or an id (synthetic models)."""
    if isinstance(task, str):
        names = config.get("task_to_id")
        if not isinstance(names, dict):
            raise ValueError(f"task {task!r}: the config has no `task_to_id` map (pass a token id)")
        if task not in names:
            raise ValueError(f"task {task!r} is not in the config's `task_to_id` ({sorted(names)})")
        task = names[task]
    if isinstance(task, bool) or not isinstance(task, int) or not 0 <= task < config["vocab_size"]:
        raise ValueError(f"task must be a name of `task_to_id` or a token id, got {task!r}")
    if not any(pos == 2 for pos, _tok in (config.get("forced_decoder_ids") or [])):
        raise ValueError("task= needs a forced_decoder_ids list with a task token at position 2 (a multilingual checkpoint)")
    return int(task)


class DecodeLanguages:
    """The languages of a decode (generate(..., language=...)): `ids` int32 [B] on the GPU, every row's language token (the caller's, or
    the detected one); `probs` float32 [B, n_lang]: softmax of the first step's logits over `language_ids`, in their order (all 0 when
    no row was left to detect); `language_ids`: the config's list."""

    def __init__(self, ids, probs, language_ids):
        self.ids, self.probs, self.language_ids = ids, probs, list(language_ids)

    def prob_of_ids(self):
        """float32 [B]: the probability of every row's own language."""
        import torch
        table = torch.as_tensor(self.language_ids, device=self.ids.device)
        col = (self.ids.long()[:, None] == table[None, :]).int().argmax(1)
        return self.probs.gather(1, col[:, None])[:, 0]


class DecodeScores:
    """Confidence signals of a greedy decode (generate(..., return_logprobs=True)), openai-whisper's definitions:
    `token_logprobs` float32 [B, len]: log-probability of every emitted token under the step's processed scores (0 at position 0, at
    forced positions and behind a row's EOS); `sum_logprob` float32 [B]: the row's sum through its EOS; `avg_logprob` float32 [B] =
    sum_logprob / scored positions (generated tokens including the EOS and forced ones; a row without EOS: all len - 1 of them);
    `no_speech_prob` float32 [B] or None: softmax(raw logits of the first step)[no_speech_token_id].
    `prompt_len`: tokens of a decoder prompt in front of the start token; they are not scored (their entries are 0)."""

    def __init__(self, ids, token_logprobs, sum_logprob, no_speech_prob, eos_token_id: int, prompt_len: int = 0):
        import torch
        self.token_logprobs, self.sum_logprob, self.no_speech_prob = token_logprobs, sum_logprob, no_speech_prob
        self.prompt_len = prompt_len
        body = ids[:, prompt_len + 1:]
        is_eos = body == eos_token_id
        width = torch.full((body.shape[0],), body.shape[1], dtype=torch.int64, device=body.device)
        self.n_scored = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, width)
        self.avg_logprob = sum_logprob / self.n_scored.clamp(min=1).to(sum_logprob.dtype)


def _check_language_args(config, language, batch, num_beams, return_token_timestamps):
    """What the engine refuses of `language=` (wt_decoder_begin: WT_E_INVALID, WT_E_UNSUPPORTED), refused before anything is enqueued.
    Returns (language_ids, rows) as `resolve_languages`, or (None, None) when the mode is off."""
    if language is None:
        return None, None
    if num_beams > 1:
        raise ValueError("language= and beam search cannot be combined")
    if return_token_timestamps:
        raise ValueError("language= and return_token_timestamps cannot be combined")
    return resolve_languages(config, language, batch)


def _check_logprob_args(return_logprobs, no_speech_token_id, num_beams, vocab_size):
    """What the engine refuses (wt_decoder_begin: WT_E_UNSUPPORTED, wt_decoder_set_logprobs: WT_E_INVALID), refused before anything is enqueued."""
    if not return_logprobs:
        if no_speech_token_id is not None:
            raise ValueError("no_speech_token_id needs return_logprobs=True")
        return
    if num_beams > 1:
        raise ValueError("beam search and return_logprobs cannot be combined (return_scores gives the beams' sequence score)")
    if no_speech_token_id is not None and not (isinstance(no_speech_token_id, int) and 0 <= no_speech_token_id < vocab_size):
        raise ValueError(f"no_speech_token_id must be an id in [0, {vocab_size}), got {no_speech_token_id!r}")


def _check_sampling_args(temperature, seed, seeds, batch, num_beams):
    """What the engine refuses (wt_decoder_set_sampling / wt_decoder_begin: WT_E_INVALID, WT_E_UNSUPPORTED), refused before anything is
    enqueued.  Returns the row seeds of a sampled decode ([] when sampling is off)."""
    import math
    if not isinstance(temperature, (int, float)) or not math.isfinite(temperature):
        raise ValueError(f"temperature must be a finite number, got {temperature!r}")
    if temperature <= 0:
        return []
    if num_beams > 1:
        raise ValueError("beam search and temperature sampling cannot be combined")
    batch = int(batch.shape[0]) if hasattr(batch, "shape") else int(batch)      # (the encoder memory itself: looked at only when sampling)
    if seeds is None:
        seeds = [int(seed) + b for b in range(batch)]
    seeds = [int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds]
    if len(seeds) < batch:
        raise ValueError(f"seeds needs one entry per utterance ({batch}), got {len(seeds)}")
    return seeds[:batch]


def _default_text_of(config):
    """ids -> text for the compression ratio of generate_with_fallback: the config's token decoder when it carries a vocabulary
    (`vocab` [+ `added_tokens`], or `tokenizer_dir` with a vocab.json), else the ids in decimal joined by spaces (synthetic models)."""
    import os
    from .text import WhisperTokenDecoder
    tok = None
    if isinstance(config.get("vocab"), dict):
        tok = WhisperTokenDecoder(config["vocab"], config.get("added_tokens"))
    elif config.get("tokenizer_dir") and os.path.exists(os.path.join(config["tokenizer_dir"], "vocab.json")):
        tok = WhisperTokenDecoder.from_dir(config["tokenizer_dir"])
    if tok is not None:
        return lambda ids: tok.decode(ids, skip_special_tokens=True)
    return lambda ids: " ".join(str(int(t)) for t in ids)


def _check_token_timestamp_args(config, info, return_token_timestamps, alignment_heads, median_filter_width, num_beams):
    """Token-level timestamps: the head list to use ([] when the mode is off).  `alignment_heads` of the call wins over the config's
    (generation_config.json's `alignment_heads`, which examples/whisper/_common.py copies into the config).  Refused before anything is
    enqueued: no heads, heads outside the model, more than 32, a listed-twice head, an even or out-of-range width, beam search."""
    if not return_token_timestamps:
        return []
    heads = alignment_heads if alignment_heads is not None else config.get("alignment_heads")
    if not heads:
        raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available. "
                         "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this property to the generation config.")
    if num_beams > 1:
        raise ValueError("beam search and token-level timestamps cannot be combined (they would need beam_indices, which the engine does not keep)")
    heads = [(int(l), int(h)) for l, h in heads]
    if len(heads) > 32:
        raise ValueError(f"at most 32 alignment heads, got {len(heads)}")
    for l, h in heads:
        if not (0 <= l < info.n_layers and 0 <= h < info.n_heads):
            raise ValueError(f"alignment head ({l}, {h}) outside {info.n_layers} layers x {info.n_heads} heads")
    if len(set(heads)) != len(heads):
        raise ValueError("an alignment head is listed twice")
    if not isinstance(median_filter_width, int) or median_filter_width < 1 or median_filter_width > 15 or median_filter_width % 2 != 1:
        raise ValueError(f"`median_filter_width` should be an odd number in [1, 15], got {median_filter_width!r}")
    return heads


class WhisperDecoderEngine:
    """Greedy decode with the KV cache resident on the device (no per-token host round trip).

    `config` is the HF config dict the reference pickles into engine_dir/config.pkl (run.py:251) — the keys
    read are those of run.py:150-169, 273, 283-284."""

    def __init__(self, engine_buffer, config: dict, device: Optional[int] = None, _session: Optional[Session] = None):
        self.session = _session if _session is not None else Session.from_serialized_engine(engine_buffer, device)
        if self.session.info.kind != 2:
            raise ValueError("not a WhisperDecoder engine")
        self.config = config
        self.max_batch = 16   # utterances per engine call (wt_decoder_begin); larger batches are chunked by generate()

    def clone(self) -> "WhisperDecoderEngine":
        """Another engine on the same device weights (own resident KV caches, step graphs, mailbox): for a second host thread / stream."""
        return WhisperDecoderEngine(None, self.config, _session=self.session.clone())

    def _params(self, max_length, force_eos_step, logits_trace, force_eos_steps=None, return_timestamps=False, prompt_len=0, task_id=None):
        """`prompt_len`: tokens of a decoder prompt in front of the start token -- every position of the rules is an absolute sequence
        position, so begin_index and the forced pairs move behind the prompt (generation/utils.py:943 counts the prompt the same way).
        `task_id`: replaces the token at forced position 2 (`task=`)."""
        cfg = self.config
        begin_index = 1 if cfg.get("forced_bos_token_id") is None else 2          # run.py:155-156 with a 1-token prompt
        forced = cfg.get("forced_decoder_ids") or []
        if return_timestamps:                     # the (1, <|notimestamps|>) pair leaves the prompt
            forced = timestamp_rules(cfg)[4]
        if forced:
            begin_index += forced[-1][0]                                           # run.py:157
        begin_index += prompt_len
        forced = [[pos + prompt_len, task_id if pos == 2 and task_id is not None else tok] for pos, tok in forced]
        p = _lib.GreedyParams()
        p.decoder_start_token_id = cfg["decoder_start_token_id"]
        p.eos_token_id, p.pad_token_id = cfg["eos_token_id"], cfg["pad_token_id"]
        p.max_length = cfg["max_length"] if max_length is None else max_length
        p.begin_index = begin_index
        self._keep = []
        for field, count, vals in (("suppress_tokens", "n_suppress_tokens", cfg.get("suppress_tokens") or []),
                                   ("begin_suppress_tokens", "n_begin_suppress_tokens", cfg.get("begin_suppress_tokens") or []),
                                   ("forced_decoder_ids", "n_forced", [x for pair in forced for x in pair])):
            arr, n = _i32_array(vals)
            self._keep.append(arr)
            setattr(p, field, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)))
            setattr(p, count, n if field != "forced_decoder_ids" else n // 2)
        p.force_eos_step = -1 if force_eos_step is None else force_eos_step
        p.logits_trace = logits_trace.data_ptr() if logits_trace is not None else None
        if force_eos_steps is not None:           # bench-only per-row transcript lengths
            arr, _n = _i32_array(force_eos_steps)
            self._keep.append(arr)
            p.force_eos_steps = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
        return p

    def _set_timestamp_rules(self, on: bool, prompt_len: int = 0):
        t = None
        if on:
            no_ts, tb, ts_begin, max_init, _forced = timestamp_rules(self.config)
            t = _lib.TimestampParams(1, no_ts, tb, ts_begin + prompt_len, max_init)
        _lib.check(self.session._lib.wt_decoder_set_timestamp_rules(self.session.handle, ctypes.byref(t) if t is not None else None),
                   "wt_decoder_set_timestamp_rules")

    def _set_beam_search(self, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False):
        b = None
        if num_beams > 1:
            if early_stopping not in (False, True):
                raise ValueError(f"early_stopping must be False or True, got {early_stopping!r} (\"never\" is not supported)")
            b = _lib.BeamParams(int(num_beams), float(length_penalty), int(bool(early_stopping)))
        _lib.check(self.session._lib.wt_decoder_set_beam_search(self.session.handle, ctypes.byref(b) if b is not None else None),
                   "wt_decoder_set_beam_search")

    def _set_token_timestamps(self, heads=(), median_filter_width: int = 7, time_precision: float = 0.02):
        t = None
        if heads:
            arr, n = _i32_array([x for pair in heads for x in pair])
            self._tt_keep = arr
            t = _lib.TokenTimestampParams(n // 2, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), int(median_filter_width), float(time_precision))
        _lib.check(self.session._lib.wt_decoder_set_token_timestamps(self.session.handle, ctypes.byref(t) if t is not None else None),
                   "wt_decoder_set_token_timestamps")
        self._tt_heads = list(heads)

    def _set_logprobs(self, on: bool = False, no_speech_token_id=None):
        t = _lib.LogprobParams(1, -1 if no_speech_token_id is None else int(no_speech_token_id)) if on else None
        _lib.check(self.session._lib.wt_decoder_set_logprobs(self.session.handle, ctypes.byref(t) if t is not None else None),
                   "wt_decoder_set_logprobs")
        self._lp_ns = no_speech_token_id if on else None

    def _set_prompt(self, rows=None, ragged: bool = False):
        """`ragged`: rows of unequal lengths (wt_decoder_set_prompt_rows; the two calls replace each other)."""
        if rows and ragged:
            width = max(len(r) for r in rows)
            arr, _n = _i32_array([x for r in rows for x in r + [0] * (width - len(r))])
            lens, _m = _i32_array([len(r) for r in rows])
            self._prompt_keep = (arr, lens)
            _lib.check(self.session._lib.wt_decoder_set_prompt_rows(self.session.handle, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), len(rows),
                                                                     width, ctypes.cast(lens, ctypes.POINTER(ctypes.c_int32))),
                       "wt_decoder_set_prompt_rows")
            self._prompt_len = width
            return
        t = None
        if rows:
            arr, _n = _i32_array([x for r in rows for x in r])
            self._prompt_keep = arr
            t = _lib.PromptParams(ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), len(rows), len(rows[0]))
        _lib.check(self.session._lib.wt_decoder_set_prompt(self.session.handle, ctypes.byref(t) if t is not None else None), "wt_decoder_set_prompt")
        self._prompt_len = len(rows[0]) if rows else 0

    def _set_languages(self, language_ids=None, rows=None):
        """`rows`: per utterance a listed id or -1 = detect (wt_decoder_set_languages); no ids: off."""
        if language_ids:
            ids, n = _i32_array(language_ids)
            tok, m = _i32_array(rows)
            self._lang_keep = (ids, tok)
            _lib.check(self.session._lib.wt_decoder_set_languages(self.session.handle, ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), n,
                                                                   ctypes.cast(tok, ctypes.POINTER(ctypes.c_int32)), m), "wt_decoder_set_languages")
        else:
            _lib.check(self.session._lib.wt_decoder_set_languages(self.session.handle, None, 0, None, 0), "wt_decoder_set_languages")
        self._lang_ids = list(language_ids) if language_ids else []

    def read_languages(self):
        """DecodeLanguages of the decode in flight (wt_decoder_read_languages, stream-ordered; behind its first step)."""
        import torch
        dev = self._enc.device
        tok = torch.empty(self._B, dtype=torch.int32, device=dev)
        prob = torch.empty(self._B, len(self._lang_ids), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_read_languages(self.session.handle, tok.data_ptr(), prob.data_ptr(), ctypes.c_void_p(stream)),
                   "wt_decoder_read_languages")
        return DecodeLanguages(tok, prob, self._lang_ids)

    def detect_language(self, encoder_hidden):
        """openai-whisper's detect_language for a batch: (ids int32 [B], probs float32 [B, n_lang] over the config's language ids) on the
        GPU -- `begin(language="auto")`, the first step, `read_languages`."""
        import torch
        parts = []
        for i in range(0, encoder_hidden.shape[0], self.max_batch):
            self.begin(encoder_hidden[i:i + self.max_batch], language="auto")
            self.steps(1)
            parts.append(self.read_languages())
        return torch.cat([p.ids for p in parts]), torch.cat([p.probs for p in parts])

    def self_kv_head(self, layer: int, head: int, which: int = 0):
        """Debug read-back: the resident self-K (which 0) or self-V (1) rows of (layer, head), numpy float32 [B, max_target_positions, 64]."""
        import numpy as np
        import torch
        out = np.empty((self._B, self.session.info.max_target_positions, 64), dtype=np.float32)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_dbg_self_kv_head(self.session.handle, layer, head, which, out.ctypes.data, ctypes.c_void_p(stream)), "wt_dbg_self_kv_head")
        return out

    def _set_sampling(self, temperature: float = 0.0, seeds=()):
        t = None
        if temperature > 0:
            arr = (ctypes.c_uint64 * len(seeds))(*seeds)
            self._seed_keep = arr
            t = _lib.SamplingParams(float(temperature), ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint64)), len(seeds), 0)
        _lib.check(self.session._lib.wt_decoder_set_sampling(self.session.handle, ctypes.byref(t) if t is not None else None),
                   "wt_decoder_set_sampling")

    def read_logprobs(self, ids):
        """DecodeScores of the decode in flight for its ids [B, cur_len] (wt_decoder_read_logprobs, stream-ordered)."""
        import torch
        ml = self._p.max_length
        dev = self._enc.device
        tok = torch.empty(self._B, ml, dtype=torch.float32, device=dev)
        total = torch.empty(self._B, dtype=torch.float32, device=dev)
        nsp = torch.empty(self._B, dtype=torch.float32, device=dev) if self._lp_ns is not None else None
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_read_logprobs(self.session.handle, tok.data_ptr(), ml, total.data_ptr(),
                                                               nsp.data_ptr() if nsp is not None else None, ctypes.c_void_p(stream)),
                   "wt_decoder_read_logprobs")
        return DecodeScores(ids, tok[:, :ids.shape[1]].clone(), total, nsp, self._p.eos_token_id, getattr(self, "_prompt_len", 0))

    def read_token_timestamps(self, cur_len: int):
        """Token-level timestamps of the decode in flight (wt_decoder_read_token_timestamps: the cross-attention DTW post-pass on the
        device, stream-ordered): float32 [B, cur_len] seconds on the GPU, entry 0 of a row is 0."""
        import torch
        ml = self._p.max_length
        buf = torch.empty(self._B, ml, dtype=torch.float32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_read_token_timestamps(self.session.handle, buf.data_ptr(), ml, ctypes.c_void_p(stream)),
                   "wt_decoder_read_token_timestamps")
        return buf[:, :cur_len].clone()

    def token_timestamp_q_hist(self):
        """Debug read-back: the captured cross-attention queries, float32 [heads, B, max_length - 1, 64] on the GPU."""
        import torch
        out = torch.empty(len(self._tt_heads), self._B, self._p.max_length - 1, 64, dtype=torch.float32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_dbg_token_timestamp_q_hist(self.session.handle, out.data_ptr(), ctypes.c_void_p(stream)), "wt_dbg_token_timestamp_q_hist")
        return out

    def token_timestamp_matrix(self):
        """Debug read-back after `read_token_timestamps`: the DTW's input, float32 [B, max_length - 1, S] on the GPU (rows < cur_len - 1 valid)."""
        import torch
        out = torch.empty(self._B, self._p.max_length - 1, self.session.info.max_source_positions, dtype=torch.float32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_dbg_token_timestamp_matrix(self.session.handle, out.data_ptr(), ctypes.c_void_p(stream)), "wt_dbg_token_timestamp_matrix")
        return out

    def cross_k_head(self, layer: int, head: int):
        """Debug read-back: the resident cross-K rows of (layer, head), numpy float32 [B, S, 64] (fp16 engines: widened)."""
        import numpy as np
        import torch
        out = np.empty((self._B, self.session.info.max_source_positions, 64), dtype=np.float32)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_dbg_cross_k_head(self.session.handle, layer, head, out.ctypes.data, ctypes.c_void_p(stream)), "wt_dbg_cross_k_head")
        return out

    def begin(self, encoder_hidden, max_length=None, force_eos_step=None, logits_trace=None, force_eos_steps=None,
              return_timestamps: bool = False, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False,
              return_token_timestamps: bool = False, alignment_heads=None, median_filter_width: int = 7,
              return_logprobs: bool = False, no_speech_token_id=None, temperature: float = 0.0, seed: int = 0, seeds=None, prompt_ids=None,
              prompts=None, language=None, task=None):
        """Start a decode (wt_decoder_begin).  `language` / `task`: per-utterance language tokens or detection, and the task token (see `generate`; read the languages with `read_languages`).  `prompt_ids` / `prompts`: a decoder prompt in front of the start token, shared or of one length / per utterance (see `generate`).  `temperature` > 0: temperature sampling on the device (wt_decoder_set_sampling), row b drawing
        with `seeds[b]`, or `seed + b` without a list; not with beams.  `return_logprobs` / `no_speech_token_id`: see `generate` (read with `read_logprobs`).  `return_timestamps`: Whisper's timestamp mode (wt_decoder_set_timestamp_rules) --
        the prompt loses <|notimestamps|> and the ids carry <|t|> tokens (ids >= timestamp_begin, t x 0.02 s).
        `num_beams` > 1: beam search on the device (wt_decoder_set_beam_search) with transformers' `length_penalty` / `early_stopping`
        (False or True); utterances x num_beams <= 16 rows per call; not together with timestamps, logits_trace or force_eos_step(s).
        `return_token_timestamps`: per-token times by cross-attention DTW on the device (wt_decoder_set_token_timestamps; read them with
        `read_token_timestamps`), over `alignment_heads` [(layer, head), ...] (default: the config's) with transformers'
        `median_filter_width`; batch decodes only, not with beams; every row uses the batch-wide token length, as the reference."""
        import torch
        _check_beam_args(num_beams, return_timestamps, logits_trace, force_eos_step, force_eos_steps)
        i = self.session.info
        tt_heads = _check_token_timestamp_args(self.config, i, True, alignment_heads, median_filter_width, num_beams) if return_token_timestamps else []
        _check_logprob_args(return_logprobs, no_speech_token_id, num_beams, i.vocab_size)
        row_seeds = _check_sampling_args(temperature, seed, seeds, encoder_hidden, num_beams)
        if encoder_hidden.dtype != torch.float32 or tuple(encoder_hidden.shape[1:]) != (i.max_source_positions, i.d_model):
            raise ValueError(f"encoder_hidden must be float32 [B,{i.max_source_positions},{i.d_model}]")
        if not encoder_hidden.is_cuda or (logits_trace is not None and not logits_trace.is_cuda):
            raise ValueError("encoder_hidden / logits_trace must be CUDA (ROCm) tensors: the C-ABI takes device pointers")
        self._enc = encoder_hidden.contiguous()
        self._B = self._enc.shape[0]
        if force_eos_steps is not None and len(force_eos_steps) != self._B:
            raise ValueError(f"force_eos_steps needs one entry per utterance ({self._B}), got {len(force_eos_steps)}")
        prompt = None
        if prompt_ids is not None and prompts is not None:
            raise ValueError("prompt_ids and prompts cannot be combined (one shared / equal-length prompt, or one per utterance)")
        if prompt_ids is not None:
            prompt = prompt_rows(prompt_ids, self._B, i.max_target_positions)
        elif prompts is not None:
            prompt = ragged_prompt_rows(prompts, self._B, i.max_target_positions)
            if not any(prompt):
                prompt = None                     # all rows empty: no prompt
        if prompt:
            _check_prompt_args(prompt, i.vocab_size, self.config["max_length"] if max_length is None else max_length, num_beams,
                               return_token_timestamps, i.precision != 0)
        plen = max(len(r) for r in prompt) if prompt else 0
        lang_ids, lang_rows = _check_language_args(self.config, language, self._B, num_beams, return_token_timestamps)
        self._p = self._params(max_length, force_eos_step, logits_trace, force_eos_steps, return_timestamps, plen,
                               None if task is None else resolve_task(self.config, task))
        self._trace = logits_trace
        self._set_timestamp_rules(return_timestamps, plen)
        self._set_prompt(prompt, ragged=prompts is not None)
        self._set_languages(lang_ids, lang_rows)
        self._set_beam_search(num_beams, length_penalty, early_stopping)
        self._set_token_timestamps(tt_heads, median_filter_width)
        self._set_logprobs(return_logprobs, no_speech_token_id)
        self._set_sampling(temperature if row_seeds else 0.0, row_seeds)
        self._beams = int(num_beams) if num_beams > 1 else 1
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_begin(self.session.handle, self._enc.data_ptr(), self._B, ctypes.byref(self._p),
                                                       ctypes.c_void_p(stream)), "wt_decoder_begin")

    def steps(self, n: int):
        import torch
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_steps(self.session.handle, n, ctypes.c_void_p(stream)), "wt_decoder_steps")

    def poll(self):
        import torch
        cur, nu, done = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_poll(self.session.handle, ctypes.byref(cur), ctypes.byref(nu), ctypes.byref(done),
                                                      ctypes.c_void_p(stream)), "wt_decoder_poll")
        return cur.value, nu.value, bool(done.value)

    def run(self, lookahead: int = 0):
        """Drive the decode in flight to its stop test (wt_decoder_run): the host keeps `lookahead` steps queued behind the running
        one and watches a pinned mailbox word instead of synchronising the stream.  Returns (cur_len, n_unfinished)."""
        import torch
        cur, nu = ctypes.c_int(), ctypes.c_int()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_run(self.session.handle, lookahead, ctypes.byref(cur), ctypes.byref(nu),
                                                     ctypes.c_void_p(stream)), "wt_decoder_run")
        return cur.value, nu.value

    def read_ids(self, cur_len: int):
        import torch
        ml = self._p.max_length
        buf = torch.empty(self._B, ml, dtype=torch.int32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_read_ids(self.session.handle, buf.data_ptr(), ml, ctypes.c_void_p(stream)),
                   "wt_decoder_read_ids")
        if getattr(self, "_beams", 1) > 1:
            # the best hypothesis per utterance, EOS behind it when it fits, then pad: the width of BeamSearchScorer.finalize is
            # min(longest hypothesis + 1, max_length).  A hypothesis never holds the EOS id itself (an EOS candidate ends its beam).
            # (int(lens.max()) below waits for the copy: the C call itself stays stream-ordered, this width does not)
            is_eos = buf[:, 1:] == self._p.eos_token_id
            lens = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full_like(buf[:, 0], ml))
            return buf[:, :min(int(lens.max()) + 1, ml)].clone()
        return buf[:, :cur_len].clone()

    def read_beam_scores(self):
        """Sequence scores of the beam decode in flight (sum of log-probabilities / length ** length_penalty), float32 [B] on the GPU."""
        import torch
        out = torch.empty(self._B, dtype=torch.float32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_read_beam_scores(self.session.handle, out.data_ptr(), ctypes.c_void_p(stream)),
                   "wt_decoder_read_beam_scores")
        return out

    def beam_trace(self, steps: int):
        """Debug read-back of a beam decode: int32 [steps, rows, 4] = (token, source beam within the utterance, score bits, done)."""
        import torch
        out = torch.empty(steps, self._B * self._beams, 4, dtype=torch.int32, device=self._enc.device)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_dbg_beam_trace(self.session.handle, out.data_ptr(), steps, ctypes.c_void_p(stream)), "wt_dbg_beam_trace")
        return out

    def generate(self, encoder_hidden, max_length=None, force_eos_step=None, logits_trace=None, chunk: int = 0, force_eos_steps=None,
                 lookahead: int = 0, return_timestamps: bool = False, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, return_scores: bool = False, return_token_timestamps: bool = False, alignment_heads=None,
                 median_filter_width: int = 7, return_logprobs: bool = False, no_speech_token_id=None, temperature: float = 0.0,
                 seed: int = 0, seeds=None, prompt_ids=None, prompts=None, language=None, task=None):
        """== greedy_search(...) of run.py:171-227 for a batch; returns int32 ids [B, len] on the GPU.
        `language`: per-utterance language tokens (include/whisper_trtllm_amd.h (9i)) for a multilingual config, whose forced list holds a
        language token at position 1: "auto" detects every row's language in the first step of the decode (openai-whisper's
        detect_language, without a decoder pass of its own); an id of the config's `language_ids`, a code ("en") or a token ("<|en|>") of
        its `lang_to_id` sets it; a list gives one of those per utterance.  The result then carries a DecodeLanguages as its LAST element
        (ids, languages) / (ids, DecodeScores, languages).  At most 16 utterances per call; not with num_beams > 1 or
        return_token_timestamps.  `task`: "transcribe" / "translate" (the config's `task_to_id`) or a token id: replaces the token at
        forced position 2.
        `prompts`: per-utterance decoder prompts of unequal lengths (several recordings under condition_on_previous_text): one sequence per
        utterance, each empty or starting with <|startofprev|>, cut like `prompt_ids`; not together with it.  With Lmax the longest, the
        returned rows are left-padded with pad_token_id to Lmax in front of the start token (`strip_prompts` removes pad and prompt),
        max_length counts Lmax and DecodeScores carry prompt_len = Lmax (include/whisper_trtllm_amd.h (9h)).  All rows empty: no prompt.
        `prompt_ids`: a decoder prompt (transformers' generate(prompt_ids=...), openai-whisper's initial_prompt / previous text): a 1-D
        sequence shared by the batch or a 2-D [B, n] one with per-row contents of equal length, first entry <|startofprev|>, the text part
        cut to its last max_target_positions // 2 - 1 tokens.  The prompt runs through the decoder in one pass on the device (the prefill,
        include/whisper_trtllm_amd.h (9g)); the returned ids hold it in front of the start token, max_length counts it, and DecodeScores
        count generated positions only.  fp32 decoder engines; not with num_beams > 1 or return_token_timestamps.
        `temperature` > 0: every token is a draw from softmax(scores / temperature) instead of the argmax (Gumbel-max over a counter-based
        generator, on the device; include/whisper_trtllm_amd.h (9f)).  Utterance b draws with `seeds[b]`, or with `seed + b`: a draw depends
        on the seed, the position and the id alone, so it is repeatable and independent of the batch.  Log-probabilities of a sampled decode
        are those of the untempered scores.  Not with num_beams > 1.
        `return_logprobs`: token log-probabilities from the device (wt_decoder_set_logprobs, no extra launch): returns (ids, DecodeScores),
        or (ids, token timestamps, DecodeScores) with `return_token_timestamps`; `no_speech_token_id` also fills
        DecodeScores.no_speech_prob.  Greedy decoding only (not with num_beams > 1).
        `return_timestamps`: timestamp mode (see `begin`).  `num_beams` > 1: beam search (see `begin`), the best hypothesis per
        utterance; `return_scores`: (ids, float32 sequence scores [B]) -- beam search only.

        Default (`chunk` 0): the stop test is followed through the engine's host mailbox (`run`), at most `lookahead` steps are
        enqueued past the stop.  `chunk` > 0 selects the older protocol -- `chunk` steps between two synchronising polls.
        `return_token_timestamps`: returns (ids, float32 token timestamps [B, len] in seconds) -- see `begin`."""
        _check_beam_args(num_beams, return_timestamps, logits_trace, force_eos_step, force_eos_steps)
        if return_logprobs or no_speech_token_id is not None:
            _check_logprob_args(return_logprobs, no_speech_token_id, num_beams, self.session.info.vocab_size)
        if return_scores and num_beams <= 1:
            raise ValueError("return_scores needs num_beams > 1 (greedy decoding keeps no sequence score)")
        row_seeds = _check_sampling_args(temperature, seed, seeds, encoder_hidden, num_beams)
        samp = lambda i, j: {"temperature": temperature, "seeds": row_seeds[i:j]} if row_seeds else {}
        lk = {}
        if language is not None:
            _check_language_args(self.config, language, int(encoder_hidden.shape[0]), num_beams, return_token_timestamps)
            if encoder_hidden.shape[0] > self.max_batch:
                raise ValueError(f"language= supports at most {self.max_batch} utterances per call")
            lk["language"] = language
        if task is not None:
            resolve_task(self.config, task)
            lk["task"] = task
        prompt = None
        if prompt_ids is not None and prompts is not None:
            raise ValueError("prompt_ids and prompts cannot be combined (one shared / equal-length prompt, or one per utterance)")
        if prompts is not None:
            info = self.session.info
            ragged = ragged_prompt_rows(prompts, encoder_hidden.shape[0], info.max_target_positions)
            if not any(ragged):
                prompts = None                    # all rows empty: no prompt
            else:
                ml = self.config["max_length"] if max_length is None else max_length
                _check_prompt_args(ragged, info.vocab_size, ml, num_beams, return_token_timestamps, info.precision != 0)
                if encoder_hidden.shape[0] > self.max_batch:
                    if task is not None:
                        raise ValueError(f"task= with prompts= supports at most {self.max_batch} utterances per call")
                    return self._generate_ragged_sliced(encoder_hidden, ragged, ml, force_eos_step, logits_trace, chunk, force_eos_steps, lookahead,
                                                        return_timestamps, return_logprobs, no_speech_token_id, temperature, row_seeds)
        if prompt_ids is not None:   # (begin() checks again on the single-batch path; here the rows are also needed to slice a >16-row batch)
            info = self.session.info
            prompt = prompt_rows(prompt_ids, encoder_hidden.shape[0], info.max_target_positions)
            _check_prompt_args(prompt, info.vocab_size, self.config["max_length"] if max_length is None else max_length, num_beams,
                               return_token_timestamps, info.precision != 0)
        # the prompt rows of utterances i..j (engine batches of a larger batch slice them with the encoder rows)
        pk = lambda i, j: {"prompt_ids": prompt if len(prompt) == 1 else prompt[i:j]} if prompt else ({"prompts": prompts} if prompts is not None else {})
        tt = None
        if return_token_timestamps:
            _check_token_timestamp_args(self.config, self.session.info, True, alignment_heads, median_filter_width, num_beams)
            tt = {"return_token_timestamps": True, "alignment_heads": alignment_heads, "median_filter_width": median_filter_width}
        group = self.max_batch // max(int(num_beams), 1)
        if num_beams > 1 and encoder_hidden.shape[0] > group:   # utterances x beams <= 16 rows per engine call
            import torch
            parts = [self.generate(encoder_hidden[i:i + group], max_length, None, None, chunk, None, lookahead, False, num_beams,
                                   length_penalty, early_stopping, True, **lk) for i in range(0, encoder_hidden.shape[0], group)]
            width = max(p[0].shape[1] for p in parts)
            ids = torch.cat([torch.nn.functional.pad(p[0], (0, width - p[0].shape[1]), value=self.config["pad_token_id"]) for p in parts], dim=0)
            return (ids, torch.cat([p[1] for p in parts])) if return_scores else ids
        if num_beams > 1:
            self.begin(encoder_hidden, max_length, num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping, **lk)
            if chunk <= 0:
                cur, _nu = self.run(lookahead)
            else:
                cur, done, ml = 1, False, self._p.max_length
                while not done and cur < ml:
                    self.steps(min(chunk, ml - cur))
                    cur, _nu, done = self.poll()
            ids = self.read_ids(cur)
            return (ids, self.read_beam_scores()) if return_scores else ids
        if encoder_hidden.shape[0] > self.max_batch:
            # larger batches run as consecutive engine batches of <= 16 utterances;
            # rows are independent, so the result is the concatenation (shorter groups are right-padded with pad_token_id)
            import torch
            if logits_trace is not None:
                raise ValueError(f"logits_trace supports at most {self.max_batch} utterances per call")
            lp = {"return_logprobs": True, "no_speech_token_id": no_speech_token_id} if return_logprobs else {}
            parts = [self.generate(encoder_hidden[i:i + self.max_batch], max_length, force_eos_step, None, chunk,
                                   None if force_eos_steps is None else force_eos_steps[i:i + self.max_batch], lookahead,
                                   return_timestamps, **(tt or {}), **lp, **samp(i, i + self.max_batch), **pk(i, i + self.max_batch), **lk)
                     for i in range(0, encoder_hidden.shape[0], self.max_batch)]
            pad = self.config["pad_token_id"]
            cat = lambda ps, value: torch.cat([torch.nn.functional.pad(p, (0, max(q.shape[1] for q in ps) - p.shape[1]), value=value) for p in ps], dim=0)
            if return_logprobs:   # rows are independent: the scores of the engine batches, side by side
                ids = cat([p[0] for p in parts], pad)
                sc = [p[-1] for p in parts]
                scores = DecodeScores(ids, cat([x.token_logprobs for x in sc], 0.0), torch.cat([x.sum_logprob for x in sc]),
                                      torch.cat([x.no_speech_prob for x in sc]) if no_speech_token_id is not None else None,
                                      self.config["eos_token_id"], len(prompt[0]) if prompt else 0)
                return (ids, cat([p[1] for p in parts], 0.0), scores) if tt else (ids, scores)
            if tt:      # every engine batch ran to its own length: its rows' times are those of that length
                return cat([p[0] for p in parts], pad), cat([p[1] for p in parts], 0.0)
            return cat(parts, pad)
        self.begin(encoder_hidden, max_length, force_eos_step, logits_trace, force_eos_steps, return_timestamps, **(tt or {}),
                   return_logprobs=return_logprobs, no_speech_token_id=no_speech_token_id, **samp(0, None), **pk(0, None), **lk)
        if chunk <= 0:
            cur, _nu = self.run(lookahead)
        else:
            cur, done = 1 + self._prompt_len, False
            ml = self._p.max_length
            while not done and cur < ml:
                self.steps(min(chunk, ml - cur))
                cur, _nu, done = self.poll()
        langs = (self.read_languages(),) if language is not None else ()
        if return_logprobs:
            ids = self.read_ids(cur)
            scores = self.read_logprobs(ids)
            return (ids, self.read_token_timestamps(cur), scores) + langs if tt else (ids, scores) + langs
        if tt:
            return (self.read_ids(cur), self.read_token_timestamps(cur)) + langs
        return (self.read_ids(cur),) + langs if langs else self.read_ids(cur)

    def _generate_ragged_sliced(self, encoder_hidden, rows, max_length, force_eos_step, logits_trace, chunk, force_eos_steps, lookahead,
                                return_timestamps, return_logprobs, no_speech_token_id, temperature, row_seeds):
        """`generate(prompts=...)` over more than 16 utterances: consecutive engine batches, each left-padded to its own longest prompt and
        with max_length lowered by what that is shorter than the whole batch's, so that every row keeps its budget of generated tokens;
        the parts are then shifted to the whole batch's longest prompt."""
        import torch
        if logits_trace is not None:
            raise ValueError(f"logits_trace supports at most {self.max_batch} utterances per call")
        L, pad, step = max(len(r) for r in rows), self.config["pad_token_id"], self.max_batch
        parts = []
        for i in range(0, encoder_hidden.shape[0], step):
            sub = rows[i:i + step]
            shift = L - max(len(r) for r in sub)
            out = self.generate(encoder_hidden[i:i + step], max_length - shift, force_eos_step, None, chunk,
                                None if force_eos_steps is None else force_eos_steps[i:i + step], lookahead, return_timestamps,
                                return_logprobs=return_logprobs, no_speech_token_id=no_speech_token_id,
                                **({"temperature": temperature, "seeds": row_seeds[i:i + step]} if row_seeds else {}), prompts=sub)
            parts.append((shift, out))
        left = lambda x, shift, value: torch.nn.functional.pad(x, (shift, 0), value=value)
        cat = lambda ps, value: torch.cat([torch.nn.functional.pad(p, (0, max(q.shape[1] for q in ps) - p.shape[1]), value=value) for p in ps], dim=0)
        if not return_logprobs:
            return cat([left(o, sh, pad) for sh, o in parts], pad)
        ids = cat([left(o[0], sh, pad) for sh, o in parts], pad)
        sc = [o[1] for _sh, o in parts]
        scores = DecodeScores(ids, cat([left(o[1].token_logprobs, sh, 0.0) for sh, o in parts], 0.0), torch.cat([x.sum_logprob for x in sc]),
                              torch.cat([x.no_speech_prob for x in sc]) if no_speech_token_id is not None else None, self.config["eos_token_id"], L)
        return ids, scores

    def generate_with_fallback(self, encoder_hidden, temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold=2.4,
                               logprob_threshold=-1.0, no_speech_threshold=0.6, no_speech_token_id=None, text_of=None, seed: int = 0,
                               seeds=None, **generate_kwargs):
        """openai-whisper's decode_with_fallback, batched: decode every row at temperatures[0]; a row needs another try when
        compression_ratio(text) > compression_ratio_threshold or avg_logprob < logprob_threshold -- unless no_speech_prob >
        no_speech_threshold (silence: the transcript is dropped anyway); a threshold of None is skipped (no_speech also without a
        `no_speech_token_id`).  The encoder rows that need it are gathered and decoded again at the next temperature, until none is left
        or the list ends; a row keeps the result of the last temperature it was decoded at.  Row i draws with `seed + i` at every
        temperature (or with `seeds[i]`, for a caller whose rows are not consecutive utterances), whichever other rows are decoded beside
        it.  `text_of(ids) -> str` gives the text whose compression ratio is taken
        (default: the config's token decoder, or the ids in decimal).  `prompt_ids` (see `generate`) goes to every try; the EOS is searched
        behind the prompt and the compression ratio is taken of the text without it.  `language` / `task` (see `generate`): the first try
        detects or sets the rows' languages, every later try decodes its rows with the languages of the first; the result then ends with
        the DecodeLanguages of the first try.  `prompts` (per-utterance, see `generate`): a try
        decodes its rows left-padded to ITS longest prompt, with max_length lowered by what that is shorter than the whole batch's -- every
        row keeps its budget of generated tokens and, drawing at its own positions, its result whichever rows are tried beside it; the
        returned rows are all left-padded to the whole batch's longest.  Returns (ids int32 [B, len] padded with pad_token_id, DecodeScores,
        temperature_used float32 [B])."""
        import torch
        from .text import compression_ratio
        temperatures = [float(t) for t in temperatures]
        if not temperatures:
            raise ValueError("temperatures must not be empty")
        for key in ("temperature", "return_logprobs", "num_beams", "return_scores", "return_token_timestamps"):
            if key in generate_kwargs:
                raise ValueError(f"generate_with_fallback does not take {key}")
        text_of = text_of or _default_text_of(self.config)
        eos, pad = self.config["eos_token_id"], self.config["pad_token_id"]
        B = int(encoder_hidden.shape[0])
        row_seed = [int(seed) + i for i in range(B)] if seeds is None else [int(x) for x in seeds]
        if len(row_seed) < B:
            raise ValueError(f"seeds needs one entry per utterance ({B}), got {len(row_seed)}")
        language = generate_kwargs.pop("language", None)
        langs = None
        if language is not None:
            if B > self.max_batch:
                raise ValueError(f"language= supports at most {self.max_batch} utterances per call")
            resolve_languages(self.config, language, B)
        lang_of = lambda rows: {} if language is None else {"language": language if langs is None else [int(found[i]) for i in rows]}
        prompt = generate_kwargs.pop("prompt_ids", None)
        ragged = generate_kwargs.pop("prompts", None)
        if prompt is not None and ragged is not None:
            raise ValueError("prompt_ids and prompts cannot be combined (one shared / equal-length prompt, or one per utterance)")
        if prompt is not None:
            prompt = prompt_rows(prompt, B, self.session.info.max_target_positions)
        plen = len(prompt[0]) if prompt else 0
        if ragged is not None:
            ragged = ragged_prompt_rows(ragged, B, self.session.info.max_target_positions)
            plen = max(len(r) for r in ragged)
            if plen == 0:
                ragged = None
            else:
                ml = generate_kwargs.pop("max_length", None)
                ml = self.config["max_length"] if ml is None else ml
        todo = list(range(B))
        rows = [None] * B                      # per original row: (ids, token_logprobs, sum_logprob, no_speech_prob, temperature)
        for t in temperatures:
            hidden = encoder_hidden if len(todo) == B else encoder_hidden[torch.as_tensor(todo, device=encoder_hidden.device)]
            shift = 0
            if ragged:   # this try's rows at their own longest prompt, then shifted to the whole batch's
                sub = [ragged[i] for i in todo]
                shift = plen - max(len(r) for r in sub)
                out = self.generate(hidden, max_length=ml - shift, return_logprobs=True, no_speech_token_id=no_speech_token_id, temperature=t,
                                    seeds=[row_seed[i] for i in todo], **generate_kwargs, prompts=sub, **lang_of(todo))
                ids, sc = out[0], out[1]
                if shift:
                    ids = torch.nn.functional.pad(ids, (shift, 0), value=pad)
                    sc.token_logprobs = torch.nn.functional.pad(sc.token_logprobs, (shift, 0), value=0.0)
            else:
                out = self.generate(hidden, return_logprobs=True, no_speech_token_id=no_speech_token_id, temperature=t,
                                    seeds=[row_seed[i] for i in todo], **generate_kwargs, **lang_of(todo),
                                    **({"prompt_ids": prompt if len(prompt) == 1 else [prompt[i] for i in todo]} if prompt else {}))
                ids, sc = out[0], out[1]
            if language is not None and langs is None:   # the first try covers every row: its languages are the decode's
                langs = out[2]
                found = langs.ids.cpu().tolist()
            avg = sc.avg_logprob.cpu().tolist()
            nsp = sc.no_speech_prob.cpu().tolist() if sc.no_speech_prob is not None else [None] * len(todo)
            host_ids = ids.cpu().tolist()
            again = []
            for k, i in enumerate(todo):
                rows[i] = (ids[k], sc.token_logprobs[k], sc.sum_logprob[k], None if sc.no_speech_prob is None else sc.no_speech_prob[k], t)
                row = host_ids[k][plen:]
                if eos in row[1:]:
                    row = row[:row.index(eos, 1) + 1]
                needs = False
                if compression_ratio_threshold is not None:
                    text = text_of(row)
                    needs = bool(text) and compression_ratio(text) > compression_ratio_threshold
                if logprob_threshold is not None and avg[k] < logprob_threshold:
                    needs = True
                if no_speech_threshold is not None and nsp[k] is not None and nsp[k] > no_speech_threshold:
                    needs = False
                if needs:
                    again.append(i)
            todo = again
            if not todo:
                break
        width = max(r[0].shape[0] for r in rows)
        padded = lambda x, value: torch.nn.functional.pad(x, (0, width - x.shape[0]), value=value)
        ids = torch.stack([padded(r[0], pad) for r in rows])
        scores = DecodeScores(ids, torch.stack([padded(r[1], 0.0) for r in rows]), torch.stack([r[2] for r in rows]),
                              torch.stack([r[3] for r in rows]) if rows[0][3] is not None else None, eos, plen)
        temps = torch.tensor([r[4] for r in rows], dtype=torch.float32, device=ids.device)
        return (ids, scores, temps, langs) if language is not None else (ids, scores, temps)

    def stream(self, slots: int = 8, pool_rows: int = 0, max_length=None, return_timestamps: bool = False, num_beams: int = 1,
               return_token_timestamps: bool = False) -> "DecodeStream":
        """Open a continuous decode on this engine (wt_decoder_stream_*): `slots` rows stay busy, every utterance stops at its own EOS
        and its slot is refilled on the device within the same step.  Ends with the next `begin` / `generate` on this engine.
        The continuous mode has no timestamp mode: `return_timestamps=True` raises ValueError."""
        if return_timestamps:
            raise ValueError("timestamp mode is a batch-decode feature (generate / begin); the continuous mode does not predict timestamps")
        if num_beams > 1:
            raise ValueError("beam search is a batch-decode feature (generate / begin); the continuous mode decodes greedily")
        if return_token_timestamps:
            raise ValueError("token-level timestamps are a batch-decode feature (generate / begin); the continuous mode keeps no query history")
        return DecodeStream(self, slots, pool_rows, max_length)

    def set_profiling(self, enabled: bool):
        _lib.check(self.session._lib.wt_engine_set_profiling(self.session.handle, int(enabled)), "wt_engine_set_profiling")

    def time_cross_attention(self, iters: int = 20) -> float:
        """Average launch time (us) of the cross-attention kernel, graph-replayed over the resident caches."""
        import torch
        us = ctypes.c_float()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_time_cross_attention(self.session.handle, iters, ctypes.byref(us),
                                                                      ctypes.c_void_p(stream)), "wt_decoder_time_cross_attention")
        return float(us.value)

    def time_kernel(self, which: str, iters: int = 20) -> float:
        """Average launch time (us) of one kind of per-layer decode launch ("qkv", "self_attn", "pair", "cross_attn", "cross_out",
        "fc1", "fc2"), graph-replayed over all layers' own weights and caches."""
        import torch
        us = ctypes.c_float()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.session._lib.wt_decoder_time_kernel(self.session.handle, which.encode(), iters, ctypes.byref(us),
                                                             ctypes.c_void_p(stream)), "wt_decoder_time_kernel")
        return float(us.value)

    def timer(self, which: str):
        t = _lib.KernelTimer()
        _lib.check(self.session._lib.wt_engine_get_timer(self.session.handle, which.encode(), ctypes.byref(t)), "wt_engine_get_timer")
        return t.ms_total, t.launches


class DecodeStream:
    """Continuous greedy decoding (the C-ABI's wt_decoder_stream_*): utterances are SUBMITTED as encoder memory, wait in a device-side
    queue, and take over a decode slot the moment its previous utterance emits EOS (or reaches max_length) -- the per-utterance stop
    the reference gets from transcribing one clip at a time (run.py:219-226), without a batch waiting for its longest row.

        st = dec.stream(slots=8)
        h = st.submit(enc(mel_chunk))             # handles, one per utterance; any number of chunks ahead (pool_rows bounds it)
        st.run(min_waiting=8)                     # steps until fewer than 8 utterances wait (submit more) or everything has finished
        for handle, ids in st.collect(): ...      # finished utterances (numpy int32 rows, start token .. EOS), cache rows released
    """

    def __init__(self, dec: "WhisperDecoderEngine", slots: int, pool_rows: int = 0, max_length=None):
        import torch
        self.dec, self.slots = dec, int(slots)
        self._lib, self._h = dec.session._lib, dec.session.handle
        self._p = dec._params(max_length, None, None)
        self.max_length = int(self._p.max_length)
        dec._set_timestamp_rules(False)     # a timestamp decode before on this handle left the mode on
        dec._set_beam_search(1)             # ... and so did a beam decode
        dec._set_token_timestamps(())       # ... and a decode with token-level timestamps
        dec._set_sampling(0.0)              # ... and a sampled decode
        dec._set_prompt(None)               # ... and a decode behind a prompt
        dec._set_languages(None)            # ... and a decode with per-row languages
        self.pool_rows = int(pool_rows) if pool_rows else 4 * self.slots
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self._lib.wt_decoder_stream_begin(self._h, self.slots, self.pool_rows, ctypes.byref(self._p), ctypes.c_void_p(stream)),
                   "wt_decoder_stream_begin")
        self._open: List[int] = []          # handles submitted and not collected yet, in submission order
        self._keep: List[Any] = []          # encoder memories whose K/V projection may still be queued on the stream
        self.n_submitted = 0
        self.n_steps = 0

    def free_rows(self) -> int:
        return self.pool_rows - len(self._open)

    def submit(self, encoder_hidden, force_eos_steps: Optional[Sequence[int]] = None) -> List[int]:
        """Queue the utterances of `encoder_hidden` f32 [n, S, d] (n <= 16, n <= free_rows()); returns their handles."""
        import torch
        i = self.dec.session.info
        if encoder_hidden.dtype != torch.float32 or tuple(encoder_hidden.shape[1:]) != (i.max_source_positions, i.d_model) or not encoder_hidden.is_cuda:
            raise ValueError(f"encoder_hidden must be a CUDA float32 [n,{i.max_source_positions},{i.d_model}] tensor")
        h = encoder_hidden.contiguous()
        n = h.shape[0]
        if force_eos_steps is not None and len(force_eos_steps) != n:
            raise ValueError("force_eos_steps needs one entry per utterance")
        fe = None
        if force_eos_steps is not None:
            fe, _ = _i32_array(force_eos_steps)
        handles = (ctypes.c_int32 * n)()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self._lib.wt_decoder_stream_submit(self._h, h.data_ptr(), n, fe, handles, ctypes.c_void_p(stream)), "wt_decoder_stream_submit")
        self._keep.append(h)
        if len(self._keep) > 8:             # projections are stream-ordered: anything this old has long been consumed by later steps
            self._keep.pop(0)
        out = [int(x) for x in handles]
        self._open.extend(out)
        self.n_submitted += n
        return out

    def run(self, min_waiting: int = 0, lookahead: int = 0):
        """Step until everything submitted has finished, or (min_waiting > 0) until fewer than `min_waiting` utterances still wait
        for a slot.  Returns (finished so far, upper bound of utterances still waiting)."""
        import torch
        fin, wait, steps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self._lib.wt_decoder_stream_run(self._h, int(min_waiting), int(lookahead), ctypes.byref(fin), ctypes.byref(wait),
                                                   ctypes.byref(steps), ctypes.c_void_p(stream)), "wt_decoder_stream_run")
        self.n_steps = steps.value          # decoder steps enqueued since the stream was opened
        return fin.value, wait.value

    def collect(self):
        """[(handle, ids)] of the utterances that have finished since the last call (numpy int32, start token through EOS / max_length);
        their cache rows return to the pool."""
        import numpy as np
        out, still = [], []
        buf = (ctypes.c_int32 * self.max_length)()
        n = ctypes.c_int()
        for h in self._open:
            _lib.check(self._lib.wt_decoder_stream_collect(self._h, h, buf, self.max_length, ctypes.byref(n)), "wt_decoder_stream_collect")
            if n.value > 0:
                out.append((h, np.ctypeslib.as_array(buf)[:n.value].copy()))
            else:
                still.append(h)
        self._open = still
        return out


def transcribe_continuous(enc: "WhisperEncoderEngine", dec: "WhisperDecoderEngine", mels, slots: int = 8, chunk: int = 8,
                          force_eos_steps: Optional[Sequence[int]] = None, max_length=None, stats: Optional[dict] = None,
                          pool_rows: int = 0, return_timestamps: bool = False, num_beams: int = 1) -> List[Any]:
    """Encoder + continuous greedy decode of `mels` ([N, n_mels, 2*S] tensor or a list of such rows) in ARRIVAL order: the encoder runs
    on chunks of `chunk` utterances just ahead of the decode, `slots` rows decode at any time.  Returns N numpy id rows (start token
    through EOS) in input order.  This is the host scheduler of the C-ABI's continuous mode -- what cal_wer.py / run.py use for a
    dataset whose transcripts differ in length.  `stats` (optional dict) receives the slot utilisation of the run."""
    import torch
    if return_timestamps:
        raise ValueError("timestamp mode is a batch-decode feature (WhisperDecoderEngine.generate); the continuous mode does not predict timestamps")
    if num_beams > 1:
        raise ValueError("beam search is a batch-decode feature (WhisperDecoderEngine.generate); the continuous mode decodes greedily")
    n = len(mels)
    results: List[Any] = [None] * n
    if n == 0:
        return results
    st = dec.stream(slots=slots, pool_rows=pool_rows, max_length=max_length)
    index_of = {}
    nxt = 0

    def submit_next() -> int:
        nonlocal nxt
        k = min(chunk, n - nxt, st.free_rows())
        if k <= 0:
            return 0
        part = mels[nxt:nxt + k]
        x = part if torch.is_tensor(part) else torch.stack(list(part))
        fe = None if force_eos_steps is None else [int(v) for v in force_eos_steps[nxt:nxt + k]]
        for j, h in enumerate(st.submit(enc(x), fe)):
            index_of[h] = nxt + j
        nxt += k
        return k

    def harvest():
        for h, ids in st.collect():
            results[index_of.pop(h)] = ids

    waiting = 0          # upper bound of the submitted utterances still waiting for a slot
    while True:
        # keep at least `slots` utterances waiting while there are more to come: a freed slot then never runs dry while the next
        # chunk's encoder pass is still ahead
        while nxt < n and waiting < slots and st.free_rows() > 0:
            waiting += submit_next()
        more = nxt < n
        if more and st.free_rows() == 0:     # cache pool exhausted: step until one more utterance has been admitted (= one has finished)
            _, waiting = st.run(min_waiting=max(1, waiting))
        else:
            _, waiting = st.run(min_waiting=slots if more else 0)
        harvest()
        if not more and not st._open:
            break
    assert all(r is not None for r in results)
    if stats is not None:   # slot utilisation = row-steps that produced a token some utterance needed / row-steps paid for
        stats["row_steps"] = int(sum(len(r) - 1 for r in results))
        stats["steps"] = int(st.n_steps)
        stats["slot_utilisation"] = stats["row_steps"] / float(max(1, st.n_steps) * slots)
    return results


def transcribe_long(enc: "WhisperEncoderEngine", dec: "WhisperDecoderEngine", frontend, audios, **options):
    """Long-form transcription (recordings longer than one window): openai-whisper's seek loop, batched over the recordings of `audios`
    (1-D float32 GPU tensors) -- see longform.transcribe_long for the options and longform.transcribe for the result."""
    from . import longform
    return longform.transcribe_long(enc, dec, frontend, audios, **options)


class WhisperPipeline:
    """`workers` independent (encoder, decoder) engine pairs on ONE GPU, each driven by its own host thread on its own HIP stream.

    Why: a greedy decode is a chain of ~170 dependent, launch-latency-bound kernels per token -- it leaves most of the chip idle
    most of the time -- while the encoder is MFMA-bound.  Batches are independent (the reference transcribes one clip after the
    other, run.py:262-290), so a second in-flight batch fills the first one's gaps: two workers of batch 8 measure ~1.4x one worker
    on whisper-medium.en (434 vs 312 audio-s/s with 447-step decodes; DESIGN.md section 6 "Workers per GPU").  Every worker is a
    complete execution context (own workspace, resident KV cache, step graphs: ~4 GB for medium.en fp32) on ONE shared, read-only copy
    of the weights (`wt_engine_clone`), so nothing mutable is shared and no lock is taken on the device path; `transcribe` hands the batches out dynamically (a worker takes the next batch when it is done).
    Under rocprofv3 (`under_rocprof()`) the pipeline clamps itself to ONE worker: concurrent graph replays from several host threads
    aborted under the profiler in round 3 (cause not established, see `under_rocprof`); the kernels profiled are the same."""

    def __init__(self, encoder_buffer, decoder_buffer, config: dict, workers: int = 2, device: Optional[int] = None):
        import torch
        if workers < 1:
            raise ValueError("workers must be >= 1")
        if workers > 1 and under_rocprof():
            logger.warning(f"WhisperPipeline: rocprofv3 is loaded into this process -- running 1 worker instead of {workers} "
                           "(concurrent graph replays from several host threads abort under the profiler; the kernels are the same)")
            workers = 1
        self.device = torch.cuda.current_device() if device is None else device
        self.config = config
        enc0, dec0 = WhisperEncoderEngine(encoder_buffer, self.device), WhisperDecoderEngine(decoder_buffer, config, self.device)
        self.engines = [(enc0, dec0)] + [(enc0.clone(), dec0.clone()) for _ in range(workers - 1)]   # ONE copy of the weights on the device
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(workers)]

    def transcribe(self, mel_batches: Sequence[Any], gen_kwargs: Optional[Sequence[dict]] = None) -> List[Any]:
        """Encoder + greedy decode of every batch `[b_i, n_mels, 2*S]` (b_i <= 16 per engine call; larger ones are chunked by
        `generate`); returns the id tensors in the order of `mel_batches`.  `gen_kwargs[i]` are extra arguments of `generate` for
        batch i (max_length, force_eos_steps, ...).  Blocks until every batch is done."""
        import torch
        n = len(mel_batches)
        if gen_kwargs is not None and len(gen_kwargs) != n:
            raise ValueError("gen_kwargs needs one entry per batch")
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))      # the caller's pending work on the inputs

        def setup(k: int):
            torch.cuda.set_device(self.device)
            self.streams[k].wait_event(ready)

        def item(k: int, i: int):
            enc, dec = self.engines[k]
            with torch.cuda.stream(self.streams[k]):
                kw = dict(gen_kwargs[i]) if gen_kwargs is not None else {}
                fallback = kw.pop("temperature_fallback", None)      # a dict of generate_with_fallback's own arguments
                if fallback is not None:
                    return dec.generate_with_fallback(enc(mel_batches[i]), **fallback, **kw)
                return dec.generate(enc(mel_batches[i]), **kw)

        return run_workers(n, len(self.engines), item, setup=setup, teardown=lambda k: self.streams[k].synchronize())


def _pipeline_transcribe_continuous(self, mels, slots: int = 8, chunk: int = 8, block: int = 64,
                                    force_eos_steps: Optional[Sequence[int]] = None, max_length=None) -> List[Any]:
    """Continuous decoding of `mels` ([N, n_mels, 2*S] CUDA tensor or list of rows) in ARRIVAL order: every worker takes blocks of `block`
    utterances and runs them through its own continuous stream (`transcribe_continuous`: `slots` rows busy, per-utterance stop, slots
    refilled on the device).  Returns N numpy id rows (start token through EOS) in input order."""
    import torch
    n = len(mels)
    blocks = [(a, min(a + block, n)) for a in range(0, n, block)]
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(self.device))

    def setup(k: int):
        torch.cuda.set_device(self.device)
        self.streams[k].wait_event(ready)

    def item(k: int, j: int):
        a, b = blocks[j]
        enc, dec = self.engines[k]
        with torch.cuda.stream(self.streams[k]):
            return transcribe_continuous(enc, dec, mels[a:b], slots=slots, chunk=chunk, max_length=max_length,
                                         force_eos_steps=None if force_eos_steps is None else force_eos_steps[a:b])

    parts = run_workers(len(blocks), len(self.engines), item, setup=setup, teardown=lambda k: self.streams[k].synchronize())
    return [row for part in parts for row in part]


WhisperPipeline.transcribe_continuous = _pipeline_transcribe_continuous


def run_workers(n_items: int, n_workers: int, item, setup=None, teardown=None) -> List[Any]:
    """Host side of `WhisperPipeline.transcribe` (no GPU in here): `n_workers` threads take item indices 0 .. n_items-1 from a shared
    counter (a worker takes the next item when it is done with its own: dynamic, not round-robin), `item(worker, index)` produces
    result[index]; `setup(worker)` / `teardown(worker)` run once per thread.  The first exception stops the hand-out and is re-raised
    in the caller's thread after every worker has returned."""
    import itertools
    import threading
    results: List[Any] = [None] * n_items
    errors: List[BaseException] = []
    counter, lock = itertools.count(), threading.Lock()

    def work(k: int):
        try:
            if setup is not None:
                setup(k)
            while not errors:
                with lock:
                    i = next(counter)
                if i >= n_items:
                    break
                results[i] = item(k, i)
            if teardown is not None:
                teardown(k)
        except BaseException as exc:   # surfaced in the caller's thread below
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(max(1, min(n_workers, n_items)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return results
