/*
 * whisper_trtllm_amd.h — C-ABI of the MI355X-native Whisper encoder/decoder engine.
 *
 * This is the drop-in boundary for the hot path of EdVince/whisper-trtllm
 * (tensorrt_llm/models/whisper/model.py + examples/whisper/run.py).  The reference crosses the
 * process→device boundary through TensorRT's execution context, wrapped by
 *   tensorrt_llm/runtime/session.py:54   Session.from_serialized_engine(bytes)
 *   tensorrt_llm/runtime/session.py:116  Session.infer_shapes(List[TensorInfo]) -> List[TensorInfo] | None
 *   tensorrt_llm/runtime/session.py:148  Session.run(inputs, outputs, stream) -> bool   (async enqueue)
 * and its only native C symbol is `initLibNvInferPlugins` (cpp/tensorrt_llm/plugins/api/InferPlugin.cpp:151),
 * loaded with ctypes.CDLL in tensorrt_llm/plugin/plugin.py:10-22.  TensorRT does not exist on ROCm, so the
 * C-ABI below is shaped like Session: an opaque engine handle built from a serialized blob, shape inference
 * by tensor name, and a stream-ordered run with name -> device-pointer bindings.  Entry points (5)-(9) add
 * the batched in-place-KV fast path that replaces run.py's per-token Session.run + clone loop.
 *
 * Conventions
 *   - every function returns 0 on success or a negative WT_E_* code; nothing throws across the ABI;
 *     `wt_last_error()` returns a thread-local human-readable message for the last failure.
 *   - the caller owns every I/O buffer (device pointers, e.g. torch tensors); the engine owns weights,
 *     workspace and the resident KV cache.  No torch types appear in any signature.
 *   - calls are stream-ordered on the `hipStream_t` passed as `void* stream`; only wt_decoder_poll and
 *     wt_decoder_greedy synchronise (documented below).  First use with a new batch size allocates workspace.
 *   - every call runs on its handle's device and restores the caller's current device before returning.
 *   - a handle is NOT thread-safe (matches one IExecutionContext per Session, session.py:48); distinct handles --
 *     on different devices or several on ONE device -- may be driven concurrently from different host threads
 *     (the Python side's WhisperPipeline runs N engine pairs per GPU that way; the library's lazily latched
 *     state is atomic / initialised once).
 */
#ifndef WHISPER_TRTLLM_AMD_H
#define WHISPER_TRTLLM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WT_ABI_VERSION 3

/* error codes */
#define WT_OK 0
#define WT_E_INVALID (-22)   /* bad argument / malformed blob / shape or dtype mismatch */
#define WT_E_NOMEM (-12)     /* device or host allocation failed */
#define WT_E_NOTFOUND (-2)   /* unknown tensor name */
#define WT_E_HIP (-5)        /* a HIP runtime call failed; message carries hipGetErrorString */
#define WT_E_UNSUPPORTED (-38)
#define WT_E_STATE (-1)      /* call sequence violated (e.g. steps before begin) */

/* tensor element types (numbering is ours; the Python shim maps trt.float32 etc. onto it) */
typedef enum { WT_F32 = 0, WT_F16 = 1, WT_I32 = 2, WT_I8 = 3 } wt_dtype;
typedef enum { WT_KIND_ENCODER = 1, WT_KIND_DECODER = 2 } wt_engine_kind;

#define WT_MAX_DIMS 6
#define WT_NAME_LEN 48

/* == TensorInfo(name, dtype, shape) of session.py:28-33 */
typedef struct {
    char name[WT_NAME_LEN];
    int32_t dtype; /* wt_dtype */
    int32_t ndim;
    int64_t shape[WT_MAX_DIMS];
} wt_tensor_desc;

/* one entry of the inputs/outputs dict of Session.run (session.py:166-176): name -> device pointer */
typedef struct {
    const char* name;
    void* ptr;
} wt_binding;

typedef struct wt_engine wt_engine;

/* model hyper-parameters baked into the blob (HF config keys, build_encoder.py:48-56 / build_decoder.py:45-56) */
typedef struct {
    int32_t kind;      /* wt_engine_kind */
    int32_t precision; /* wt_dtype of the GEMM / GEMV weight operands: WT_F32, or WT_F16 (--engine_precision float16, builder.py:55;
                          accumulation, LayerNorm, softmax, residual stream and every Session-visible tensor stay fp32) */
    int32_t d_model, n_heads, n_layers, ffn_dim;
    int32_t n_mels, max_source_positions, max_target_positions, vocab_size;
} wt_engine_info;

/* (1) replaces Session.from_serialized_engine (session.py:54): parse the blob, upload weights to `device`.
 * Blobs are versioned (engine_pack.py VERSION); a blob written by another version is refused with WT_E_UNSUPPORTED. */
int wt_engine_open(const void* blob, size_t nbytes, int device, wt_engine** out);
/* (1b) a second handle on the SAME weights (TensorRT: one ICudaEngine, several IExecutionContexts -- session.py:48 creates one per
 * Session): the read-only weight payload is shared and reference-counted, workspace / resident caches / step graphs are the new
 * handle's own.  Lets N host threads drive N decodes on one device (distinct handles may run concurrently) at the cost of one copy
 * of the weights.  The payload is freed when the last handle sharing it is closed, in any order. */
int wt_engine_clone(const wt_engine* src, wt_engine** out);
/* (2) engine teardown (TensorRT: ICudaEngine/IExecutionContext destructors). */
void wt_engine_close(wt_engine* e);
int wt_engine_get_info(const wt_engine* e, wt_engine_info* out);
/* How an fp32 engine forms its large matrix products: 0 = v_mfma_f32_32x32x2_f32 (the fp32 matrix instruction), 1 = "x3": every
 * fp32 operand exactly split into three bf16 values (x = b1 + b2 + b3 to 2^-24 relative), the product accumulated in fp32 from the six
 * partial products of order <= 2^-16 on v_mfma_f32_32x32x16_bf16; the dropped ones are each up to 2^-24 |a||w| in the worst case, about
 * 2^-23 per product.  On random operands it is measured as accurate as the fp32 instruction; on a sum that grows coherently (all products
 * of one sign) its accumulation error grows faster with K: 3.7e-6 of sum |a||w| against the fp32 instruction's 4.2e-7 at K = 4096
 * (tests/test_gpu_kernels.py::test_gemm_x3_is_an_fp32_gemm).  16 / 6 = 2.7x the fp32 instruction's peak.  The default for fp32 engines;
 * fp16 engines report 0. */
int wt_engine_gemm_mode(const wt_engine* e);

/* (3) replaces Session.infer_shapes (session.py:116-146): check names/dtypes of the inputs, remember the
 * input shapes for the next run, and report the outputs.  `*n_out` is in: capacity of `out`, out: count.
 * Encoder  in : data f32 [B,n_mels,2*S], length f32 [B] (ignored)            out: hidden_states f32 [B,S,d]
 * Decoder  in : data i32 [1,1], length i32 [1] (ignored), encoder_hidden_states f32 [1,S,d],
 *               self_past_key/value f32 [L,H,s,64], cross_past_key/value f32 [L,H,S,64],
 *               past_self_cache_mask f32 [m_s], past_cross_cache_mask f32 [m_c]  (only the LENGTHS are read)
 *          out: hidden_states f32 [1,1,V] (logits), next_self_keys/values f32 [L,H,min(m_s-1,s)+1,64],
 *               next_cross_keys/values f32 [L,H,S,64]            (model.py:474-516, :459-468) */
int wt_engine_infer_shapes(wt_engine* e, const wt_tensor_desc* in, int n_in, wt_tensor_desc* out, int* n_out);

/* (4) replaces Session.run (session.py:148-178) == context.execute_async_v3(stream): enqueue one engine
 * execution with the shapes of the last wt_engine_infer_shapes call.  Asynchronous: 0 != finished. */
int wt_engine_run(wt_engine* e, const wt_binding* in, int n_in, const wt_binding* out, int n_out, void* stream);

/* (5) batched encoder: mel f32 [batch, n_mels, 2*S] -> hidden f32 [batch, S, d].  Asynchronous. */
int wt_encoder_forward(wt_engine* enc, const float* mel, int batch, float* hidden_out, void* stream);

/* greedy-search rules == get_logits_processor / get_stopping_criteria of run.py:150-169 */
typedef struct {
    int32_t decoder_start_token_id;
    int32_t eos_token_id;
    int32_t pad_token_id;
    int32_t max_length;               /* MaxLengthCriteria: stop when len >= max_length */
    int32_t begin_index;              /* SuppressTokensAtBeginLogitsProcessor.begin_index */
    const int32_t* suppress_tokens;   /* host pointers, copied at begin */
    int32_t n_suppress_tokens;
    const int32_t* begin_suppress_tokens;
    int32_t n_begin_suppress_tokens;
    const int32_t* forced_decoder_ids; /* n_forced pairs (generation index, token id) */
    int32_t n_forced;
    int32_t force_eos_step;           /* bench only: emit EOS at this 0-based step for every row; -1 = off */
    float* logits_trace;              /* optional device buffer f32 [batch, max_length-1, V] of raw logits, or NULL */
    const int32_t* force_eos_steps;   /* bench only: host array [batch], row b emits EOS at 0-based step force_eos_steps[b]
                                         (< 0: never) -- the variable-length workload of bench.py; NULL = off */
} wt_greedy_params;

/* (6) start a greedy decode of `batch` utterances (1 <= batch <= 16 per call, WT_E_UNSUPPORTED above; shard larger
 * batches over calls or GPUs): project the encoder memory f32 [batch,S,d] into the
 * resident cross-KV cache, reset the self-KV cache and the id buffer to [[decoder_start_token_id]]*batch.
 * Replaces greedy_search() step 0 (run.py:171-197 with past_key_values=None).  An fp16 engine keeps these RESIDENT caches in fp16
 * (they never leave the engine; the by-value caches of wt_engine_run stay f32 like the reference's, model.py:464-468).
 * Asynchronous when the token rules
 * (suppress / begin-suppress / forced lists) equal those of the previous decode on this handle; a changed rule set is
 * uploaded and the stream synchronised once. */
int wt_decoder_begin(wt_engine* dec, const float* enc_hidden, int batch, const wt_greedy_params* p, void* stream);
/* (7) enqueue `n_steps` decoder steps (token embed -> L layers -> vocab projection -> logits processors ->
 * argmax -> pad/EOS bookkeeping -> append), all on device.  Steps after every row finished are no-ops.
 * Replaces the body of run.py:195-217.  Asynchronous. */
int wt_decoder_steps(wt_engine* dec, int n_steps, void* stream);
/* (8) synchronise `stream` and report progress: current sequence length (prompt included), number of
 * unfinished rows, and whether the stop test of run.py:219-226 has fired. */
int wt_decoder_poll(wt_engine* dec, int* cur_len, int* n_unfinished, int* done, void* stream);
/* (8b) run the decode in flight to its stop test (run.py:195-226): enqueues steps one at a time, keeping `lookahead` steps queued
 * behind the one the GPU is executing (0 = engine default: 1 for the large models, 3 when a step is < ~0.3 ms), and follows the
 * progress through a pinned host word the last kernel of every step writes -- no stream synchronisation, no idle GPU between
 * chunks, and at most `lookahead` steps enqueued past the stop (they are no-ops for the token state).  Returns once the stop test
 * has been OBSERVED; the surplus steps may still be draining, so follow it with stream-ordered calls (wt_decoder_read_ids).
 * `*cur_len` = final sequence length (prompt included), `*n_unfinished` = rows that never produced EOS. */
int wt_decoder_run(wt_engine* dec, int lookahead, int* cur_len, int* n_unfinished, void* stream);
/* copy the generated ids (int32 [batch, cur_len], row-major) into a DEVICE buffer of capacity
 * batch*max_length int32; stream-ordered. */
int wt_decoder_read_ids(wt_engine* dec, int32_t* ids_out, int ld, void* stream);
/* (9) convenience: begin + wt_decoder_run; writes ids int32 [batch, max_length] (row stride
 * max_length) to DEVICE memory and the final length to *out_len.  Synchronises the stream. */
int wt_decoder_greedy(wt_engine* dec, const float* enc_hidden, int batch, const wt_greedy_params* p,
                      int32_t* ids_out, int* out_len, void* stream);

/* (9b) timestamp mode of the batch decode (wt_decoder_begin / _steps / _run / _greedy): Whisper predicts <|t|> tokens
 * (timestamp_begin + i = i x 0.02 s) under one more logits processor after Suppress -> SuppressAtBegin -> Force, the rules of
 * WhisperTimeStampLogitsProcessor (transformers generation/logits_process.py), per row at sequence length cur_len (prompt included):
 *   1. <|notimestamps|> is always masked;
 *   2. at cur_len == begin_index - 1 the token is timestamp_begin (<|0.00|>);
 *   3. of the ids from begin_index on, a timestamp after a timestamp (or as the first one) is followed by text: [timestamp_begin, V)
 *      masked; a timestamp after text by a timestamp or EOS: [0, eos_token_id) masked;
 *   4. at cur_len == begin_index with max_initial_timestamp_index >= 0: ids above timestamp_begin + max_initial_timestamp_index masked;
 *   5. if logsumexp(scores[timestamp_begin:]) > max(scores[:timestamp_begin]), every text id is masked;
 * then the argmax (lowest index on ties, NaN-aware) and the usual pad / EOS / max_length bookkeeping.  The setting applies from the
 * next wt_decoder_begin on this handle; t == NULL or t->enabled == 0 turns it off.  WT_E_INVALID unless 0 < timestamp_begin < V,
 * 0 <= no_timestamps_token_id < timestamp_begin and begin_index >= 2; wt_decoder_begin refuses (WT_E_INVALID) a forced list that
 * holds no_timestamps_token_id or a forced position >= begin_index - 1, and wt_decoder_stream_begin refuses (WT_E_UNSUPPORTED) while
 * the mode is on.  The logits pass through HBM in this mode (one more launch per step than the fused greedy argmax). */
typedef struct {
    int32_t enabled;
    int32_t no_timestamps_token_id;
    int32_t timestamp_begin;               /* first timestamp id (<|0.00|>); ids >= it are timestamps */
    int32_t begin_index;                   /* sequence length at which the first generated timestamp is followed (.en: 2) */
    int32_t max_initial_timestamp_index;   /* < 0: no cap on the first timestamp */
} wt_timestamp_params;
int wt_decoder_set_timestamp_rules(wt_engine* dec, const wt_timestamp_params* t);

/* (9c) beam search for the batch decode (wt_decoder_begin / _steps / _run / _greedy), on the device: the semantics of transformers'
 * beam_search (generation/utils.py) with BeamSearchScorer / BeamHypotheses (generation/beam_search.py), one beam group and one returned
 * hypothesis per utterance.  Per step: log_softmax over the whole vocabulary first, then Suppress -> SuppressAtBegin -> Force on the
 * log-probabilities, plus the running beam score (0 for beam 0, -1e9 for the others at the start); per utterance the 2 * num_beams best
 * of the num_beams * V candidates in order (lowest flat index first among equals); an EOS candidate of rank < num_beams becomes a
 * finished hypothesis (score = sum of log-probabilities / length ** length_penalty, the length without the EOS), the first num_beams
 * others are the next beams; an utterance is done when its store is full and (early_stopping, or its worst kept score >= best candidate
 * score / (cur_len + 1) ** length_penalty).  A NaN logit ranks first and is left out of its row's log-sum-exp; a row without any finite
 * logit has a NaN log-sum-exp and only NaN / -inf candidates.  Among hypotheses of exactly equal score the returned one is unspecified
 * (the engine takes the highest store slot, the reference the last of a stable sort).
 * The setting applies from the next wt_decoder_begin on this handle; b == NULL or num_beams <= 1 turns it off.  With it on,
 * wt_decoder_begin(batch = utterances) decodes batch * num_beams rows: WT_E_UNSUPPORTED when that exceeds 16, when num_beams > 8, for
 * early_stopping outside {0, 1}, together with timestamp mode, logits_trace or force_eos_step(s), and from wt_decoder_stream_begin.
 * wt_decoder_poll / _run report the beam stop test (every utterance done, or max_length); wt_decoder_read_ids returns the best
 * hypothesis per utterance [batch][max_length] (EOS behind it when it fits, then pad_token_id), wt_decoder_read_beam_scores its score
 * (device float [batch]; both are stream-ordered and may be called at any point of the decode). */
typedef struct {
    int32_t num_beams;
    float length_penalty;
    int32_t early_stopping;    /* 0: the heuristic of early_stopping=False, 1: stop at num_beams finished hypotheses */
} wt_beam_params;
int wt_decoder_set_beam_search(wt_engine* dec, const wt_beam_params* b);
int wt_decoder_read_beam_scores(wt_engine* dec, float* scores_out, void* stream);

/* (9d) token-level timestamps for the batch decode (wt_decoder_begin / _steps / _run / _greedy): transformers'
 * WhisperForConditionalGeneration._extract_token_timestamps (cross-attention weights of the alignment heads -> normalisation over the
 * tokens -> median filter along the frames -> mean over the heads -> dynamic time warping), on the device.  With the mode on, the
 * cross-attention launches of the listed (layer, head) pairs also store their finished query per row and step (fp32, n_heads x rows x
 * (max_length - 1) x 64 floats, allocated by wt_decoder_begin), and every row keeps stepping on pad input after its EOS, as the
 * reference's rows do: those steps are part of the alignment.  wt_decoder_read_token_timestamps then runs the post-pass over that
 * history and the resident cross-K cache, stream-ordered: with N = cur_len - 1 steps (the batch-wide length, for every row, as the
 * reference) and S encoder frames, per utterance W = softmax(q K^T) per head [N][S] in fp32, (W - mean) / std over the tokens (population
 * std; a single token gives NaN as in the reference), a median of `median_filter_width` along the frames with reflect padding (the input
 * unchanged when S <= width / 2), the mean over the heads, DTW on the negated matrix (fp32 cost, ties resolved as
 * _dynamic_time_warping does), and out[b][0] = 0, out[b][1 + k] = time_precision x the frame at which the path reaches token k; entries
 * from cur_len on are 0.  `out` is DEVICE float [batch][ld], ld >= max_length; call it before the next wt_decoder_begin.
 * The setting applies from the next wt_decoder_begin on this handle; t == NULL or n_heads <= 0 turns it off, and the engine then enqueues
 * exactly what it did before.  WT_E_INVALID for a (layer, head) outside the model or listed twice, more than 32 heads, or a width that is
 * not odd in [1, 15]; wt_decoder_begin refuses (WT_E_UNSUPPORTED) the mode together with beam search (it would need beam_indices), and
 * wt_decoder_stream_begin refuses it.  It combines with the timestamp mode (9b) and with force_eos_step(s). */
typedef struct {
    int32_t n_heads;
    const int32_t* heads;            /* host pointer, n_heads pairs (layer, head); copied by the call */
    int32_t median_filter_width;     /* odd, 1 .. 15 (transformers' default: 7) */
    double time_precision;           /* seconds per encoder frame (Whisper: 0.02) */
} wt_token_timestamp_params;
int wt_decoder_set_token_timestamps(wt_engine* dec, const wt_token_timestamp_params* t);
int wt_decoder_read_token_timestamps(wt_engine* dec, float* out, int ld, void* stream);

/* (9e) token log-probabilities for the batch decode (wt_decoder_begin / _steps / _run / _greedy), on the device and without another
 * launch: the log-sum-exp of a step's scores is carried beside the running argmax of the vocabulary projection, so the logits still never
 * reach memory.  With s = the step's scores after every processor it applies (Suppress -> SuppressAtBegin -> Force -> the timestamp rules
 * in timestamp mode), the step that writes position t of row b stores token_logprob[b][t] = s[tok] - logsumexp(s) over the entries that
 * are not -inf (transformers' compute_transition_scores(normalize_logits=True)): exactly 0 at a forced position (forced_decoder_ids and
 * the timestamp mode's <|0.00|>), NaN when a surviving score is NaN, the EOS score of the step where force_eos_step(s) replaced the token.
 * Position 0 and the positions behind a row's EOS are 0; the EOS itself is scored.  sum_logprob[b] is the fp32 sum of the row's entries
 * through its EOS, accumulated in step order (openai-whisper's avg_logprob = sum_logprob / number of scored positions).  With
 * no_speech_token_id >= 0, no_speech_prob[b] = softmax(raw logits of step 0)[no_speech_token_id], over the UNPROCESSED logits of the
 * step whose input is the start token (-1: off).
 * wt_decoder_read_logprobs copies them out, stream-ordered, at any point of the decode: token_logprobs DEVICE float [batch][ld], ld >=
 * max_length; sum_logprob DEVICE float [batch]; no_speech_prob DEVICE float [batch] or NULL.  WT_E_STATE without a decode in this mode.
 * The setting applies from the next wt_decoder_begin on this handle (which clears the buffers); p == NULL or enabled == 0 turns it off,
 * and the engine then enqueues exactly what it did before.  WT_E_INVALID for a no_speech_token_id outside [-1, V); wt_decoder_begin refuses
 * (WT_E_UNSUPPORTED) the mode together with beam search (wt_decoder_read_beam_scores is its score), and wt_decoder_stream_begin refuses
 * it.  It combines with the timestamp mode (9b), token-level timestamps (9d), logits_trace and force_eos_step(s). */
typedef struct {
    int32_t enabled;
    int32_t no_speech_token_id;      /* -1: no no_speech_prob */
} wt_logprob_params;
int wt_decoder_set_logprobs(wt_engine* dec, const wt_logprob_params* p);
int wt_decoder_read_logprobs(wt_engine* dec, float* token_logprobs, int ld, float* sum_logprob, float* no_speech_prob, void* stream);

/* (9f) temperature sampling for the batch decode (wt_decoder_begin / _steps / _run / _greedy), on the device, where the argmax lives: the
 * logits still never reach memory.  A draw from softmax(s / T) is argmax_v (s[v] / T + g[v]) with independent standard Gumbel noise g
 * (the Gumbel-max identity), so the vocabulary projection's argmax epilogue, the select kernels and the finish kernel keep their
 * structure and compare a key instead of a score.  With s = the step's scores after every processor it applies (Suppress ->
 * SuppressAtBegin -> Force -> the timestamp rules), the row b that writes sequence position t (its current length, prompt included) takes
 *   x   = Philox4x32-10(counter = (v >> 2, t, 0, 0), key = (seed[b] & 0xffffffff, seed[b] >> 32))[v & 3]
 *   u   = ((x >> 9) + 0.5) * 2^-23            (exact in fp32, strictly inside (0, 1))
 *   key = s[v] / T + (-logf(-logf(u)))        (fp32; s / T is transformers' TemperatureLogitsWarper)
 * and the token is the NaN-aware argmax of key, the lowest id among equals.  -inf stays -inf, a NaN score ranks first as it does in the
 * greedy decode, a forced position yields the forced token.  The generator is counter-based: a draw depends on (seed, position, id)
 * alone -- not on the batch slot, the batch size, the fused or non-fused path or the order of anything -- and is bitwise repeatable.  In
 * timestamp mode (9b) the rules use the unperturbed scores (the timestamps' log-sum-exp against the best text score, the forced <|0.00|>)
 * and the token is the best key among the ids the rules leave.
 * A sampled decode runs with the log-probability mode (9e) on, whether or not wt_decoder_set_logprobs asked for it, and its entries are
 * those of the UNTEMPERED scores: token_logprob = s[tok] - logsumexp(s), openai-whisper's definition (GreedyDecoder.update takes
 * log_softmax(logits) and samples from logits / temperature).
 * seeds: n_seeds 64-bit row seeds (host pointer, copied by the call), or NULL: row b uses seed + b.
 * The setting applies from the next wt_decoder_begin on this handle; p == NULL or temperature <= 0 turns it off, and the engine then
 * enqueues exactly what it did before.  WT_E_INVALID for a temperature that is not finite; wt_decoder_begin returns WT_E_INVALID when the
 * seed list is shorter than its batch, refuses (WT_E_UNSUPPORTED) sampling together with beam search, and wt_decoder_stream_begin refuses
 * it.  It combines with the timestamp mode (9b), token-level timestamps (9d), the log-probability mode (9e), logits_trace and
 * force_eos_step(s).  One temperature per call; no top-k / top-p warpers, no best_of. */
typedef struct {
    float temperature;            /* <= 0: sampling off (greedy) */
    const uint64_t* seeds;        /* host pointer [batch of the next begin], copied by the call; NULL: seed + row */
    int32_t n_seeds;
    uint64_t seed;
} wt_sampling_params;
int wt_decoder_set_sampling(wt_engine* dec, const wt_sampling_params* p);

/* (9g) decoder prompts (transformers' generate(prompt_ids=...), openai-whisper's initial_prompt / condition_on_previous_text): `len`
 * tokens in front of decoder_start_token_id, the first of them <|startofprev|>.  Row b of the id buffer then starts as
 * prompt[b][0..len), decoder_start_token_id, and wt_decoder_begin runs positions 0..len-1 of every row through all decoder layers in
 * ONE pass, the prefill: GEMMs over batch * len rows and a causal attention kernel instead of len dependent decode steps.  It writes
 * the prompt's keys and values into rows 0..len-1 of the resident self caches and leaves the decode at cur_len = len + 1 with the start
 * token at position len as the input of step 0; no vocabulary projection runs for prompt positions.  The step loop is what it was:
 * every rule keys on the absolute sequence length, so ALL positions of wt_greedy_params and wt_timestamp_params (begin_index,
 * forced_decoder_ids, the timestamp rules' begin_index) stay absolute sequence positions -- the caller shifts them by len -- and
 * max_length counts the prompt, as in transformers.  Step 0 is still the step whose input is the start token: no_speech_prob (9e) keeps
 * its meaning, sampling (9f) draws at the absolute positions.  wt_decoder_read_ids returns whole rows, prompt included; the
 * log-probability entries (9e) of positions 0..len are 0.
 * ids: host pointer, row-major [n_rows][len], copied by the call.  n_rows == 1: every row of the next decode uses row 0; else n_rows
 * must be >= that decode's batch.  One prompt length per call.
 * The setting applies from the next wt_decoder_begin on this handle; p == NULL or len <= 0 turns it off, and wt_decoder_begin then
 * enqueues exactly what it did before.  WT_E_INVALID for a token outside the vocabulary; wt_decoder_begin returns WT_E_INVALID when
 * n_rows is neither 1 nor >= its batch or when len + 2 > max_length, and refuses (WT_E_UNSUPPORTED) a prompt on an fp16 decoder engine,
 * together with beam search (9c) and together with token-level timestamps (9d: their history is indexed by step and sized by the
 * sequence length); wt_decoder_stream_begin refuses (WT_E_UNSUPPORTED) while a prompt is set.  It combines with the timestamp mode
 * (9b), the log-probability mode (9e) and sampling (9f). */
typedef struct {
    const int32_t* ids;   /* host, row-major [n_rows][len]; copied by the call */
    int32_t n_rows;       /* 1: every row of the next decode uses row 0; else must be >= that decode's batch */
    int32_t len;          /* tokens placed BEFORE decoder_start_token_id, 0 < len */
} wt_prompt_params;
int wt_decoder_set_prompt(wt_engine* dec, const wt_prompt_params* p);   /* NULL or len <= 0: off */
/* (9h) per-row prompt lengths (several recordings under condition_on_previous_text carry different amounts of previous text): row b
 * holds lens[b] prompt tokens, 0 <= lens[b] <= ld.  With Lmax = the longest row of the decode's batch, row b of the id buffer starts as
 * pad_token_id x (Lmax - lens[b]), prompt[b][0..lens[b]), decoder_start_token_id -- left-padded, as transformers pads decoder_input_ids
 * -- and the decode begins at cur_len = Lmax + 1 for EVERY row, so all of (9g)'s absolute positions are shifted by Lmax and max_length
 * counts Lmax; the row's decoder position and the valid keys of its self cache are its own lens[b] (a row with lens[b] == 0 starts at
 * position 0 as an unprompted row does), and sampling (9f) draws at the row's own position lens[b] + 1 + generated tokens, so a row's
 * draws do not depend on its neighbours' prompts.  The prefill runs once over batch x Lmax positions with the rows right-padded;
 * causality keeps the filler from every real position, and each decode step overwrites its cache row before attention reads it.
 * wt_decoder_read_ids returns the left-padded rows; the log-probability entries (9e) of positions 0..Lmax are 0.
 * ids host row-major [n_rows][ld], lens[n_rows] in [0, ld]; copied by the call.  n_rows >= the next decode's
 * batch.  max(lens) == 0 or ids == NULL: off.  Same refusals as wt_decoder_set_prompt (fp16 decoder engine, beams, token-level
 * timestamps, the continuous mode); wt_decoder_set_prompt and this call replace each other.  With every lens[b] equal the decode is
 * bitwise the one wt_decoder_set_prompt gives. */
int wt_decoder_set_prompt_rows(wt_engine* dec, const int32_t* ids, int n_rows, int ld, const int32_t* lens);

/* (9i) language detection and per-row language tokens (openai-whisper's detect_language; multilingual checkpoints whose forced list is
 * [[1, <|xx|>], [2, task], ...]).  lang_ids: the n_lang language token ids (1..128, any order, distinct, inside the vocabulary, none the
 * EOS id).  With the mode on, the token appended at the language position -- the sequence position behind decoder_start_token_id, prompt
 * length + 1, the same for every row also behind per-row prompts (9h) -- is the ROW'S OWN instead of forced_decoder_ids' batch-wide one:
 * row_tok[b] when that is one of lang_ids, and where it is negative (or row_tok == NULL: every row) the language the model detects.
 * Detection is a rule of the first step: its final hidden state is the one detect_language computes from the start token alone, so a
 * small kernel beside the vocabulary projection takes the logits of lang_ids only (the suppress lists do not apply), their softmax and
 * the argmax (ties: the lowest id; a NaN row: NaN probabilities and the lowest listed id) -- no extra decoder pass.  The position counts
 * as forced: log-probability (9e) exactly 0, no draw (9f).  Only the first step of a decode with a row to detect launches the kernel;
 * every other step, and every step with the mode off, is what it was.
 * wt_decoder_read_languages copies out, stream-ordered, behind the first step: tok DEVICE i32 [batch] (the rows' language tokens) and prob
 * DEVICE f32 [batch][n_lang] (softmax over lang_ids, in their order; all 0 when no row was left to detect); either may be NULL.
 * lang_ids / row_tok: host pointers, copied by the call; row_tok holds n_rows >= the next decode's batch entries.  n_lang <= 0 or
 * lang_ids == NULL: off.  The setting applies from the next wt_decoder_begin on this handle, which returns WT_E_INVALID for ids outside
 * the rules above, a row entry that is not listed, too few rows, or a language position at or behind the timestamp rules' begin_index - 1,
 * and refuses (WT_E_UNSUPPORTED) the mode together with beam search (9c) and token-level timestamps (9d); wt_decoder_stream_begin
 * refuses it.  It combines with the timestamp mode (9b), log-probabilities (9e), sampling (9f) and prompts (9g, 9h); fp32 and fp16 engines. */
int wt_decoder_set_languages(wt_engine* dec, const int32_t* lang_ids, int n_lang, const int32_t* row_tok, int n_rows);
int wt_decoder_read_languages(wt_engine* dec, int32_t* tok, float* prob, void* stream);

/* ---- (10) continuous decoding: every utterance stops at its own EOS and its decode slot is refilled at once.
 * The reference gets per-utterance stopping from transcribing one clip at a time (examples/whisper/run.py:219-226; dataset loop
 * cal_wer.py:249-287); a batch started by wt_decoder_begin runs to its longest row.  Here `slots` rows (1..16) stay busy: utterances
 * are submitted ahead of time (their cross K/V projected into a free row of a cache POOL of `pool_rows` rows, <= 256; 0 = 4 x slots),
 * wait in a device-side queue, and the kernel that sees a row emit EOS (or reach max_length) puts the next waiting utterance into that
 * slot within the same step.  Ids of every utterance equal those of the same utterance decoded alone.  Finished utterances are
 * reported through pinned host memory: no device-to-host copy, no stream synchronisation.  logits_trace / force_eos_step(s) of `p`
 * must be unset.  One stream per handle; wt_decoder_begin on the handle ends it. */
int wt_decoder_stream_begin(wt_engine* dec, int slots, int pool_rows, const wt_greedy_params* p, void* stream);
/* submit `n` (1..16) more utterances: enc_hidden f32 [n,S,d] on the device (consumed stream-ordered by this call's K/V projection).
 * `force_eos_steps` (bench only, NULL = off): utterance i emits EOS at its own 0-based step force_eos_steps[i].  handles[i] receives
 * the handle to collect utterance i with.  WT_E_STATE when fewer than n cache rows are free (collect finished utterances first).
 * Utterances are admitted to slots in submission order.  Asynchronous. */
int wt_decoder_stream_submit(wt_engine* dec, const float* enc_hidden, int n, const int32_t* force_eos_steps, int32_t* handles, void* stream);
/* enqueue decoder steps (as wt_decoder_run: `lookahead` steps queued behind the running one, progress followed through the pinned
 * mailbox) until every submitted utterance has finished -- or, with min_waiting > 0, until fewer than `min_waiting` submitted
 * utterances are still waiting for a slot, so that the caller can submit more before a slot runs dry.  *n_finished = utterances
 * finished since wt_decoder_stream_begin, *n_waiting = an upper bound of those still waiting, *n_steps = decoder steps enqueued since
 * wt_decoder_stream_begin (each is `slots` row-steps: the denominator of the slot utilisation).  Any of the three may be NULL. */
int wt_decoder_stream_run(wt_engine* dec, int min_waiting, int lookahead, int* n_finished, int* n_waiting, int* n_steps, void* stream);
/* *len = length of utterance `handle` (start token and EOS included) once it has finished, 0 while it waits or decodes.  With ids_out
 * != NULL (HOST memory, capacity `cap` >= *len int32) a finished utterance's ids are copied out and its cache row is released. */
int wt_decoder_stream_collect(wt_engine* dec, int handle, int32_t* ids_out, int cap, int* len);

/* per-phase device timers (hipEvents on the caller's stream) for bench.py's roofline block */
typedef struct {
    float ms_total;    /* sum over launches of the timed kernel since the last reset */
    int64_t launches;
} wt_kernel_timer;
/* enable/disable event timing of the dominant decode kernel (cross-attention) and the encoder GEMM */
int wt_engine_set_profiling(wt_engine* e, int enabled);
int wt_engine_get_timer(wt_engine* e, const char* which, wt_kernel_timer* out);
/* average launch time (us) of the dominant decode kernel, cross-attention, over the engine's resident caches:
 * the L per-layer launches are captured into a hipGraph (as the decode step runs them), replayed `iters` times
 * between two hipEvents on the launch stream.  Needs a decode in flight (wt_decoder_begin).  Synchronises. */
int wt_decoder_time_cross_attention(wt_engine* dec, int iters, float* avg_us, void* stream);
/* the same for any of the seven per-layer launches of a decode step: which = "qkv" (LN + q|k|v GEMV + KV append), "self_attn",
 * "pair" (self out-projection + folded cross query), "cross_attn", "cross_out" (split merge + cross out-projection), "fc1", "fc2".
 * The residual stream is not advanced (every launch reads the buffers as they stand).  Synchronises.  Call it only BETWEEN
 * steps of a decode (after a wt_decoder_poll): the launches overwrite the step scratch (query, attention context, FFN buffer,
 * second residual buffer, split partials and the self-cache row at the current length) -- all of which the next step
 * rewrites before it reads them, so the decode itself is not disturbed. */
int wt_decoder_time_kernel(wt_engine* dec, const char* which, int iters, float* avg_us, void* stream);

/* ---- log-mel front-end: replaces the CPU numpy STFT inside the reference's timed loop,
 * `hf_processor(sample["array"], ...)` run.py:267 == WhisperFeatureExtractor._np_extract_fbank_features
 * (transformers/models/whisper/feature_extraction_whisper.py:94-111).  The host passes the Hann window as fp64 [n_fft] (the
 * reference frames in float64, audio_utils.py:399-401) and the mel filter bank f32 [n_mels][npw] (columns >= n_bins zero, npw =
 * n_bins rounded up to a multiple of 4); the fp64 DFT matrix is built inside.  Windowed DFT and power spectrum run in fp64
 * (v_mfma_f64_16x16x4_f64), like the reference's float64 rfft; features agree with it to ~1e-6. */
typedef struct wt_logmel wt_logmel;
int wt_logmel_create(int device, int n_fft, int hop, int n_mels, int n_frames, const double* window, const float* filters, int npw,
                     wt_logmel** out);
void wt_logmel_destroy(wt_logmel* h);
/* audio f32 [batch][n_in] on the device (n_in samples each; shorter than 30 s = zero-padded, longer = trimmed)
 * -> mel_out f32 [batch][n_mels][n_frames].  Asynchronous on `stream`.
 * Non-finite input follows the reference (np.maximum and ndarray.max propagate NaN): an utterance with a NaN sample, or an Inf one
 * (Inf - Inf in the DFT, 0 * Inf in the mel projection), comes out NaN in every element, and the other utterances of the batch are
 * untouched.  Samples are expected within |x| <= 32768 (int16 range): beyond it the float32 power spectrum can overflow where the
 * reference's float64 one does not. */
int wt_logmel_forward(wt_logmel* h, const float* audio, int batch, int n_in, float* mel_out, void* stream);
/* window b = samples [offsets[b], offsets[b] + n_valid[b]) of the flat device buffer `audio`, zero-padded to the handle's window and
 * reflected at the WINDOW's edges (not into neighbouring audio); offsets / n_valid: host arrays of `batch` entries, copied by the call.
 * Bitwise the result of wt_logmel_forward on a copy of that slice.  n_valid[b] >= 1 (longer than the window = trimmed), offsets[b] >= 0;
 * every window is normalised on its own.  The caller guarantees that the slices lie inside the buffer. */
int wt_logmel_forward_windows(wt_logmel* h, const float* audio, const int64_t* offsets, const int32_t* n_valid, int batch,
                              float* mel_out, void* stream);

const char* wt_last_error(void);
int wt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
