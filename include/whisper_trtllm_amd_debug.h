/*
 * whisper_trtllm_amd_debug.h — kernel-level test hooks of libwhisper_trtllm_amd.so.
 *
 * NOT part of the drop-in boundary (that is whisper_trtllm_amd.h).  These launch one HIP kernel each on
 * caller-provided device buffers so tests/test_gpu_kernels.py can check every kernel against a plain
 * fp32 torch reference at edge shapes (ragged tiles, K tails, every batch-width instantiation).
 * All pointers are device pointers; calls are asynchronous on `stream`; 0 = ok, else see wt_last_error().
 */
#ifndef WHISPER_TRTLLM_AMD_DEBUG_H
#define WHISPER_TRTLLM_AMD_DEBUG_H
#include <stddef.h>

#include "whisper_trtllm_amd.h"   /* wt_timestamp_params */
#ifdef __cplusplus
extern "C" {
#endif

/* C[M][N] = act(A[M][K(lda)] W[N][K]^T + bias) (+ resid); act: 0 none, 1 erf-GELU */
int wt_dbg_gemm(const float* A, int lda, const float* W, const float* bias, const float* resid, float* C, int M, int N,
                int K, int act, void* stream);
/* the same launch from a probe build of the LDS-DMA kernel (K % 16 == 0): every workgroup leaves {HW_ID, XCC_ID, wall clock (100 MHz) at
 * entry, first tile landed, K loop done, stores drained, last store issued, 0} in stamps[workgroup][8] (tools/gemm_stamps.py) */
int wt_dbg_gemm_stamps(const float* A, int lda, const float* W, const float* bias, const float* resid, float* C, int M, int N, int K,
                       int act, long long* stamps, void* stream);
/* fp16 operands (A [M][K(lda)], W [N][K] as IEEE half), fp32 accumulate; C is half when out_half else float */
int wt_dbg_gemm_f16(const void* A, int lda, const void* W, const float* bias, const float* resid, void* C, int M, int N, int K,
                    int act, int out_half, void* stream);
/* the same with the LDS-DMA kernel forced (K % 64 == 0): variant 2 = 128x128 two-stage, 3 = 256x128 three-stage; 0 = by shape */
int wt_dbg_gemm_f16_variant(const void* A, int lda, const void* W, const float* bias, const float* resid, void* C, int M, int N, int K,
                            int act, int out_half, int variant, void* stream);
int wt_dbg_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int d, void* stream);
/* qkv [B*S][3*H*64] -> ctx [B*S][H*64], softmax(QK^T/8)V per head */
int wt_dbg_encoder_attention(const float* qkv, float* ctx, int B, int S, int H, void* stream);
/* same with fp16 qkv / ctx (fp32 scores, softmax and accumulators) */
int wt_dbg_encoder_attention_f16(const void* qkv, void* ctx, int B, int S, int H, void* stream);
/* Y[B][N] = act((X' W^T + bias) * scale) (+ resid); xmode 0: X'=X[B][K], 1: X'=LayerNorm(X).  This hook (and wt_dbg_skinny_f16) covers
 * the plain epilogue (YMODE_PLAIN) only: the argmax epilogue is wt_dbg_vocab_argmax's, the q|k|v cache append wt_dbg_skinny_qkv_append's. */
int wt_dbg_skinny(const float* X, const float* ln_w, const float* ln_b, const float* W, const float* bias,
                  const float* resid, float* Y, int B, int N, int K, int xmode, int act, float scale, void* stream);
/* q [B][H*64] (pre-scaled), k/v cache [B][H][s_cap][64] with the first `len` rows valid -> out [B][H*64];
 * part: scratch [B][H][n_split][68]; cnt: int [B][H], must be zero on entry and is left zero */
int wt_dbg_encoder_attention_occupancy(void);   /* workgroups of enc_attn_kernel per CU as the runtime computes it */
int wt_dbg_gemm_x3(const float* A, const float* W, const float* bias, const float* resid, void* C, int M, int N, int K, int act,
                   void* a_planes, void* w_planes, int flags, void* stream);   /* fp32 GEMM from bf16 MFMAs of exactly split operands; flags: 1 three-plane output, 2 planes already split */
int wt_dbg_encoder_attention_split(const float* qkv, void* ctx_planes, int B, int S, int H, void* stream);   /* context as three bf16 planes [3][B*S][H*64] */
int wt_dbg_encoder_attention_x3(const float* qkv, void* qkv_planes, void* ctx_planes, int B, int S, int H, int skip_split, void* stream);
int wt_dbg_skinny_gelu_in(const float* X, const float* r, const float* t, const float* W, const float* bias, const float* resid, float* Y,
                          int B, int N, int K, void* stream);   /* probe: timing only */
int wt_dbg_decode_attention(const float* q, const float* kcache, const float* vcache, float* part, int* cnt, float* out,
                            int B, int H, int s_cap, int len, int n_split, void* stream);
/* the same with the folded query: `u` [B][H*64] is finished per row as (u - mean(ln_h[b]) * ln_r) * rstd(ln_h[b]) + ln_t
 * (LayerNorm statistics of ln_h [B][H*64], eps 1e-5) before the attention — DESIGN.md §4, builder.py:_fold_cross_query */
int wt_dbg_decode_attention_folded(const float* u, const float* kcache, const float* vcache, float* part, int* cnt, float* out,
                                   const float* ln_h, const float* ln_r, const float* ln_t, int B, int H, int s_cap, int len,
                                   int n_split, void* stream);
/* decode attention with the split merge DEFERRED into the consumer: dec_attn_kernel leaves its n_split >= 2 partials in
 * `part` [B][H][n_split][68] and the out-projection Y = merge(part) . W^T + bias + resid ([B][H*64]) merges them while it
 * stages its activation rows (the cross-attention -> out-projection pair of the decode step) */
int wt_dbg_attention_then_projection(const float* q, const float* kcache, const float* vcache, float* part, const float* W,
                                     const float* bias, const float* resid, float* Y, int B, int H, int s_cap, int len, int n_split,
                                     void* stream);
/* the decode step's self-attention -> pair launch with TWO key splits and the merge deferred into BOTH halves of the pair:
 * a = softmax(q K^T) V over the first `len` cache rows (partials in `part` [B][H][2][68]); h1 = h + Wo.a + bo (Wo [d][d]);
 * u = Wf.[a ; h] + c (Wf [d][2d]) */
int wt_dbg_self_attention_then_pair(const float* q, const float* kcache, const float* vcache, float* part, const float* Wo, const float* bo,
                                    const float* h, float* h1, const float* Wf, const float* c, float* u, int B, int H, int s_cap, int len,
                                    void* stream);
/* two skinny GEMMs in one launch: Ya = Xa . Wa^T + bias_a + resid_a ([B][Na], K = Ka) and
 * Yb = [Xb ; Xb2] . Wb^T + bias_b ([B][Nb], K = Kb = 2 * columns of Xb) */
int wt_dbg_skinny_pair(const float* Xa, const float* Wa, const float* bias_a, const float* resid_a, float* Ya, int Na, int Ka,
                       const float* Xb, const float* Xb2, const float* Wb, const float* bias_b, float* Yb, int Nb, int Kb, int B,
                       void* stream);

/* ---- fp16 decoder engines: IEEE-half weights (`W`, `Wa`, `Wb`) and / or IEEE-half K/V caches; activations, accumulation, LayerNorm,
 * softmax and outputs are fp32.  Arguments as in the fp32 hooks of the same name. */
int wt_dbg_skinny_f16(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, const float* resid, float* Y,
                      int B, int N, int K, int xmode, int act, float scale, void* stream);
/* ln_h / ln_r / ln_t: all null (plain query) or all set (folded query) */
int wt_dbg_decode_attention_f16(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out, const float* ln_h,
                                const float* ln_r, const float* ln_t, int B, int H, int s_cap, int len, int n_split, void* stream);
/* two key splits, merge deferred into the out-projection (half caches, half W) */
int wt_dbg_attention_then_projection_f16(const float* q, const void* kcache, const void* vcache, float* part, const void* W, const float* bias,
                                         const float* resid, float* Y, int B, int H, int s_cap, int len, void* stream);
int wt_dbg_skinny_pair_f16(const float* Xa, const void* Wa, const float* bias_a, const float* resid_a, float* Ya, int Na, int Ka, const float* Xb,
                           const float* Xb2, const void* Wb, const float* bias_b, float* Yb, int Nb, int Kb, int B, void* stream);
/* cross-K/V projection: A half [B][rows_total][H*64] (the first `rows` rows of every utterance), W half [2*H*64][H*64], bias f32 ->
 * K / V caches [B][H][kv_cap][64], rows [seq_off, seq_off + rows), stored as half (out_half) or f32 */
int wt_dbg_gemm_f16_kv(const void* A, int rows_total, const void* W, const float* bias, void* kcache, void* vcache, int B, int rows, int H,
                       int kv_cap, int seq_off, int out_half, void* stream);

/* launch_gemm_x3 with its tile instantiation forced: tile 128 (128x128), 192 (192x256), 256 (256x256), 0 = by shape (as wt_dbg_gemm_x3) */
int wt_dbg_gemm_x3_tile(const float* A, const float* W, const float* bias, const float* resid, void* C, int M, int N, int K, int act,
                        void* a_planes, void* w_planes, int flags, int tile, void* stream);
/* LayerNorm (eps 1e-5) of x [rows][d] written as three bf16 planes [3][rows][d] (b1 = rn(y), b2 = rn(y - b1), b3 = rn(y - b1 - b2)) */
int wt_dbg_layernorm_split(const float* x, const float* w, const float* b, void* planes, int rows, int d, void* stream);

/* The encoder's two convolutions exactly as an fp32 / fp16 engine launches them (the same GemmParams helpers, wt_common.h), mel
 * [B][C][2S] -> out [B][S][d] float: conv1 (k 3, pad 1) + GELU, conv2 (k 3, stride 2, pad 1) + GELU + pos [S][d].
 * mode 0: fp32 MFMA (float weights [d][3C] / [d][3d] in the converter's layout), 1: x3 (the weights given as three bf16 planes each,
 * plane p at + p * d * 3C / d * 3d elements), 2: fp16 (half weights).  tile: x3 only, as wt_dbg_gemm_x3_tile.
 * scratch (wt_dbg_encoder_convs_scratch_bytes): melT at offset 0, c1 at offset c1_off = align_up(n_melT * esz, 256), with
 *   n_melT = B (2S + 2) C + 4 C and n_c1 = B (2S + 2) d + 4 d elements, esz = 6 in mode 1 (three bf16 planes of n elements each,
 *   plane p at + 2 p n bytes), else 4 (mode 0: float; mode 2: half data at the start of the region).  Utterance b's rows sit at
 *   b (2S + 2) + r: row t + 1 holds frame t (melT) / conv1's output at frame t (c1), rows 0 and 2S + 1 are the zero padding.
 * Every call first clears both regions (what the engine does when its workspace grows), then runs the three launches. */
size_t wt_dbg_encoder_convs_scratch_bytes(int B, int C, int S, int d, int mode);
int wt_dbg_encoder_convs(const float* mel, const void* conv1_w, const float* conv1_b, const void* conv2_w, const float* conv2_b, const float* pos,
                         float* out, void* scratch, int B, int C, int S, int d, int mode, int tile, void* stream);
/* One decoder layer's cross-K/V projection as the engine launches it: A f32 [B][rows_total][H*64] (the first `rows` rows of every
 * utterance), W f32 [2*H*64][H*64], bias [2*H*64] -> f32 caches [layer_rows][H][cap][64], utterance b at cache row row0 + b, sequence rows
 * [seq_off, seq_off + rows); nothing else is written.  mode 0: fp32 MFMA, 1: x3 (scratch: A's planes at 0, 6 B rows_total H*64 bytes,
 * then W's planes at the next multiple of 256 bytes, 12 (H*64)^2 bytes); tile as wt_dbg_gemm_x3_tile. */
int wt_dbg_cross_kv(const float* A, int rows_total, const float* W, const float* bias, float* kcache, float* vcache, void* scratch, int B, int rows,
                    int H, int cap, int seq_off, int layer_rows, int row0, int mode, int tile, void* stream);

/* the timestamp mode's two launches (ts_select_kernel + greedy_finish_kernel<true>, exactly as the engine enqueues them) on crafted
 * rows: logits f32 [B][V] (B <= 16), ids int32 [B][max_length] (the row's history; position cur_len[0] is overwritten), cur_len a HOST
 * array [B] with 1 <= cur_len[b] < max_length, t / eos as in wt_timestamp_params / wt_greedy_params (no suppress masks, no forced ids).
 * tok_out int32 [B]: the chosen token; stats_out f32 [B][2]: (logsumexp of the masked timestamp scores, masked text maximum).
 * scratch: wt_dbg_timestamp_select_scratch_bytes(B, V, max_length) bytes.  Synchronises `stream` (the state upload). */
size_t wt_dbg_timestamp_select_scratch_bytes(int B, int V, int max_length);
int wt_dbg_timestamp_select(const float* logits, int B, int V, int32_t* ids, int max_length, const int32_t* cur_len,
                            const wt_timestamp_params* t, int eos, int32_t* tok_out, float* stats_out, void* scratch, void* stream);

/* beam search: the engine's two launches (beam_select_kernel + beam_finish_kernel) and finalize on crafted rows.  logits f32
 * [U * nb][V], beam_scores f32 [U * nb], mask bytes [V] or NULL (bit 0: suppressed, bit 1: suppressed when cur_len == begin_index), ids
 * int32 [U * nb][max_length] (the rows' history, cur_len ids each, 1 <= cur_len < max_length), forced_token < 0: none.  Outputs (device):
 * cand_out int32 [U][16][3]: the sorted 2 * nb candidates (token, source beam, score bits), token -1 = none; next_out int32 [U * nb][4]:
 * (token, source beam, score bits, utterance done) of every row; fin_ids int32 [U][max_length] / fin_scores f32 [U]: finalize after the
 * step.  scratch: wt_dbg_beam_select_scratch_bytes(U, nb, V, max_length) bytes.  Synchronises `stream`. */
size_t wt_dbg_beam_select_scratch_bytes(int U, int nb, int V, int max_length);
int wt_dbg_beam_select(const float* logits, const float* beam_scores, const unsigned char* mask, int U, int nb, int V, const int32_t* ids,
                       int max_length, int cur_len, int begin_index, int forced_token, int eos, int pad, const wt_beam_params* b,
                       int32_t* cand_out, int32_t* next_out, int32_t* fin_ids, float* fin_scores, void* scratch, void* stream);
/* self attention through an ancestry table (dec_attn_kernel's beam instantiation): key s of row b is read from cache row anc[b * s_cap + s]
 * (device int32 [B][s_cap], entries in [0, B)); caches f32 or half (kv_half) [B][H][s_cap][64], unsplit */
int wt_dbg_decode_attention_beam(const float* q, const void* kcache, const void* vcache, const int32_t* anc, float* out, int B, int H, int s_cap,
                                 int len, int kv_half, void* stream);
/* cross attention with rows mapped to shared cache rows (the slot_row form the beam step uses): row b reads cache row slot_row[b] (device
 * int32 [B]) of caches [rows][H][s_cap][64], f32 or half; part / cnt as wt_dbg_decode_attention */
int wt_dbg_decode_attention_rows(const float* q, const void* kcache, const void* vcache, const int32_t* slot_row, float* part, int* cnt, float* out,
                                 int B, int H, int s_cap, int len, int n_split, int kv_half, void* stream);
/* the grouped cross-attention form: caches [B / group][H][s_cap][64], cache row u shared by query rows u * group .. + group - 1, one
 * block per (split, head, u) carrying all of them; group 2 or 4 */
int wt_dbg_decode_attention_grouped(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out, int B, int H,
                                    int s_cap, int len, int n_split, int group, int kv_half, void* stream);
/* Decode attention launched as the step graph launches it (engine.hip, enqueue_layer_part): with `self_len` it reproduces LP_SELF_ATTN --
 * fixed_len = 0, every row's key count read on the device as DecState.self_len[b] + 1 (a batch decode: all rows equal; the continuous
 * mode: every slot at its own position) --, with `fixed_len` > 0 and ln_h / ln_r / ln_t it reproduces LP_CROSS_ATTN (folded query, all
 * rows over fixed_len keys).  Exactly one of the two is given.
 * self_len: HOST int32 [B], 0 <= self_len[b] < s_cap, uploaded into a DecState in `scratch`
 *   (wt_dbg_decode_attention_state_scratch_bytes() bytes; the call then synchronises `stream`), or NULL.
 * alive: device int32 [B] or NULL: the skip-finished-rows graph (rows with alive[b] == 0 leave before they stream K/V; the launch table
 *   has that form for nt = 1 only, with nt = 0 the plain kernel runs and attends every row).
 * slot_row: device int32 [B] or NULL: row b reads cache row max(slot_row[b], 0) of caches [rows][H][s_cap][64]; -1 = idle slot.
 *   Entries outside [-1, rows) are refused (the table is read back and checked before the launch).  Without it rows >= B.
 * kv_half: caches IEEE half; nt: 1 non-temporal K/V loads, 0 default policy (what wt_decoder_begin picks for small steps);
 * n_split 1..16; defer_merge (n_split >= 2): the partials stay in `part` [B][H][n_split][68] for the consumer, no ticket, `out` unused.
 * ln_h / ln_r / ln_t: all NULL (plain query) or all set (folded query).  part / cnt / out as wt_dbg_decode_attention.
 * Returns -22 without launching on any argument outside these ranges (B > 16, a partial LayerNorm set, a length outside the cache, ...). */
size_t wt_dbg_decode_attention_state_scratch_bytes(void);
int wt_dbg_decode_attention_state(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out,
                                  const int32_t* self_len, int fixed_len, const int32_t* alive, const int32_t* slot_row, int rows,
                                  const float* ln_h, const float* ln_r, const float* ln_t, int B, int H, int s_cap, int n_split, int kv_half,
                                  int nt, int defer_merge, void* scratch, void* stream);
/* wt_dbg_self_attention_then_pair as the step graph runs it (LP_SELF_ATTN with two splits and the merge deferred, then LP_PAIR): the key
 * count per row from the device state -- self_len a HOST int32 [B] as above -- or one fixed_len > 0 for all rows (exactly one of the two).
 * half: caches and both weight matrices IEEE half (an fp16 decoder engine), else all float; nt as above (the engine passes one flag to
 * both launches).  scratch: wt_dbg_self_attention_then_pair_state_scratch_bytes() bytes. */
size_t wt_dbg_self_attention_then_pair_state_scratch_bytes(void);
int wt_dbg_self_attention_then_pair_state(const float* q, const void* kcache, const void* vcache, float* part, const void* Wo, const float* bo,
                                          const float* h, float* h1, const void* Wf, const float* c, float* u, const int32_t* self_len,
                                          int fixed_len, int B, int H, int s_cap, int half, int nt, void* scratch, void* stream);
/* a beam decode in flight: the plain logits of the last executed step, device f32 [rows][V] */
int wt_dbg_beam_logits(wt_engine* dec, float* logits_out, void* stream);
/* a beam decode in flight: per executed step and row (token, source beam within the utterance, score bits, utterance done), device int32
 * [steps][rows][4] */
int wt_dbg_beam_trace(wt_engine* dec, int32_t* trace_out, int steps, void* stream);

/* ---- the greedy step's fused launches (tests/test_gpu_select.py), parameterised by the helpers the engine itself launches through
 * (wt_common.h).  Host arrays (`cur_len`, `self_len`, `forced`, `state`, ...) are uploaded into `scratch`; these calls synchronise `stream`. */
/* The vocabulary GEMV, logits[b][n] = X'[b] . W[n] (+ bias[n]): X [B][K] (K % 8 == 0, K <= 1024; xmode 1: LayerNorm with ln_w / ln_b first,
 * as the engine; 0: plain), W [N][K] float or IEEE half (w_half), bias [N] or NULL, w_nt: non-temporal weight loads.
 * fused != 0: the argmax epilogue.  mask bytes [N] (bit 0: suppressed, bit 1: suppressed on rows with cur_len[b] == begin_index), cur_len a
 *   HOST array [B]; every workgroup leaves its masked (max, argmax) per row -- torch.argmax semantics: NaN is the maximum, lowest index on
 *   ties -- in part_val / part_idx [B][parts], parts = wt_dbg_vocab_argmax_parts(B, N, K, w_half) (the launch's workgroup count; workgroup
 *   g owns the rows [g * rpw, (g + 1) * rpw) with rpw = ceil(N / parts) rounded up to the plan's row-group multiple, see the test);
 *   `logits` [B][N] or NULL receives the raw (unmasked) logits, the engine's logits_trace.
 * fused == 0: the plain epilogue the unfused path uses: `logits` [B][N] is the output, mask / parts are not touched.
 * scratch: wt_dbg_vocab_argmax_scratch_bytes() bytes. */
int wt_dbg_vocab_argmax_parts(int B, int N, int K, int w_half);
size_t wt_dbg_vocab_argmax_scratch_bytes(void);
int wt_dbg_vocab_argmax(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, const unsigned char* mask,
                        const int32_t* cur_len, int begin_index, int B, int N, int K, int xmode, int w_half, int w_nt, int fused, float* logits,
                        float* part_val, int32_t* part_idx, void* scratch, void* stream);
/* LayerNorm + fused q|k|v projection of a decoder layer: X [B][d], W [3d][d] float or half, bias [3d] -> q [B][d] = scale * (first third);
 * the k / v thirds are written at sequence row self_len[b] (HOST array [B], 0 <= self_len[b] < s_cap, one position PER ROW) of the caches
 * [B][d / 64][s_cap][64], float or IEEE half (kv_half); nothing else of the caches is written.
 * scratch: wt_dbg_skinny_qkv_append_scratch_bytes() bytes. */
size_t wt_dbg_skinny_qkv_append_scratch_bytes(void);
int wt_dbg_skinny_qkv_append(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* q, void* kcache,
                             void* vcache, const int32_t* self_len, int B, int d, int s_cap, int w_half, int kv_half, int w_nt, float scale,
                             void* scratch, void* stream);
/* The q|k|v launch of the decode step with the residual half of the folded cross-attention query on board (LP_QKV, d <= 1024):
 * wt_dbg_skinny_qkv_append's arguments and outputs, bit for bit, plus uh [B][d] = Wh . X + c over the RAW rows X in the same launch
 * (Wh [d][d] float or half like W: columns [d, 2d) of the folded weight, contiguous; c [d]).
 * scratch: wt_dbg_skinny_qkv_append_scratch_bytes() bytes. */
int wt_dbg_skinny_qkv_hoist(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* q, void* kcache,
                            void* vcache, const int32_t* self_len, const void* Wh, const float* c, float* uh, int B, int d, int s_cap,
                            int w_half, int kv_half, int w_nt, float scale, void* scratch, void* stream);
/* The pair launch that follows it (LP_PAIR): h1 = h + Wo . a + bo and u = Wa . a + uh (Wa [d][d]: columns [0, d) of the folded weight,
 * contiguous; Wo / Wa float or half).  The context comes from a [B][d] or, with a NULL, from the two split partials part [B][d/64][2][68]
 * of a self-attention with the merge deferred.  The pair launch has ONE load policy (non-temporal weight loads), hence no w_nt. */
int wt_dbg_skinny_pair_hoisted(const float* a, const float* part, const void* Wo, const float* bo, const float* h, float* h1, const void* Wa,
                               const float* uh, float* u, int B, int d, int w_half, void* stream);
/* The plain greedy tail as the engine enqueues it: greedy_select_kernel over logits [B][V] (part_val / part_idx NULL), or, with logits NULL,
 * the fused form over precomputed partials part_val / part_idx [B][n_parts] (the vocabulary GEMV's); then greedy_finish_kernel<false>.
 * mask bytes [V] (device), forced a HOST array [max_length] (forced token of sequence index i, < 0: none), ids int32 [B][max_length] and
 * unfinished int32 [B] (device, updated in place), force_eos_step (< 0: off) / force_eos_rows (HOST [B] or NULL) the two forced-EOS forms.
 * state: HOST int32 [52] in and out = DecState's {done, n_unfinished, step, seq, cur_len[16], pos[16], self_len[16]}; 1 <= cur_len[b] <
 * max_length.  next_x [B][d] (or NULL) = tok_emb[token] + pos_emb[pos[0] + 1], tok_emb [V][d] float or half (emb_half), pos_emb
 * [pos_rows][d].  No mailbox.  scratch: wt_dbg_greedy_select_scratch_bytes(max_length) bytes. */
size_t wt_dbg_greedy_select_scratch_bytes(int max_length);
int wt_dbg_greedy_select(const float* logits, const float* part_val, const int32_t* part_idx, int n_parts, const unsigned char* mask,
                         const int32_t* forced, int32_t* ids, int32_t* unfinished, int32_t* state, int force_eos_step,
                         const int32_t* force_eos_rows, const void* tok_emb, const float* pos_emb, int pos_rows, int emb_half, float* next_x, int B,
                         int V, int d, int max_length, int begin_index, int eos, int pad, void* scratch, void* stream);
/* The greedy tail of the log-probability mode (wt_decoder_set_logprobs) on caller-supplied operands, through the engine's own launch
 * builders.  form 0: the vocabulary GEMV with the log-sum-exp epilogue over X [B][K] (plain activations, no LayerNorm) and W [V][K] (float),
 * then greedy_finish_kernel<false, true>; form 1: greedy_select_kernel<true> over `logits` [B][V], then the same finish kernel; form 2:
 * timestamp mode, ts_select_kernel<true> + greedy_finish_kernel<true, true> over `logits` with the rules `t`.  mask bytes [V] (device; bit 0
 * suppressed, bit 1 suppressed at begin_index), forced a HOST array [max_length], ids int32 [B][max_length] (device; position cur_len is
 * written), cur_len: every row's length (1 <= cur_len < max_length), step: DecState.step (no_speech_prob is stored at step 0 only),
 * no_speech_token_id < 0: off.  Outputs (device): logprob_out f32 [B] = the step's token_logprob, sum_out f32 [B] (starts at 0),
 * no_speech_out f32 [B] or NULL.  scratch: wt_dbg_logprob_select_scratch_bytes(B, V, max_length) bytes.  Synchronises `stream`. */
size_t wt_dbg_logprob_select_scratch_bytes(int B, int V, int max_length);
int wt_dbg_logprob_select(int form, const float* X, const float* W, int K, const float* logits, const unsigned char* mask, const int32_t* forced,
                          int32_t* ids, int B, int V, int max_length, int cur_len, int step, int begin_index, int eos, int force_eos_step,
                          const wt_timestamp_params* t, int no_speech_token_id, float* logprob_out, float* sum_out, float* no_speech_out,
                          void* scratch, void* stream);
/* The same tail in its temperature-sampling form (wt_decoder_set_sampling): the arguments of wt_dbg_logprob_select plus the temperature
 * (> 0) and `seeds`, a HOST array of B 64-bit row seeds.  form 0: the vocabulary GEMV's sampling epilogue over X, W, then
 * greedy_finish_kernel<false, true, true>; form 1: sample_select_kernel over `logits`, in the partition of form 0's GEMV for this K (so K is needed here too), or, with `t` given, the timestamp mode's
 * ts_select_kernel<true, true> + greedy_finish_kernel<true, true, true>.  Position cur_len of `ids` receives the drawn token, logprob_out
 * its log-probability under the UNTEMPERED scores, key_out f32 [B] (device) the key it won with (in timestamp mode: the best key among
 * the ids the rules leave, also at the forced <|0.00|>).  scratch: wt_dbg_sample_select_scratch_bytes(B, V, max_length) bytes.
 * Synchronises `stream`. */
size_t wt_dbg_sample_select_scratch_bytes(int B, int V, int max_length);
int wt_dbg_sample_select(int form, const float* X, const float* W, int K, const float* logits, const unsigned char* mask, const int32_t* forced,
                         int32_t* ids, int B, int V, int max_length, int cur_len, int step, int begin_index, int eos, int force_eos_step,
                         const wt_timestamp_params* t, int no_speech_token_id, float temperature, const uint64_t* seeds, float* logprob_out,
                         float* sum_out, float* no_speech_out, float* key_out, void* scratch, void* stream);
/* step 0's input: x[b] = tok_emb[ids[b][cur_len[b] - 1]] + pos_emb[pos[b]]; ids [B][ids_ld], cur_len, pos: HOST arrays; tok_emb [V][d] float
 * or half (emb_half), pos_emb [pos_rows][d].  scratch: wt_dbg_dec_embed_scratch_bytes(B, ids_ld) bytes. */
size_t wt_dbg_dec_embed_scratch_bytes(int B, int ids_ld);
int wt_dbg_dec_embed(const int32_t* ids, int ids_ld, const int32_t* cur_len, const int32_t* pos, const void* tok_emb, int V, const float* pos_emb,
                     int pos_rows, int emb_half, float* x, int B, int d, void* scratch, void* stream);

/* ---- token-level timestamps (tests/test_gpu_token_timestamps.py): the post-pass launches, built by the engine's own parameter struct
 * (wt_common.h TokTsParams).
 * matrix: q_hist f32 [n_sel][N][64] and K [n_sel][S][64] (float, or IEEE half with kv_half) of ONE utterance -> W = softmax(q K^T) per head,
 * normalised over the N tokens, median of `width` along S, mean over the heads -> matrix_out f32 [N][S].  `w_out` (or NULL) receives the
 * softmax rows [n_sel][N][S] before the normalisation.
 * median: w_in f32 [n_sel][N][S] taken as already normalised -> median of `width` + mean over the heads -> matrix_out [N][S] (with
 * n_sel = 1 the median alone: a selection, so the output equals an input element bit for bit).
 * dtw: matrix f32 [B][N][S] -> ts_out f32 [B][N + 1] (entry 0 = 0), path_out int32 [B][2][N + S] (text indices, then time indices, in
 * backtrace order: last cell first), path_len int32 [B].
 * scratch: wt_dbg_token_timestamps_scratch_bytes(n_sel, B, N, S) bytes. */
size_t wt_dbg_token_timestamps_scratch_bytes(int n_sel, int B, int N, int S);
int wt_dbg_token_timestamp_matrix_kernels(const float* q_hist, const void* K, int kv_half, int n_sel, int N, int S, int width, float* w_out,
                                          float* matrix_out, void* scratch, void* stream);
int wt_dbg_token_timestamp_median(const float* w_in, int n_sel, int N, int S, int width, float* matrix_out, void* scratch, void* stream);
int wt_dbg_token_timestamp_dtw(const float* matrix, int B, int N, int S, double time_precision, float* ts_out, int32_t* path_out,
                               int32_t* path_len, void* scratch, void* stream);
/* a decode with token-level timestamps in flight: the captured queries, device f32 [n_sel][rows][max_length - 1][64] (steps not yet
 * executed are 0), and -- after wt_decoder_read_token_timestamps -- the matrix, device f32 [rows][max_length - 1][S] (token rows from
 * cur_len - 1 on are not written) */
int wt_dbg_token_timestamp_q_hist(wt_engine* dec, float* out, void* stream);
int wt_dbg_token_timestamp_matrix(wt_engine* dec, float* out, void* stream);
/* the halves of the post-pass alone (timing): which = 1 the matrix launches of every utterance, 2 the DTW launch over the matrix as it
 * stands; and the bytes of the mode's device allocation (query history, head table, W, statistics, matrix, trace, output) */
int wt_dbg_token_timestamp_postpass(wt_engine* dec, int which, void* stream);
size_t wt_dbg_token_timestamp_bytes(const wt_engine* dec);
/* how many step-graph captures the handle has made so far: a decode whose step configuration (csrc/host_logic.h: StepKey) repeats the
 * previous one's captures nothing */
int wt_dbg_step_graph_captures(const wt_engine* dec);
/* the resident cross-K rows of one (layer, head) of the decode in flight, widened to float: HOST f32 [rows][S][64].  Synchronises. */
int wt_dbg_cross_k_head(wt_engine* dec, int layer, int head, float* out_host, void* stream);
/* the stages of the log-mel front-end that wt_logmel_forward does not return, as its last call on `h` with this `batch` left them:
 * pw_out f32 [batch][n_frames][npw], the fp64-DFT power spectrum (columns >= n_bins are 0), and logmel_out f32
 * [batch][n_frames][n_mels], log10(max(1e-10, mel)) before the max - 8 clamp and the (x + 4) / 4 scaling.  Either may be NULL.  Two
 * device-to-device copies on `stream` (the stream of that forward), no kernel.  WT_E_INVALID when batch exceeds the handle's workspace. */
int wt_dbg_logmel_stages(wt_logmel* h, int batch, float* pw_out, float* logmel_out, void* stream);
/* prefill_attn_kernel alone (kernels_prefill.hip): ctx [B][nq][ldc] = softmax(q_scale . q k^T) v per head, q device f32 [B][nq][ldq] with
 * head h at column 64 h, kcache / vcache device f32 [B][H][cap][64] of which keys [0, nk) are read.  causal 1: query t sees keys 0..t and
 * nk must equal nq; 0: every query sees all nk keys.  ldq / ldc multiples of 4, >= 64 H. */
int wt_dbg_prefill_attention(const float* q, const float* kcache, const float* vcache, float* ctx, int B, int H, int nq, int nk, int cap, int ldq,
                             int ldc, int causal, float q_scale, void* stream);
/* the prefill's query finish alone: q [rows][d] = (u - mean(h1) . r) * rstd(h1) + t per row (what dec_attn_kernel does to its folded
 * query); u / h1 / q device f32 [rows][d], r / t device f32 [d], d <= 1280 */
int wt_dbg_prefill_query_finish(const float* u, const float* h1, const float* r, const float* t, float* q, int rows, int d, void* stream);
/* the resident self-K (which = 0) or self-V (1) rows of one (layer, head) of the decode in flight: HOST f32 [rows][max_target_positions][64],
 * rows the decode has not written hold whatever the cache held.  fp32 decoder engines only.  Synchronises. */
int wt_dbg_self_kv_head(wt_engine* dec, int layer, int head, int which, float* out_host, void* stream);
/* lang_select_kernel alone, launched as the first step of a language-detecting decode launches it (wt_decoder_set_languages): per row b of
 * x (device f32 [B][d], the residual stream in front of the final LayerNorm; ln_w / ln_b device f32 [d], both NULL: x is used as it is)
 * z[l] = dot(LayerNorm(x_b), emb[lang_ids[l]]) over emb device [V][d] (f32, or IEEE half with emb_half), lang_prob device f32
 * [B][n_lang] = softmax(z), and lang_tok device i32 [B]: an entry < 0 becomes the id of the largest z (torch.argmax over the masked
 * vocabulary: NaN first, equals to the lowest id), an entry >= 0 stays.  lang_ids HOST i32 [n_lang], 1 <= n_lang <= 128, each inside
 * [0, V); d a multiple of 4, <= 1280; B <= 16.  scratch: device, wt_dbg_lang_select_scratch_bytes(). */
size_t wt_dbg_lang_select_scratch_bytes(void);
int wt_dbg_lang_select(const float* x, const float* ln_w, const float* ln_b, const void* emb, int emb_half, const int32_t* lang_ids, int n_lang,
                       int V, int B, int d, int32_t* lang_tok, float* lang_prob, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
