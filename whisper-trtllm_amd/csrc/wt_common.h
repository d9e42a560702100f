// Shared declarations of the MI355X Whisper engine (internal; the public ABI is include/whisper_trtllm_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "host_logic.h"  // HEAD_DIM and the decode limits (MAX_ROWS, STREAM_QCAP, MAX_BEAMS, TT_MAX_*), BlobHeader / BlobTensor, EngineDims,
                         // the decode configuration (host-only part, also built under ASan/UBSan)

namespace wt {

// ---- device-resident decode state: every per-step quantity kernels need lives here so that one captured
// hipGraph replays for every step (nothing step-dependent is baked into kernel arguments) ------------------
// The per-ROW quantities are arrays over the decode slots: a batch started by wt_decoder_begin keeps its rows aligned (all entries
// equal), the continuous mode (wt_decoder_stream_*) refills a slot with the next waiting utterance the moment its row stops, so every
// slot runs at its own position -- what the reference's one-clip-at-a-time loop gives for free (run.py:219-226, cal_wer.py:249-287).
struct DecState {
    int done;          // stop test fired (all rows EOS, or cur_len >= max_length); continuous mode: no slot active and nothing waiting
    int n_unfinished;  // rows that have not produced EOS yet (continuous mode: active slots)
    int step;          // 0-based count of executed steps
    int seq;           // greedy_finish launches since wt_decoder_begin, no-op ones included (the host mailbox's progress counter)
    int epoch;         // which wt_decoder_begin this state belongs to (low 16 bits travel in the mailbox word)
    int q_head;        // continuous mode: utterances admitted to a slot so far (device-owned) ...
    int q_tail;        // ... of those published by the host (stream_publish_kernel)
    int pad0;
    int cur_len[MAX_ROWS];    // tokens in row b of `ids` so far (prompt included)
    int pos[MAX_ROWS];        // decoder position of the token being fed to row b
    int self_len[MAX_ROWS];   // valid keys already in row b's self cache; the new key/value row is written at this index
    int slot_row[MAX_ROWS];   // continuous mode: cross-cache pool row of the utterance in slot b, -1 = idle slot
    int row_force[MAX_ROWS];  // continuous mode, bench only: row-local 0-based step at which slot b's utterance emits EOS, -1 = never
    int queue[STREAM_QCAP];       // continuous mode: pool rows waiting for a slot, entry i at queue[i % STREAM_QCAP]
    int rec_force[STREAM_QCAP];   // continuous mode: row_force of the utterance in pool row r
};

// Host mailbox word (64 bits, written by greedy_finish_kernel with ONE system-scope store into pinned host memory after every
// step, read by wt_decoder_run without touching the stream): [63:48] epoch, [47:32] seq, [31] done, [30:16] cur_len,
// [15:0] bit b = row b unfinished.
__host__ __device__ inline unsigned long long mailbox_word(int epoch, int seq, int done, int cur_len, unsigned unfinished_mask) {
    return ((unsigned long long)(epoch & 0xffff) << 48) | ((unsigned long long)(seq & 0xffff) << 32) |
           ((unsigned long long)(done ? 1u : 0u) << 31) | ((unsigned long long)(cur_len & 0x7fff) << 16) | (unfinished_mask & 0xffffu);
}

// ---- fp32 GEMM (encoder / cross-KV):  C[m][n] = epi( sum_k A[m][k] * W[n][k] + bias[n] ) ------------------
struct GemmParams {
    const float* A;       // row m at A + (m / a_rows_per_batch) * a_batch_stride + (m % a_rows_per_batch) * lda
    const float* W;       // [N][K] row-major (nn.Linear layout, x @ W^T)
    const float* bias;    // [N] or nullptr
    const float* resid;   // same addressing as C, or nullptr (may alias C)
    const float* pos;     // [c_rows_per_batch][N] added after the activation (encoder embed_positions) or nullptr
    float* C;             // row m at C + (m / c_rows_per_batch) * c_batch_stride + (m % c_rows_per_batch) * ldc
    float* C2;            // EPI_KV_HEADS: value cache base (C is the key cache base)
    long long a_batch_stride, c_batch_stride;
    int M, N, K, lda, ldc;
    int a_rows_per_batch, c_rows_per_batch;
    int act;              // 0 none, 1 exact-erf GELU
    int epi;              // 0 row-major, 1 split into K/V head caches [b][h][s_cap][64]
    int kv_heads, kv_cap, kv_seq_off;  // EPI_KV_HEADS: heads per row, cache capacity (rows), first row to write
    int epi_fits32;                    // set by launch_gemm_f32: every output / residual / position offset fits an int (fast epilogue)
    // launch_gemm_x3 (fp32 product on the bf16 matrix cores, exactly split operands): A and W point at plane 0 of THREE bf16 planes with
    // the fp32 operand's row layout (lda / a_batch_stride / K in ELEMENTS as usual), plane p at + p * a_plane / w_plane elements
    long long a_plane, w_plane;
    int out_split;                     // the epilogue writes C as three bf16 planes (row layout as C, plane p at + p * c_plane elements)
    long long c_plane;
    long long* dbg_stamps;             // probe builds only (wt_dbg_gemm_stamps): [tiles][8] placement + wall-clock stamps per workgroup
};
enum { EPI_ROWMAJOR = 0, EPI_KV_HEADS = 1 };

constexpr int PART_STRIDE = 68;  // attention split partial: o[64], m, l, 2 pad floats

// ---- decode-step skinny GEMM:  y[b][n] = epi( sum_k X(b)[k] * W[n][k] + bias[n] ),  b < NB <= 8 -----------
enum { XMODE_PLAIN = 0, XMODE_LAYERNORM = 1 };
enum { YMODE_PLAIN = 0, YMODE_QKV_APPEND = 1, YMODE_ARGMAX = 2 };
struct SkinnyParams {
    const float* X;        // [B][K]  (with X2: [B][K/2], columns [0, K/2))
    const float* parts;    // optional: X is the MERGE of attention split partials [B][parts_H][parts_nsplit][PART_STRIDE] (o[64], m, l)
                           //           written by dec_attn_kernel with defer_merge (K = parts_H * 64, LDS-staged path only)
    const float* X2;       // optional second activation [B][K/2] for columns [K/2, K): y = W . [X ; X2]  (x_direct path)
    const float* ln_w;     // LAYERNORM gamma/beta [K]
    const float* ln_b;
    const float* W;        // [N][K]
    const float* bias;     // [N] or nullptr
    const float* resid;    // [B][N] or nullptr (may alias Y)
    float* Y;              // PLAIN: [B][N]
    float* kcache;         // QKV_APPEND: self key/value cache of this layer [B][H][s_cap][64]; q goes to Y [B][d]
    float* vcache;
    const DecState* st;
    int B, N, K;
    int xmode;             // XMODE_*
    int w_nt;              // stream W with non-temporal loads
    int x_direct;          // PLAIN only: every wave loads its activations straight from L2 (no LDS staging)
    int act;               // 0 none, 1 GELU
    int ymode;
    int d_model, s_cap;    // QKV_APPEND
    float q_scale;         // QKV_APPEND: multiply the q third by this (head_dim^-0.5)
    int parts_nsplit, parts_H;
    int w_half;            // W (and only W) is IEEE half [N][K]: fp16 decoder engines; K-slices must be multiples of 8
    int kv_half;           // QKV_APPEND: the self caches are IEEE half (resident caches of an fp16 engine's fast path)
    // YMODE_ARGMAX (vocabulary projection of the greedy fast path): the logits never reach HBM unless a trace is requested.
    // Every workgroup reduces its rows to one masked (max, argmax) per batch row: am_val / am_idx [B][am_ld], column = workgroup.
    const uint8_t* am_mask;  // [N] bit0: always suppressed, bit1: suppressed when cur_len == am_begin_index
    float* am_val;
    int* am_idx;
    float* am_trace;       // optional raw-logits trace [B][am_trace_steps][N] (row st->step), or nullptr
    int am_ld, am_begin_index, am_trace_steps;
    // log-probability mode (am_lp != 0; wt_decoder_set_logprobs): the LP instantiations of the ARGMAX epilogue also reduce, per batch row and
    // workgroup, the online log-sum-exp pair (max, sum of exp(x - max)) of the masked scores -- and, with am_lp == 2, a second pair over the
    // raw logits (no_speech_prob) -- into am_lse [B][am_ld] as (m, s, raw m, raw s); the masked score of id am_eos and the raw logit of id
    // am_ns (< 0: none) go to am_side [B][2].  am_lp == 0: the plain instantiations run, exactly as before.
    float4* am_lse;
    float* am_side;
    int am_lp, am_eos, am_ns;
    // temperature sampling (am_samp != 0; wt_decoder_set_sampling; needs am_lp != 0): the SAMP instantiations compare the Gumbel-max key
    // s / am_temp + g(am_seeds[b], st->cur_len[b], n) (sample_key below) instead of the score s; am_val then holds the winning KEY and am_sc
    // [B][am_ld] the winner's score s.  am_samp == 0: the instantiations without it run, exactly as before.
    int am_samp;
    float am_temp;
    const unsigned long long* am_seeds;   // [B]
    float* am_sc;
};

// ---- decode attention (query length 1), split over the key axis ---------------------------------------------
struct DecAttnParams {
    const float* q;        // [B][d] (already scaled)
    const float* kcache;   // [B][H][s_cap][64]
    const float* vcache;
    float* part;           // scratch [B][H][n_split][PART_STRIDE] (n_split > 1)
    int* cnt;              // arrival tickets [B][H], zero between launches (n_split > 1)
    float* out;            // [B][d] normalised attention output
    const DecState* st;
    int B, H, s_cap;
    int n_split;
    int fixed_len;         // >0: number of keys (cross attention); 0: use st->self_len + 1
    int nt;                // stream K/V with non-temporal loads (0: default cache policy)
    int defer_merge;       // n_split > 1: leave the split partials in `part` (plain stores, no ticket); the consumer GEMV merges them
    // folded cross-attention query: q holds u = s.Wq.diag(gamma).h1 (+ const) and the kernel finishes the
    // LayerNorm per row: q = (u - mean(h1) . ln_r) * rstd(h1) + ln_t.  ln_h == nullptr: q is used as it is.
    const float* ln_h;     // [B][d] residual stream whose LayerNorm statistics normalise q
    const float* ln_r;     // [d] row sums of s.Wq.diag(gamma)
    const float* ln_t;     // [d] s.(Wq.beta + bq)
    int kv_half;           // kcache / vcache are IEEE half (fp16 decoder engines keep their RESIDENT caches in fp16; fp32 arithmetic)
    const int* alive;      // optional [B]: rows with alive[b] == 0 (finished: they emit pad whatever their logits) stream no K/V; their
                           // context / partials keep the previous step's (finite) values.  nullptr: every row attends.
    const int* slot_row;   // optional [B] (continuous mode, cross attention): slot b reads cache row max(slot_row[b], 0) instead of row b
    // beam search, self attention: key s of row b lives in physical cache row anc[(parity * MAX_ROWS + b) * anc_ld + s], parity =
    // st->step & 1 (0 without st): the ancestry table beam_finish_kernel maintains instead of regathering the caches.  Unsplit only.
    const int* anc;
    int anc_ld;
    // beam search, cross attention, grouped form (2 or 4; 0 / 1: off): cache row u is shared by the query rows u * group .. + group - 1,
    // one block streams it once for all of them (grid z = B / group).  Not with slot_row / alive / anc.
    int group;
    // token-level timestamps (wt_decoder_set_token_timestamps), cross attention only: the blocks of split 0 whose head h has qh_sel[h] >= 0
    // store the finished query (after the folded-LayerNorm finish) into qh[qh_sel[h]][b][st->step][64], before a finished row leaves.
    // qh == nullptr: the instantiations without the capture run, exactly as before.
    float* qh;             // [n_sel][qh_rows][qh_steps][64]
    const int* qh_sel;     // this layer's [H]: selection index of head h, or -1
    int qh_rows, qh_steps;
};

// ---- prefill attention (query length nq; kernels_prefill.hip): the prompt positions of a decode through one decoder layer together ----
struct PrefillAttnParams {
    const float* q;        // [B][nq][ldq], head h at column 64 h (not scaled: q_scale below)
    const float* k;        // head cache [rows >= B][H][cap][64], utterance b in cache row b; only keys [0, nk) are read
    const float* v;
    float* ctx;            // [B][nq][ldc], head h at column 64 h
    int B, H, nq, nk, cap;
    int ldq, ldc;          // multiples of 4, >= 64 H
    int causal;            // 1: query t sees keys 0..t (nk == nq); 0: every query sees keys 0..nk-1
    float q_scale;
};
hipError_t launch_prefill_attention(const PrefillAttnParams& p, hipStream_t s);
// q[m] = (u[m] - mean(h1[m]) . r) * rstd(h1[m]) + t over `rows` rows of d <= 1280: the folded cross-attention query finished as
// dec_attn_kernel finishes it (DecAttnParams.ln_h / ln_r / ln_t); q may alias u
hipError_t launch_prefill_query_finish(const float* u, const float* h1, const float* r, const float* t, float* q, int rows, int d, hipStream_t s);
// x[b * len + t] = embed_tokens[prompt(b)[t]] + embed_positions[t]; prompt [n_rows][len] on the device, n_rows == 1: shared by all rows
hipError_t launch_prefill_embed(const int* prompt, int n_rows, int len, const float* tok_emb, const float* pos_emb, float* x, int B, int d,
                                hipStream_t s);
// behind launch_dec_init: ids row b = prompt(b), start token; cur_len = len + 1, pos = len, self_len = len for every row
hipError_t launch_prefill_state(DecState* st, int* ids, const int* prompt, int n_rows, int len, int B, int max_length, int start_token,
                                hipStream_t s);
// the ragged form: prompt [B][len] right-padded, lens[B] device; ids row b = pad x (len - lens[b]), prompt(b), start token; cur_len = len + 1 for
// every row, pos = self_len = lens[b]
hipError_t launch_prefill_state_rows(DecState* st, int* ids, const int* prompt, const int* lens, int len, int B, int max_length, int start_token,
                                     int pad, hipStream_t s);

// ---- token-level timestamps: the post-pass over the captured queries and the resident cross-K cache (kernels_token_timestamps.hip) ----
// Per utterance b and selected head: W[t][s] = softmax_s(q_hist[t] . K[s]); W = (W - mean_t) / std_t (population std over the N tokens);
// a median of odd `width` along s with reflect padding (the input unchanged when S <= width / 2); the mean over the heads = matrix[N][S];
// DTW on -matrix with an fp32 cost, cell = (float)((double)(-m) + (double)c), predecessor 0 (diagonal) if c0 < c1 && c0 < c2, else 1 (up)
// if c1 < c0 && c1 < c2, else 2 (left); backtrace from (N, S) with the borders trace[0][:] = 2, trace[:][0] = 1;
// out[b][0] = 0, out[b][1 + k] = (float)(time_precision * frame at which the path first reaches token k).
struct TokTsParams {
    const float* q_hist;   // [n_sel][qh_rows][qh_steps][64]
    int qh_rows, qh_steps;
    const void* cross_k;   // resident cross-K caches [L][cross_rows][H][S][64], float or IEEE half (kv_half)
    int kv_half, cross_rows, H, S;
    int n_sel;
    int layer[TT_MAX_HEADS], head[TT_MAX_HEADS];
    int width;             // odd, 1 .. TT_MAX_WIDTH
    double time_precision;
    const DecState* st;    // N = st->cur_len[0] - 1 (the batch-wide length, as the reference), or, st == nullptr, n_fixed
    int n_fixed, n_cap;    // n_cap: row capacity of W / matrix / trace and the grid's bound on N
    int B;
    float* W;              // scratch [n_sel][n_cap][S]: one utterance's softmax rows
    float* mean;           // scratch [n_sel][S]
    float* sdev;           // scratch [n_sel][S]
    float* matrix;         // [B][n_cap][S]
    uint8_t* trace;        // [B][n_cap][trace_ld]: predecessor codes of rows 1..N, columns 0..S (column 0 unused)
    int trace_ld;          // multiple of 4, >= S + 1
    int* path;             // optional [B][2][n_cap + S]: the path in backtrace order (text indices, then time indices)
    int* path_len;         // optional [B]
    float* out;            // [B][out_ld]
    int out_ld;
};
inline int tt_trace_ld(int S) { return (S + 1 + 3) & ~3; }
// one utterance's matrix (three launches: softmax rows, column statistics, median + head mean)
hipError_t launch_tt_matrix(const TokTsParams& p, int b, hipStream_t s);
// the median + head mean alone over p.W as it stands (p.mean == nullptr: W is taken as already normalised)
hipError_t launch_tt_median(const TokTsParams& p, int b, hipStream_t s);
// DTW + backtrace + timestamps of all B utterances (one workgroup each)
hipError_t launch_tt_dtw(const TokTsParams& p, hipStream_t s);

// A/B tuning switches (WT_NSPLIT_CROSS, WT_GEMM_NO_DMA, ...; DESIGN.md "Tuning knobs") are lab tools, not part of the C-ABI's
// contract: they are read ONLY when the process also sets WT_TUNING=1, so a stray variable in a production environment cannot
// change what the library behind the ABI does.
inline const char* tuning_env(const char* name) {
    static const bool on = [] { const char* t = getenv("WT_TUNING"); return t && t[0] == '1'; }();
    return on ? getenv(name) : nullptr;
}

// torch.argmax semantics (the reference's greedy step, run.py:205): NaN counts as the maximum, the lowest index wins ties.
// True when candidate (v, i) beats the running (best, bidx).
__device__ __forceinline__ bool argmax_better(float v, int i, float best, int bidx) {
    const bool vn = v != v, bn = best != best;
    return vn ? (!bn || i < bidx) : (!bn && (v > best || (v == best && i < bidx)));
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE property: a launcher keeps one "done" flag per device
// (`static PerDeviceFlag f; if (!f.get()) { ...set...; f.set(); }`), so a second device opened in the same process gets
// its dynamic-LDS limit raised too.
// Distinct handles may be driven from different host threads at once (runtime.WhisperPipeline does): the flag is atomic, and two
// threads that both find it clear simply both set the (idempotent) attribute.
struct PerDeviceFlag {
    std::atomic<bool> done[64] = {};
    static int cur() { int dev = 0; (void)hipGetDevice(&dev); return dev & 63; }
    bool get() const { return done[cur()].load(std::memory_order_acquire); }
    void set() { done[cur()].store(true, std::memory_order_release); }
};

// Every ABI entry point runs on its handle's device and leaves the CALLER's current device (torch's) as it found it.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// launchers (kernels_*.hip)
hipError_t launch_mel_transpose(const float* mel, float* melT, int B, int n_mels, int frames, hipStream_t s);
hipError_t launch_mel_transpose_split(const float* mel, void* planes, size_t plane_stride, int B, int n_mels, int frames, hipStream_t s);   // three bf16 planes
hipError_t launch_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int d, hipStream_t s);
hipError_t launch_gemm_f32(const GemmParams& p, hipStream_t s);
// ---- fp32 GEMM on the bf16 matrix cores.  x = b1 + b2 + b3 with bf16 b1 = rn(x), b2 = rn(x - b1), b3 = rn(x - b1 - b2) represents an fp32
// value to 2^-24 relative or better (three 8-bit significands cover fp32's 24 bits; bf16 has fp32's exponent range), with |b2| <= 2^-8 |x|
// and |b3| <= 2^-16 |x|.  A product a.w is the sum of the six partial products a_i.w_j with i + j <= 4; the three dropped ones (a2.w3,
// a3.w2, a3.w3) are each up to 2^-24 |a||w| in the worst case, about 2^-23 |a||w| per product together -- the size of the rounding of
// an fp32 FMA, and measured no worse than the fp32 MFMA on random operands (tests/test_gpu_kernels.py::test_gemm_x3_is_an_fp32_gemm).
// On a coherently growing sum (products of one sign) the accumulation error grows faster with K than the fp32 MFMA's: 3.7e-6 against
// 4.2e-7 of sum |a||w| at K = 4096 (same test; the mechanism is not established).
// Every partial product of two bf16 values is exact in the MFMA's fp32 accumulator, which accumulates as the fp32 MFMA does.  Six
// v_mfma_f32_32x32x16_bf16 replace sixteen v_mfma_f32_32x32x2_f32 per 32x32x16 block: 16 / 6 = 2.7x the fp32 MFMA peak.
// force_tile: 128 / 192 / 256 selects that tile instantiation (tests); 0 = by shape (or WT_GEMM_X3_TILE under WT_TUNING=1).
hipError_t launch_gemm_x3(const GemmParams& p, hipStream_t s, int force_tile = 0);
bool gemm_x3_usable(const GemmParams& p);   // shape / alignment limits of launch_gemm_x3 (else: launch_gemm_f32 on the fp32 operands)
hipError_t launch_split3(const float* x, void* planes, size_t n, size_t plane_stride, hipStream_t s);   // fp32 [n] -> three bf16 planes
hipError_t launch_layernorm_split(const float* x, const float* w, const float* b, void* planes, size_t plane_stride, int rows, int d, hipStream_t s);
hipError_t launch_encoder_attention(const float* qkv, float* ctx, int B, int S, int H, hipStream_t s, void* ctx_planes = nullptr, size_t plane_stride = 0);
    // ctx_planes != nullptr: the context goes out as three bf16 planes (the A operand of launch_gemm_x3) instead of fp32 `ctx`
int encoder_attention_blocks_per_cu();
// x3 form (both products from bf16 MFMAs of exactly split operands, fp32 scores / softmax / accumulators): q|k|v in, context out as planes
hipError_t launch_encoder_attention_x3(const void* qkv_planes, size_t in_plane, void* ctx_planes, size_t out_plane, int B, int S, int H, hipStream_t s);
// fp16-encoder path (kernels_encoder_f16.hip): `void*` operands are __half buffers
hipError_t launch_mel_transpose_h(const float* mel, void* melT, int B, int n_mels, int frames, hipStream_t s);
hipError_t launch_layernorm_h(const float* x, const float* w, const float* b, void* y, int rows, int d, hipStream_t s);
hipError_t launch_cast_h(const float* x, void* y, size_t n, hipStream_t s);
hipError_t launch_gemm_f16(const GemmParams& p, bool out_half, hipStream_t s, int force_variant = 0);  // 0: by shape; 2 / 3: see kernels_encoder_f16.hip
hipError_t launch_encoder_attention_f16(const void* qkv, void* ctx, int B, int S, int H, hipStream_t s);  // half in, half out  // p.A / p.W point at __half data

hipError_t launch_dec_embed(const int* ids, int ids_ld, const float* tok_emb, const float* pos_emb, float* x, int B,
                            int d, const DecState* st, hipStream_t s, int emb_half = 0);   // emb_half: tok_emb is IEEE half
hipError_t launch_skinny(const SkinnyParams& p, hipStream_t s);
hipError_t launch_skinny_gelu_in_probe(const SkinnyParams& p, hipStream_t s);   // probe only (tools/microbench.py fold_fc1)
int skinny_grid(const SkinnyParams& p);  // workgroups launch_skinny uses for p (column count of am_val / am_idx), -1 if p is invalid
// two independent skinny GEMMs (same batch) in ONE launch: blocks [0, grid_a) run `a`, the rest run `b`
hipError_t launch_skinny_pair(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s);
// the q|k|v launch (`a`: LayerNorm -> q|k|v -> append, exactly as launch_skinny runs it) carrying a plain LDS-staged GEMV `b` (K <= 1024)
// on the workgroups it leaves idle: the residual half of the folded cross-attention query (qfold_resid_skinny_params)
hipError_t launch_skinny_qkv_hoist(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s);
hipError_t launch_dec_attn(const DecAttnParams& p, hipStream_t s);

constexpr int SELECT_CHUNKS = 8;   // vocabulary chunks (workgroups per row) of greedy_select_kernel / ts_select_kernel
// Timestamp mode: one chunk's partial result per row (ts_select_kernel -> greedy_finish_kernel<true>).  Over the masked scores of the
// chunk: the text maximum and its index over [0, tb), the timestamp maximum and its index over [tb, V) (both NaN-aware, lowest index on
// ties), and the timestamp log-sum-exp as (zmax, zsum) = (largest finite timestamp score, sum of exp(x - zmax)); a NaN timestamp score
// makes zsum NaN.
struct TsPart {
    float tmax;
    int targ;
    float smax;
    int sarg;
    float zmax, zsum;
    float xmax, xsum;      // log-probability mode only (else unused): the same pair over the chunk's text scores
};

// Beam search (wt_decoder_set_beam_search): rows are [utterance][beam], row = u * nb + j.
constexpr int BEAM_KMAX = 2 * MAX_BEAMS;   // candidates kept per utterance and step: 2 * num_beams
// One vocabulary chunk of one row (beam_select_kernel -> beam_finish_kernel): the online log-sum-exp pair over ALL ids of the chunk
// (m = largest non-NaN logit, s = sum of exp(x - m); NaN logits are left out of it) and the chunk's 2 * nb best ids under the
// suppress masks (masked: -inf), NaN-aware, lowest index on ties; idx < 0: the chunk holds fewer ids than that.
struct BeamPart {
    float m, s;
    float val[BEAM_KMAX];
    int idx[BEAM_KMAX];
    int pad[2];
};
// Device state of a beam decode.  The id history and the ancestry table are double-buffered on the parity of DecState.step: a step
// reads buffer step & 1 and beam_finish_kernel writes the re-parented rows into the other one.
struct BeamParams {
    int nb, U;                 // beams per utterance, utterances (rows B = U * nb)
    float length_penalty;
    int early_stopping;
    BeamPart* part;            // [B][SELECT_CHUNKS]
    float* scores;             // [B] running beam scores (sum of log-probabilities)
    int* ids2;                 // [B][max_length]: id buffer of odd steps (SelectParams.ids: even steps)
    int* anc;                  // [2][MAX_ROWS][anc_ld]: physical self-cache row of key s of row b
    int anc_ld;
    int* urow;                 // [MAX_ROWS]: row -> utterance (the cross-attention's slot_row table)
    // BeamHypotheses per utterance: nb entries of (score, length, ids), the worst kept score, the done flag
    int* hyp_n;                // [U]
    int* hyp_done;             // [U]
    double* hyp_worst;         // [U]
    double* hyp_score;         // [U][nb]
    int* hyp_len;              // [U][nb]
    int* hyp_ids;              // [U][nb][hyp_ld]
    int hyp_ld;
    int* out_ids;              // [U][max_length]: finalize's best hypothesis (EOS behind it when it fits, then pad)
    float* out_scores;         // [U]
    int* trace;                // optional [max_length][B][4]: per step and row (token, source beam within the utterance, score bits, done)
    int* dbg_cand;             // optional (debug hook) [U][BEAM_KMAX][3]: the sorted candidates (token, source beam, score bits), token -1 = none
};

struct SelectParams {
    const float* logits;   // [B][V]
    const uint8_t* mask;   // [V] bit0: always suppressed, bit1: suppressed when cur_len == begin_index
    const int* forced;     // [max_length] forced token for generation index i, or -1
    int* ids;              // [B][max_length]
    int* unfinished;       // [B]
    DecState* st;
    float* trace;          // optional [B][max_length-1][V]
    float* part_val;       // scratch [B][n_parts] partial maxima (n_parts = 8 chunks of greedy_select_kernel, or the workgroups
    int* part_idx;         //   of the vocabulary GEMV when the argmax is fused into its epilogue: fused != 0)
    int n_parts, fused;
    const float* tok_emb;  // next-step embedding: embed_tokens [V][d], embed_positions [T][d]
    const float* pos_emb;
    float* next_x;         // [B][d] decoder input of the next step, or nullptr
    int d_model;
    int B, V, max_length, begin_index, eos, pad, force_eos_step;
    int emb_half;          // tok_emb is IEEE half (fp16 decoder engines)
    const int* force_eos_rows;       // optional [B]: row b emits EOS at 0-based step force_eos_rows[b] (< 0: never) -- bench-only transcript lengths
    unsigned long long* mailbox;     // optional: device address of the engine's pinned host mailbox (mailbox_word above)
    // continuous mode (stream != 0): finished utterances report to the host through pinned memory, indexed by cross-cache pool row
    int stream, start_token;
    int* host_ids;                   // device address of the pinned id rows [pool][max_length]
    int* host_len;                   // device address of the pinned final lengths [pool] (0 = still decoding)
    // timestamp mode (ts_on != 0; wt_decoder_set_timestamp_rules): the logits reach HBM (fused == 0), ts_select_kernel + the timestamp
    // instantiation of greedy_finish_kernel replace the plain argmax.  no_ts = <|notimestamps|>, tb = first timestamp id,
    // ts_begin_index = sequence length of the first generated timestamp + 1, max_init < 0: no max-initial-timestamp rule
    int ts_on, no_ts, tb, ts_begin_index, max_init;
    TsPart* ts_part;                 // scratch [B][SELECT_CHUNKS]
    int* ts_tok;                     // optional [B]: the rule-chosen token before the forced / pad / EOS bookkeeping (debug hook)
    float* ts_stats;                 // optional [B][2]: (log-sum-exp of the timestamp scores, text maximum) after the masks (debug hook)
    // beam search (beam_on != 0; wt_decoder_set_beam_search): plain logits in HBM, then beam_select_kernel + beam_finish_kernel
    int beam_on;
    BeamParams beam;
    // log-probability mode (lp_on != 0; wt_decoder_set_logprobs): the LP instantiations of the select / finish kernels run.  lp_part
    // [B][n_parts] holds one (m, s, raw m, raw s) per partial (the vocabulary GEMV's workgroups, or the select kernels' chunks), lp_side
    // [B][2] the masked score of the EOS id and the raw logit of id lp_ns.  The finish kernel writes token_logprob[b][cur_len] into lp_tok
    // [B][max_length], adds it to lp_sum [B] while row b is unfinished, and at step 0 stores softmax(raw logits)[lp_ns] into lp_nsp [B]
    // (lp_ns < 0: off).
    int lp_on, lp_ns;
    float4* lp_part;
    float* lp_side;
    float* lp_tok;
    float* lp_sum;
    float* lp_nsp;
    // temperature sampling (samp_on != 0; wt_decoder_set_sampling; with lp_on): the SAMP instantiations of the select / finish kernels run.
    // A partial's part_val is the best Gumbel-max KEY of its ids (sample_key below) and samp_sc [B][n_parts] the score s of that id.  Timestamp
    // mode: TsPart.tmax / smax are the best text / timestamp KEYS of the chunk, and samp_ts [B][SELECT_CHUNKS] holds (score of targ, score
    // of sarg, the chunk's best unperturbed text score -- rule 5's tmax --, unused).  samp_key [B] (optional): the key the token won with.
    // Without the fused epilogue (fused == 0, no timestamp mode) sample_select_kernel walks the logits in the partition of the sampling GEMV
    // for (B, V, samp_K) -- samp_K = that GEMV's K -- and writes one partial per GEMV workgroup: the part / lp_part / samp_sc rows must hold
    // samp_parts_cap >= that plan's workgroups, which replace n_parts for the launch.
    int samp_on, samp_K, samp_parts_cap;
    float samp_temp;
    const unsigned long long* samp_seeds;   // [B]
    float* samp_sc;
    float4* samp_ts;
    float* samp_key;
    // per-row language tokens (lang_pos > 0; wt_decoder_set_languages): at cur_len == lang_pos the forced token of row b is lang_tok[b]
    // instead of forced[cur_len] (written by the host, or by lang_select_kernel earlier in that step)
    int lang_pos;
    const int* lang_tok;             // [B]
};
// Language detection, a rule of the first step (DESIGN.md "Language detection"): per row the logits of the listed language ids alone, from
// the residual stream entering the final LayerNorm, their softmax and the winning id.
struct LangSelectParams {
    const float* x;                  // [B][d] the step's final hidden state, in front of the final LayerNorm
    const float *ln_w, *ln_b;        // the final LayerNorm (nullptr: x is used as it is)
    const float* emb;                // the tied embedding / projection matrix [V][d]: fp32, or IEEE half with emb_half
    int emb_half;
    const int* lang_ids;             // [n_lang] token ids inside the vocabulary, 1 <= n_lang <= LANG_MAX, any order
    int n_lang, B, d;                // d a multiple of 4, <= LANG_D_MAX
    int* lang_tok;                   // [B] in: >= 0 keeps the caller's choice; out: the winning id where it was negative
    float* lang_prob;                // [B][n_lang]
};
constexpr int LANG_D_MAX = 1280;
hipError_t launch_lang_select(const LangSelectParams& p, hipStream_t s);
// ---- temperature sampling: Gumbel-max over a counter-based generator (DESIGN.md "Temperature sampling").  Philox-4x32-10 (Salmon et al.,
// SC'11): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped by the Weyl constants between rounds.
__host__ __device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// standard Gumbel noise of one 32-bit draw: u = ((x >> 9) + 0.5) 2^-23 is exact in fp32 and strictly inside (0, 1)
__device__ __forceinline__ float gumbel_of(const unsigned x) {
    const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}
// the four draws that serve vocabulary ids 4 * v4 .. 4 * v4 + 3 of a row with `seed` writing sequence position t
__device__ __forceinline__ void sample_draws(const unsigned long long seed, const int t, const int v4, unsigned out[4]) {
    philox4x32_10((unsigned)v4, (unsigned)t, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), out);
}
// key of a score under temperature T: s / T + g (IEEE division: what the reference's TemperatureLogitsWarper computes); -inf stays -inf, NaN NaN
__device__ __forceinline__ float sample_key(const float s, const float T, const unsigned x) { return s / T + gumbel_of(x); }
// online log-sum-exp pairs (m = largest score that is neither NaN nor -inf, s = sum of exp(x - m)): the empty pair is (-inf, 0), a NaN score
// makes s NaN
__device__ __forceinline__ float lse_rescale(float s, float m, float nm) { return s == 0.f ? 0.f : s * expf(m - nm); }
__device__ __forceinline__ void lse_add(float& m, float& s, const float x) {
    if (x > m) {
        s = lse_rescale(s, m, x) + 1.f;
        m = x;
    } else if (x != -INFINITY) {
        s += expf(x - m);
    }
}
__device__ __forceinline__ void lse_merge(float& m, float& s, const float om, const float os) {   // (m, s) += (om, os), in this order
    const float nm = fmaxf(m, om);
    s = lse_rescale(s, m, nm) + lse_rescale(os, om, nm);
    m = nm;
}
hipError_t launch_greedy_select(const SelectParams& p, hipStream_t s);
hipError_t launch_beam_init(const SelectParams& p, hipStream_t s);       // beam scores 0 / -1e9, identity ancestry, empty hypothesis stores
hipError_t launch_beam_finalize(const SelectParams& p, hipStream_t s);   // BeamSearchScorer.finalize into beam.out_ids / out_scores (idempotent)
hipError_t launch_dec_init(DecState* st, int* ids, int* unfinished, int B, int max_length, int start_token, int epoch, hipStream_t s);
// continuous mode: empty slots, empty queue
hipError_t launch_stream_init(DecState* st, int* unfinished, int B, int epoch, hipStream_t s);
// continuous mode: append `n` prepared utterances (cross-cache pool rows, forced-EOS steps) to the waiting queue and admit into idle slots
struct StreamPublish {
    int n;
    int rows[MAX_ROWS];
    int force[MAX_ROWS];
};
hipError_t launch_stream_publish(const SelectParams& p, const StreamPublish& pub, hipStream_t s);
hipError_t launch_copy_cache_rows(const float* src, float* dst, int LH, int src_rows, int dst_rows, int n_rows,
                                  hipStream_t s);
hipError_t launch_set_state(DecState* st, int cur_len, int pos, int self_len, hipStream_t s);

// ---- SkinnyParams / SelectParams of the greedy step's fused launches.  engine.hip and the debug hooks (debug_api.hip) both build their
// launches here, so a test of a hook (tests/test_gpu_select.py) is a test of what the engine launches.
// LayerNorm + fused q|k|v projection of one decoder layer: q (scaled by head_dim^-0.5) -> q [B][d], the k / v rows appended in place at
// st->self_len[b] into the layer's self caches [B][H][s_cap][64] (float, or IEEE half with kv_half)
inline SkinnyParams qkv_append_skinny_params(const float* h, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* q,
                                             void* kcache, void* vcache, const DecState* st, int B, int d, int s_cap, int w_nt, int w_half,
                                             int kv_half) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = h; k.ln_w = ln_w; k.ln_b = ln_b; k.xmode = XMODE_LAYERNORM; k.W = (const float*)W; k.bias = bias;
    k.Y = q; k.kcache = (float*)kcache; k.vcache = (float*)vcache; k.st = st; k.B = B; k.N = 3 * d; k.K = d; k.ymode = YMODE_QKV_APPEND;
    k.d_model = d; k.s_cap = s_cap; k.q_scale = 0.125f; k.w_nt = w_nt; k.w_half = w_half; k.kv_half = kv_half;
    return k;
}
// The folded cross-attention query u = fold_w . [a ; h] + fold_c in two launches (d <= 1024): the half that multiplies the layer input h
// rides in the q|k|v launch (uh = fold_wh . h + fold_c, h raw), the half that multiplies the self-attention context `a` stays in the pair
// launch with uh as its residual (u = fold_wa . a + uh).  fold_wa / fold_wh: columns [0, d) / [d, 2d) of fold_w as contiguous [d][d].
inline SkinnyParams qfold_resid_skinny_params(const float* h, const void* fold_wh, const float* fold_c, float* uh, const DecState* st, int B,
                                              int d, int w_nt, int w_half) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = h; k.xmode = XMODE_PLAIN; k.W = (const float*)fold_wh; k.bias = fold_c; k.Y = uh; k.st = st; k.B = B; k.N = d; k.K = d;
    k.q_scale = 1.f; k.w_nt = w_nt; k.w_half = w_half;
    return k;
}
// `a`: the context rows [B][d], or, with `parts`, the two split partials of the self-attention (SkinnyParams.parts, H = d / 64)
inline SkinnyParams qfold_ctx_skinny_params(const float* a, const float* parts, const void* fold_wa, const float* uh, float* u,
                                            const DecState* st, int B, int d, int w_nt, int w_half) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = a; k.xmode = XMODE_PLAIN; k.W = (const float*)fold_wa; k.resid = uh; k.Y = u; k.st = st; k.B = B; k.N = d; k.K = d;
    k.q_scale = 1.f; k.w_nt = w_nt; k.w_half = w_half;
    if (parts) { k.parts = parts; k.parts_nsplit = 2; k.parts_H = d / HEAD_DIM; }
    return k;
}
// final LayerNorm + vocabulary projection (no bias): plain logits [B][V] ...
inline SkinnyParams vocab_skinny_params(const float* h, const float* ln_w, const float* ln_b, const void* W, float* logits, const DecState* st,
                                        int B, int V, int d, int w_nt, int w_half) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = h; k.ln_w = ln_w; k.ln_b = ln_b; k.xmode = XMODE_LAYERNORM; k.W = (const float*)W; k.Y = logits;
    k.st = st; k.B = B; k.N = V; k.K = d; k.q_scale = 1.f; k.w_nt = w_nt; k.w_half = w_half;
    return k;
}
// ... or Suppress -> SuppressAtBegin -> argmax in the epilogue (Force / pad / EOS rules: greedy_finish_kernel): one partial per row and
// workgroup into sp.part_val / part_idx [B][grid], the raw logits into sp.trace when set.  Returns the workgroup count (-1: no plan);
// greedy_select_fused hands it to the finish kernel.
inline int vocab_skinny_fuse_argmax(SkinnyParams& k, const SelectParams& sp) {
    k.ymode = YMODE_ARGMAX; k.Y = nullptr; k.am_mask = sp.mask; k.am_val = sp.part_val; k.am_idx = sp.part_idx;
    k.am_begin_index = sp.begin_index; k.am_trace = sp.trace; k.am_trace_steps = sp.max_length - 1;
    if (sp.lp_on) {
        k.am_lp = sp.lp_ns >= 0 ? 2 : 1; k.am_lse = sp.lp_part; k.am_side = sp.lp_side; k.am_eos = sp.eos; k.am_ns = sp.lp_ns;
        if (sp.samp_on) {
            k.am_samp = 1; k.am_temp = sp.samp_temp; k.am_seeds = sp.samp_seeds; k.am_sc = sp.samp_sc;
        }
    }
    const int grid = skinny_grid(k);
    k.am_ld = grid;
    return grid;
}
// the first step's language detection on the final hidden state `h` (the residual stream the vocabulary stage normalises too)
inline LangSelectParams lang_select_params(const float* h, const float* ln_w, const float* ln_b, const void* emb, int emb_half, const int* lang_ids,
                                           int n_lang, int B, int d, int* lang_tok, float* lang_prob) {
    LangSelectParams p;
    memset(&p, 0, sizeof p);
    p.x = h; p.ln_w = ln_w; p.ln_b = ln_b; p.emb = (const float*)emb; p.emb_half = emb_half ? 1 : 0; p.lang_ids = lang_ids; p.n_lang = n_lang;
    p.B = B; p.d = d; p.lang_tok = lang_tok; p.lang_prob = lang_prob;
    return p;
}
inline void greedy_select_fused(SelectParams& sp, int parts) { sp.fused = 1; sp.n_parts = parts; }
// the plain greedy tail (greedy_select_kernel's SELECT_CHUNKS partials unless greedy_select_fused follows, then greedy_finish_kernel)
inline void greedy_select_params(SelectParams& sp, const float* logits, const uint8_t* mask, const int* forced, int* ids, int* unfinished,
                                 DecState* st, float* trace, float* part_val, int* part_idx, const void* tok_emb, const float* pos_emb,
                                 float* next_x, int d, int emb_half, int B, int V, int max_length, int begin_index, int eos, int pad,
                                 int force_eos_step, const int* force_eos_rows, unsigned long long* mailbox, int start_token) {
    memset(&sp, 0, sizeof sp);
    sp.logits = logits; sp.mask = mask; sp.forced = forced; sp.ids = ids; sp.unfinished = unfinished;
    sp.st = st; sp.trace = trace; sp.B = B; sp.V = V; sp.max_length = max_length;
    sp.begin_index = begin_index; sp.eos = eos; sp.pad = pad; sp.force_eos_step = force_eos_step;
    sp.part_val = part_val; sp.part_idx = part_idx; sp.tok_emb = (const float*)tok_emb; sp.pos_emb = pos_emb; sp.next_x = next_x;
    sp.d_model = d; sp.n_parts = SELECT_CHUNKS; sp.fused = 0; sp.emb_half = emb_half;
    sp.force_eos_rows = force_eos_rows; sp.mailbox = mailbox;
    sp.start_token = start_token;
    sp.lang_pos = -1;
}

// ---- GemmParams of the encoder's two convolutions and of the cross-K/V projection.  engine.hip and the debug hooks (debug_api.hip) both
// build their launches here, so a test of a hook is a test of what the engine launches.
// Conv workspace (per utterance b of B, Fr = 2 S frames): melT [B][Fr + 2][C] and c1 [B][Fr + 2][d], row t + 1 = frame t, rows 0 and
// Fr + 1 the convolutions' zero padding, then 4 rows of slack; conv_ws_elems gives their elements.  CONV_X3 keeps both as three bf16 planes
// (plane p at + p * elements), CONV_F16 as IEEE half, CONV_F32 as float.  conv1 (k 3, pad 1, GELU) reads melT and writes c1's rows 1..Fr;
// conv2 (k 3, stride 2, pad 1, GELU, + pos) reads c1 with lda = 2d and writes out [B][S][d] (float).
enum { CONV_F32 = 0, CONV_X3 = 1, CONV_F16 = 2 };
inline void conv_ws_elems(int B, int S, int C, int d, size_t& n_melT, size_t& n_c1) {
    const size_t rows = (size_t)B * (2 * (size_t)S + 2);
    n_melT = rows * C + 4 * (size_t)C;
    n_c1 = rows * d + 4 * (size_t)d;
}
// zero melT and c1 (their pad rows are never written by the kernels); esz: bytes per element of the whole buffer (4 fp32 -- the fp16
// engines clear their half data in the same fp32-sized region --, 6 for three bf16 planes)
inline hipError_t conv_ws_clear(void* melT, size_t n_melT, void* c1, size_t n_c1, size_t esz, hipStream_t s) {
    hipError_t e = hipMemsetAsync(melT, 0, n_melT * esz, s);
    return e == hipSuccess ? hipMemsetAsync(c1, 0, n_c1 * esz, s) : e;
}
// w1 / w2: conv weights as the converter lays them out ([d][3 C] / [d][3 d], builder._conv_as_gemm): float, half, or plane 0 of three bf16 planes
inline void conv_gemm_params(int mode, const void* melT, size_t n_melT, void* c1, size_t n_c1, const void* w1, const float* b1, const void* w2,
                             const float* b2, const float* pos, float* out, int B, int S, int C, int d, GemmParams& c1g, GemmParams& c2g) {
    const int Fr = 2 * S;
    const size_t esz = mode == CONV_F32 ? 4 : 2;
    memset(&c1g, 0, sizeof c1g);
    c1g.A = (const float*)melT; c1g.lda = C; c1g.a_rows_per_batch = Fr; c1g.a_batch_stride = (long long)(Fr + 2) * C;
    c1g.W = (const float*)w1; c1g.bias = b1; c1g.M = B * Fr; c1g.N = d; c1g.K = 3 * C; c1g.act = 1;
    c1g.C = (float*)((char*)c1 + (size_t)d * esz); c1g.ldc = d; c1g.c_rows_per_batch = Fr; c1g.c_batch_stride = (long long)(Fr + 2) * d;
    memset(&c2g, 0, sizeof c2g);
    c2g.A = (const float*)c1; c2g.lda = 2 * d; c2g.a_rows_per_batch = S; c2g.a_batch_stride = (long long)(Fr + 2) * d;
    c2g.W = (const float*)w2; c2g.bias = b2; c2g.M = B * S; c2g.N = d; c2g.K = 3 * d; c2g.act = 1; c2g.pos = pos;
    c2g.C = out; c2g.ldc = d; c2g.c_rows_per_batch = S; c2g.c_batch_stride = (long long)S * d;
    if (mode == CONV_X3) {   // conv1's GELU output goes out as planes for conv2
        c1g.a_plane = (long long)n_melT; c1g.w_plane = (long long)d * 3 * C; c1g.out_split = 1; c1g.c_plane = (long long)n_c1;
        c2g.a_plane = (long long)n_c1; c2g.w_plane = (long long)d * 3 * d;
    }
}
// Cross-K/V projection of ONE decoder layer: encoder rows [0, rows) of each of B utterances (A [B][rows_total][d], float or half) times
// W [2d][d] into the head-split caches [layer_rows][H][cap][64] of that layer (ck / cv: the layer's base), utterance b at cache row
// row0 + b, sequence rows [seq_off, seq_off + rows); kv_esz bytes per cache element.  The x3 form: cross_kv_x3 on top.
inline GemmParams cross_kv_gemm_params(const void* A, int rows_total, const void* W, const float* bias, void* ck, void* cv, int kv_esz, int B,
                                       int rows, int H, int cap, int seq_off, int row0) {
    const int d = H * HEAD_DIM;
    const size_t row_off = (size_t)row0 * H * cap * HEAD_DIM * kv_esz;
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = (const float*)A; g.lda = d; g.a_rows_per_batch = rows; g.a_batch_stride = (long long)rows_total * d;
    g.W = (const float*)W; g.bias = bias; g.M = B * rows; g.N = 2 * d; g.K = d;
    g.epi = EPI_KV_HEADS; g.C = (float*)((char*)ck + row_off); g.C2 = (float*)((char*)cv + row_off);
    g.c_rows_per_batch = rows; g.kv_heads = H; g.kv_cap = cap; g.kv_seq_off = seq_off;
    return g;
}
// A3: the encoder rows as three bf16 planes of a_plane elements each (split3 of A), W3: the layer's weights as three planes of 2 d^2
inline void cross_kv_x3(GemmParams& g, const void* A3, size_t a_plane, const void* W3) {
    g.A = (const float*)A3; g.a_plane = (long long)a_plane; g.W = (const float*)W3; g.w_plane = 2ll * g.K * g.K;
}

// GELU (erf form) of the encoder epilogues.  erff() is ~38 vector ALU instructions in two divergent branches, executed beside the other
// workgroups' MFMAs: 10 % of a small.en fc1 launch, 4 % of medium.en's.  Branch-free form: erf(|x| / sqrt 2) = 1 - 2^Q(|x|), Q of degree 8
// without constant term (coefficients and error check: tools/fit_gelu.py), and
//   gelu(x) = x - h for x >= 0,  h for x < 0,  h = 0.5 x 2^Q(|x|)       (no 1 + erf cancellation in the negative tail)
// 13 instructions + one v_exp_f32.  |gelu_erf - exact| <= 5.1e-7 on [-12, 12] in float32 arithmetic, <= 1.3e-7 max(|x|, 1): one ulp of the
// result, the size of the rounding of x - h itself.
__device__ __forceinline__ float gelu_erf(float x) {
    const float t = fabsf(x);   // no clamp: beyond the fitted range Q(t) t keeps falling monotonically to -inf (checked in fit_gelu.py), 2^Q -> 0
    float q = -2.835055965988431e-06f;
    q = fmaf(q, t, 3.937911969842389e-05f);
    q = fmaf(q, t, -0.00018618583271745592f);
    q = fmaf(q, t, -0.00013692546053789556f);
    q = fmaf(q, t, 0.007063408847898245f);
    q = fmaf(q, t, -0.05249617248773575f);
    q = fmaf(q, t, -0.4592081904411316f);
    q = fmaf(q, t, -1.1511051654815674f);
    const float h = (0.5f * x) * __builtin_amdgcn_exp2f(q * t);
    // (fmaxf: gelu(x) >= x / 2 for x >= 0, so the max is an identity for finite x; for x = +inf, where h = inf * 0 = NaN, it returns +inf
    //  like the erf form.  x = -inf gives NaN in both forms, NaN stays NaN.)
    return x >= 0.f ? fmaxf(x - h, 0.5f * x) : h;
}

}  // namespace wt
