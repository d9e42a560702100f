// Host-only logic of the C-ABI: serialized-engine ("weight pack") parsing, config validation, the Session-style
// shape inference and the decode configuration (what a decode may combine, and what its step graph depends on).  No HIP types or calls: this file and host_logic.cpp also build with plain g++ under
// -fsanitize=address,undefined for the CPU tests (tests/native/fuzz_host_logic.cpp, tests/test_host_sanitizer.py; tests/native/test_decode_config.cpp,
// tests/test_decode_config_host.py).
// Reference call sites replaced: tensorrt_llm/runtime/session.py:54 (from_serialized_engine) and :116-146 (infer_shapes).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/whisper_trtllm_amd.h"

namespace wt {

constexpr int HEAD_DIM = 64;  // every Whisper size uses 64-wide heads (d_model / n_heads)
constexpr int MAX_ROWS = 16;       // decode slots per engine call
constexpr int STREAM_QCAP = 256;   // continuous mode: ring of waiting utterances, and the largest cross-cache pool (rows)
constexpr int MAX_BEAMS = 8;
constexpr int TT_MAX_HEADS = 32;
constexpr int TT_MAX_WIDTH = 15;
constexpr int TT_MAX_TOKENS = 1024;   // N of one DTW workgroup (one thread per token row)
constexpr int LANG_MAX = 128;         // language ids of wt_decoder_set_languages (lang_select_kernel stages one logit per id in LDS)

// ---- serialized engine layout, written by whisper-trtllm_amd/engine_pack.py --------------------------------
// [BlobHeader][BlobTensor * n_tensors][raw tensor bytes, each 256-byte aligned]
struct BlobHeader {
    char magic[8];  // "WTENGINE"
    uint32_t version, kind, precision, n_tensors;
    int32_t cfg[24];  // see CFG_* below
    uint64_t table_off, data_off, total_bytes;
};
struct BlobTensor {
    char name[96];
    uint32_t dtype, ndim;
    int64_t shape[4];
    uint64_t offset, nbytes;  // offset from blob start
};
static_assert(sizeof(BlobHeader) == 144, "blob header layout");
static_assert(sizeof(BlobTensor) == 152, "blob tensor layout");
enum { CFG_D_MODEL = 0, CFG_HEADS, CFG_LAYERS, CFG_FFN, CFG_MELS, CFG_SRC_POS, CFG_TGT_POS, CFG_VOCAB, CFG_TIED };
constexpr uint32_t BLOB_VERSION = 2;

struct EngineDims {
    int kind = 0, precision = 0;
    int d = 0, H = 0, L = 0, F = 0, C = 0, S = 0, T = 0, V = 0, tied = 0;
};

struct ParsedBlob {
    BlobHeader hd;
    EngineDims dims;
    std::vector<BlobTensor> tensors;  // validated: in-bounds, aligned, known dtype, shape x element size == nbytes
};

// Every check is overflow-safe (no sum of file-controlled 64-bit terms).  Returns WT_OK or a WT_E_* code with a message in err.
int parse_blob(const void* blob, size_t nbytes, ParsedBlob* out, char* err, size_t errlen);

// shapes remembered between infer_shapes and run (Session keeps them in the execution context, session.py:137-146)
struct ShapeState {
    bool ok = false;
    int c_B = 1, c_s = 0, c_ms = 0, c_mc = 0;
};
int infer_shapes(const EngineDims& e, const wt_tensor_desc* in, int n_in, wt_tensor_desc* out, int* n_out, ShapeState* st,
                 char* err, size_t errlen);

// ---- decode configuration -------------------------------------------------------------------------------------
// What the wt_decoder_set_* calls asked for; the next wt_decoder_begin / wt_decoder_stream_begin resolves it.  Only the setters write it.
struct DecodeRequest {
    wt_timestamp_params ts = {0, 0, 0, 0, 0};   // enabled == 0: off
    wt_logprob_params lp = {0, -1};             // enabled == 0: off
    float samp_temp = 0.f;                      // 0: greedy
    unsigned long long samp_seed = 0;
    std::vector<unsigned long long> samp_seeds; // the seed list when samp_list, else unused (seed + row)
    bool samp_list = false;
    wt_beam_params beam = {1, 1.f, 0};          // num_beams <= 1: off
    struct TokTs {                              // n_sel == 0: off
        int n_sel = 0, width = 7;
        double time_precision = 0.02;
        int layer[TT_MAX_HEADS] = {}, head[TT_MAX_HEADS] = {};
    } tt;
    std::vector<int> prompt;                    // [prompt_rows][prompt_len]; len 0: off
    int prompt_rows = 0, prompt_len = 0;
    std::vector<int> prompt_lens;               // wt_decoder_set_prompt_rows: tokens of each row of `prompt` ([prompt_rows][prompt_len]); empty: every row holds prompt_len
    std::vector<int> lang_ids;                  // wt_decoder_set_languages: the language token ids; empty: off
    std::vector<int> lang_rows;                 // ... and the rows' own: a listed id, or negative = detect; empty: detect every row
};

// Exactly the values a captured step graph bakes into kernel arguments: the graphs are replayed while the key of the decode in flight
// equals the key they were captured under, and dropped when it does not (enqueue_steps).  A POD created zero-filled, padding included
// (resolve_decode_config), so that two keys compare bytewise.  NOT in it, because no captured launch carries them: the contents of the
// suppress / forced tables, the per-row forced lengths and the language tables (device tables at fixed addresses), the seeds (a device table), the prompt
// (prefilled before the first step; the steps read positions from the device state) and the median width / time precision of the
// token timestamps (arguments of the post-pass only).
struct StepKey {
    int B, max_length, begin_index, eos, pad, start_token, force_eos_step, force_rows_on;
    float* logits_trace;
    wt_timestamp_params ts;
    wt_beam_params beam;       // num_beams <= 1: off ({1, 1.f, 0})
    int beam_group;            // > 1: the cross-attention of the beam decode runs the grouped form (num_beams 2 or 4)
    wt_logprob_params lp;      // on for a sampled decode too: the sampling kernels are forms of the log-probability mode's
    float samp_temp;           // 0: greedy
    struct {
        int n_sel, layer[TT_MAX_HEADS], head[TT_MAX_HEADS];
    } tt;                      // token-level timestamps: the alignment heads (n_sel == 0: off) ...
    int tt_rows, tt_steps;     // ... and the query history's dimensions: rows = B, steps = max_length - 1 (0 when off)
    int nt_loads;              // stream weights and K/V with non-temporal loads
    int nsplit_self, nsplit_cross;
    unsigned workspace_gen;    // the engine's count of workspace (re)allocations: the graphs carry device and pinned addresses
    int lang_pos;              // per-row language tokens: the sequence position whose forced token is the row's own (prompt_len + 1), -1: off ...
    int n_lang;                // ... and the listed language ids (the first step's lang_select launch), 0: off
    int reserved;              // 0: rounds the struct up to its alignment, so that it has no padding at all
    bool operator==(const StepKey& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    bool operator!=(const StepKey& o) const { return !(*this == o); }
};

static_assert(sizeof(StepKey) == 8 * sizeof(int) + sizeof(float*) + sizeof(wt_timestamp_params) + sizeof(wt_beam_params) + sizeof(wt_logprob_params) +
                                     (12 + 2 * TT_MAX_HEADS) * sizeof(int), "StepKey has padding");

// The decode in flight: the step key, and what only the host or the post-pass reads.  A stream decode has every batch-only feature off.
struct DecodeConfig {
    StepKey key;
    bool stream;               // continuous mode (wt_decoder_stream_begin): key.B decode slots over pool_rows cross-cache rows
    int pool_rows;             // 0 in a batch decode
    int U;                     // utterances: key.B = U * num_beams
    int prompt_len, prompt_rows;   // decoder prompt: tokens in front of the start token (0: off) and the rows uploaded (1: shared, or B)
    int prompt_ragged;             // per-row prompt lengths (wt_decoder_set_prompt_rows): prompt_len is then the longest of the batch's rows, ...
    int prompt_lens[MAX_ROWS];     // ... these are the rows' own, and the id rows are left-padded to prompt_len
    int tt_width;              // token timestamps: median filter width and seconds per encoder frame
    double tt_time_precision;
    int lang_detect;               // per-row language tokens: some row's entry is negative, so the first step runs lang_select_kernel
    int lang_ids[LANG_MAX];        // the key.n_lang listed ids ...
    int lang_rows[MAX_ROWS];       // ... and the rows' entries as the host uploads them (a listed id, or -1 = detect)
};

// What resolve_decode_config needs to know of the engine beyond its dimensions, and the A/B tuning switches (it reads no environment).
struct DecodeFacts {
    bool w_half = false;       // fp16 decoder engine
    int kv_esz = 4;            // bytes per element of the resident caches
    int nsplit_self = 1;       // WT_NSPLIT_SELF (unset: 1)
    bool nsplit_cross_set = false;
    int nsplit_cross = 0;      // WT_NSPLIT_CROSS, when set
    bool no_defer_merge = false;       // WT_NO_DEFER_MERGE
    bool beam_cross_grouped = false;   // WT_BEAM_CROSS=grouped
};

int pick_splits(int B, int H, int len);   // key splits of the cross-attention launch

// The one place that decides whether the request, the call's parameters and the engine go together, and what the decode then runs with:
// every compatibility and range check of wt_decoder_begin (`rows` utterances) and wt_decoder_stream_begin (`rows` slots over `pool_rows`
// cache rows, <= 0: 4 x slots), the token-id checks of the rule tables, B = U * num_beams, "sampling on" -> "log-probability kernels on",
// the language tables (ids inside the vocabulary, distinct, none the EOS id, row entries negative or listed),
// and the arithmetic tuning choices (nt_loads, the key splits, beam_group).  Pure.  Returns WT_OK or a WT_E_* code with a message in err;
// *out is complete only on WT_OK (key.workspace_gen stays 0: the engine fills it where it compares keys).
int resolve_decode_config(const EngineDims& e, const DecodeFacts& f, const DecodeRequest& r, const wt_greedy_params* p, int rows, int pool_rows,
                          bool stream, DecodeConfig* out, char* err, size_t errlen);

}  // namespace wt
