// Host-only logic of the C-ABI (see host_logic.h).  Plain C++17, no HIP: also built with g++ -fsanitize=address,undefined
// by the CPU test-suite and driven with mutated blobs.
#include "host_logic.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

namespace wt {

static int fail(char* err, size_t errlen, int code, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return code;
}

int parse_blob(const void* blob, size_t nbytes, ParsedBlob* out, char* err, size_t errlen) {
    if (!blob || !out) return fail(err, errlen, WT_E_INVALID, "parse_blob: null argument");
    out->tensors.clear();
    if (nbytes < sizeof(BlobHeader)) return fail(err, errlen, WT_E_INVALID, "engine blob too small (%zu bytes)", nbytes);
    BlobHeader& hd = out->hd;
    memcpy(&hd, blob, sizeof hd);
    if (memcmp(hd.magic, "WTENGINE", 8) != 0) return fail(err, errlen, WT_E_INVALID, "engine blob has bad magic");
    if (hd.version != BLOB_VERSION)
        return fail(err, errlen, WT_E_UNSUPPORTED, "engine blob version %u not supported (this library reads version %u; rebuild the engine)",
                    hd.version, BLOB_VERSION);
    // bounds: never add two file-controlled 64-bit numbers; compare against what is left instead
    const uint64_t n64 = (uint64_t)nbytes;
    bool ok = hd.total_bytes == n64 && hd.table_off >= sizeof(BlobHeader) && hd.table_off <= n64 &&
              (uint64_t)hd.n_tensors <= (n64 - hd.table_off) / sizeof(BlobTensor);
    uint64_t table_end = 0;
    if (ok) {
        table_end = hd.table_off + (uint64_t)hd.n_tensors * sizeof(BlobTensor);  // <= n64 by the check above
        ok = hd.data_off >= table_end && hd.data_off <= n64 && (hd.data_off & 15) == 0;
    }
    if (!ok)
        return fail(err, errlen, WT_E_INVALID, "engine blob is truncated or corrupt (header says %llu bytes, got %zu)",
                    (unsigned long long)hd.total_bytes, nbytes);
    if (hd.kind != WT_KIND_ENCODER && hd.kind != WT_KIND_DECODER) return fail(err, errlen, WT_E_INVALID, "unknown engine kind %u", hd.kind);
    if (hd.precision != WT_F32 && hd.precision != WT_F16)
        return fail(err, errlen, WT_E_UNSUPPORTED, "engine precision %u: float32 or float16 (builder.py:55)", hd.precision);

    EngineDims& e = out->dims;
    e.kind = (int)hd.kind;
    e.precision = (int)hd.precision;
    e.d = hd.cfg[CFG_D_MODEL]; e.H = hd.cfg[CFG_HEADS]; e.L = hd.cfg[CFG_LAYERS]; e.F = hd.cfg[CFG_FFN];
    e.C = hd.cfg[CFG_MELS]; e.S = hd.cfg[CFG_SRC_POS]; e.T = hd.cfg[CFG_TGT_POS]; e.V = hd.cfg[CFG_VOCAB];
    e.tied = hd.cfg[CFG_TIED] != 0;
    auto bad = [&](const char* why) {
        return fail(err, errlen, WT_E_INVALID, "engine config invalid: %s (d=%d H=%d L=%d F=%d C=%d S=%d T=%d V=%d)", why, e.d, e.H,
                    e.L, e.F, e.C, e.S, e.T, e.V);
    };
    if (e.d <= 0 || e.H <= 0 || e.H > 16 || e.d != e.H * HEAD_DIM) return bad("head_dim must be 64, at most 16 heads");
    if (e.d > 1024 || (e.d & 3)) return bad("d_model must be a multiple of 4 and <= 1024");
    if (e.L <= 0 || e.L > 64 || e.F <= 0 || (e.F & 3) || e.F > 4096) return bad("ffn_dim must be a multiple of 4 and <= 4096, 1..64 layers");
    if (e.S <= 0 || e.S > 4096 || e.C <= 0 || e.C > 128 || (e.C & 3)) return bad("num_mel_bins must be a multiple of 4 and <= 128, max_source_positions <= 4096");
    if (e.kind == WT_KIND_DECODER && (e.T <= 1 || e.T > 4096 || e.V <= 0 || e.V > (1 << 20))) return bad("decoder needs max_target_positions in 2..4096 and a vocabulary");
    if (e.precision == WT_F16 && e.kind == WT_KIND_ENCODER && ((e.C & 7) || (e.d & 7) || (e.F & 7) || e.F < e.d))
        return bad("float16 encoder needs num_mel_bins, d_model, ffn_dim multiples of 8 and ffn_dim >= d_model (workspace layout)");
    if (e.precision == WT_F16 && e.kind == WT_KIND_DECODER && ((e.d & 7) || (e.F & 7)))
        return bad("float16 decoder needs d_model and ffn_dim to be multiples of 8 (eight halves per 16-byte weight load)");

    const char* base = (const char*)blob;
    out->tensors.reserve(hd.n_tensors);
    for (uint32_t i = 0; i < hd.n_tensors; ++i) {
        BlobTensor bt;
        memcpy(&bt, base + hd.table_off + (uint64_t)i * sizeof(BlobTensor), sizeof bt);
        bt.name[sizeof(bt.name) - 1] = 0;
        bool tok = bt.offset >= hd.data_off && bt.offset <= n64 && bt.nbytes <= n64 - bt.offset && (bt.offset & 15) == 0 &&
                   (bt.dtype == WT_F32 || bt.dtype == WT_F16) && bt.ndim <= 4;
        if (!tok) return fail(err, errlen, WT_E_INVALID, "tensor '%s' has a bad table entry", bt.name);
        // element count with an overflow guard: no dimension (and no partial product) may exceed the blob size
        uint64_t n = 1;
        for (uint32_t k = 0; k < bt.ndim && tok; ++k) {
            if (bt.shape[k] < 0 || (uint64_t)bt.shape[k] > n64) { tok = false; break; }
            if (bt.shape[k] != 0 && n > n64 / (uint64_t)bt.shape[k]) { tok = false; break; }
            n *= (uint64_t)bt.shape[k];
        }
        const uint64_t esz = bt.dtype == WT_F16 ? 2 : 4;
        if (!tok || n > n64 / esz || n * esz != bt.nbytes)
            return fail(err, errlen, WT_E_INVALID, "tensor '%s': shape and byte count disagree", bt.name);
        out->tensors.push_back(bt);
    }
    return WT_OK;
}

// --------------------------------------------------------------------------------------------- shape inference
static void set_desc(wt_tensor_desc* t, const char* name, int dtype, std::initializer_list<int64_t> shape) {
    memset(t, 0, sizeof *t);
    snprintf(t->name, sizeof t->name, "%s", name);
    t->dtype = dtype;
    t->ndim = (int)shape.size();
    int k = 0;
    for (int64_t s : shape) t->shape[k++] = s;
}

int infer_shapes(const EngineDims& e, const wt_tensor_desc* in, int n_in, wt_tensor_desc* out, int* n_out, ShapeState* st, char* err,
                 size_t errlen) {
    if ((!in && n_in) || n_in < 0 || !out || !n_out || !st) return fail(err, errlen, WT_E_INVALID, "wt_engine_infer_shapes: null argument");
    st->ok = false;
    auto find = [&](const char* name) -> const wt_tensor_desc* {
        for (int i = 0; i < n_in; ++i)
            if (strncmp(in[i].name, name, WT_NAME_LEN) == 0) return &in[i];
        return nullptr;
    };
    struct Spec { const char* name; int dtype; };
    static const Spec enc_in[] = {{"data", WT_F32}, {"length", WT_F32}};
    static const Spec dec_in[] = {{"data", WT_I32}, {"length", WT_I32}, {"encoder_hidden_states", WT_F32},
                                  {"self_past_key", WT_F32}, {"self_past_value", WT_F32}, {"cross_past_key", WT_F32},
                                  {"cross_past_value", WT_F32}, {"past_self_cache_mask", WT_F32}, {"past_cross_cache_mask", WT_F32}};
    const Spec* specs = e.kind == WT_KIND_ENCODER ? enc_in : dec_in;
    const int nspec = e.kind == WT_KIND_ENCODER ? 2 : 9;
    for (int i = 0; i < n_in; ++i) {  // session.py:128-136: unknown name / wrong dtype -> error
        const Spec* sp = nullptr;
        for (int k = 0; k < nspec; ++k)
            if (strncmp(in[i].name, specs[k].name, WT_NAME_LEN) == 0) sp = &specs[k];
        if (!sp) return fail(err, errlen, WT_E_NOTFOUND, "Tensor:%.*s is not an input tensor", WT_NAME_LEN, in[i].name);
        if (sp->dtype != in[i].dtype) return fail(err, errlen, WT_E_INVALID, "Tensor:%.*s has wrong dtype", WT_NAME_LEN, in[i].name);
        if (in[i].ndim < 0 || in[i].ndim > WT_MAX_DIMS) return fail(err, errlen, WT_E_INVALID, "Tensor:%.*s has a bad rank", WT_NAME_LEN, in[i].name);
    }
    auto shape_is = [](const wt_tensor_desc* t, std::initializer_list<int64_t> want) {
        if (!t || t->ndim != (int)want.size()) return false;
        int k = 0;
        for (int64_t s : want) {
            if (s >= 0 && t->shape[k] != s) return false;
            ++k;
        }
        return true;
    };
    if (e.kind == WT_KIND_ENCODER) {
        const wt_tensor_desc* data = find("data");
        if (!shape_is(data, {-1, e.C, 2 * e.S}) || data->shape[0] < 1 || data->shape[0] > (1 << 16))
            return fail(err, errlen, WT_E_INVALID, "encoder input 'data' must be f32 [B,%d,%d]", e.C, 2 * e.S);
        if (*n_out < 1) return fail(err, errlen, WT_E_INVALID, "output descriptor capacity too small");
        st->c_B = (int)data->shape[0];
        set_desc(&out[0], "hidden_states", WT_F32, {data->shape[0], e.S, e.d});
        *n_out = 1;
        st->ok = true;
        return WT_OK;
    }
    const int64_t L = e.L, H = e.H, S = e.S;
    if (!shape_is(find("data"), {1, 1}))
        return fail(err, errlen, WT_E_INVALID, "decoder input 'data' must be i32 [1,1] (batch_size and id_len are fixed to 1, model.py:474-477)");
    if (!shape_is(find("encoder_hidden_states"), {1, S, e.d}))
        return fail(err, errlen, WT_E_INVALID, "'encoder_hidden_states' must be f32 [1,%d,%d]", (int)S, e.d);
    const wt_tensor_desc *spk = find("self_past_key"), *spv = find("self_past_value");
    if (!shape_is(spk, {L, H, -1, HEAD_DIM}) || !shape_is(spv, {L, H, -1, HEAD_DIM}) || spk->shape[2] != spv->shape[2] ||
        spk->shape[2] < 1 || spk->shape[2] > e.T + 1)
        return fail(err, errlen, WT_E_INVALID, "'self_past_key/value' must be f32 [%d,%d,s,64] with 1 <= s <= %d", (int)L, (int)H, e.T + 1);
    if (!shape_is(find("cross_past_key"), {L, H, S, HEAD_DIM}) || !shape_is(find("cross_past_value"), {L, H, S, HEAD_DIM}))
        return fail(err, errlen, WT_E_INVALID, "'cross_past_key/value' must be f32 [%d,%d,%d,64]", (int)L, (int)H, (int)S);
    const wt_tensor_desc *ms = find("past_self_cache_mask"), *mc = find("past_cross_cache_mask");
    if (!ms || ms->ndim != 1 || ms->shape[0] < 1 || ms->shape[0] > e.T + 1)
        return fail(err, errlen, WT_E_INVALID, "'past_self_cache_mask' must be f32 [m_s], 1 <= m_s <= %d", e.T + 1);
    if (!mc || mc->ndim != 1 || mc->shape[0] < 1 || mc->shape[0] > S + 1)
        return fail(err, errlen, WT_E_INVALID, "'past_cross_cache_mask' must be f32 [m_c], 1 <= m_c <= %d", (int)S + 1);
    if (ms->shape[0] - 1 >= e.T) return fail(err, errlen, WT_E_INVALID, "position %d exceeds max_target_positions %d", (int)ms->shape[0] - 1, e.T);
    if (*n_out < 5) return fail(err, errlen, WT_E_INVALID, "output descriptor capacity too small");
    st->c_s = (int)spk->shape[2];
    st->c_ms = (int)ms->shape[0];
    st->c_mc = (int)mc->shape[0];
    const int64_t cache_len = st->c_ms - 1 < st->c_s ? st->c_ms - 1 : st->c_s;  // model.py:278
    set_desc(&out[0], "hidden_states", WT_F32, {1, 1, e.V});
    set_desc(&out[1], "next_self_keys", WT_F32, {L, H, cache_len + 1, HEAD_DIM});
    set_desc(&out[2], "next_self_values", WT_F32, {L, H, cache_len + 1, HEAD_DIM});
    set_desc(&out[3], "next_cross_keys", WT_F32, {L, H, S, HEAD_DIM});
    set_desc(&out[4], "next_cross_values", WT_F32, {L, H, S, HEAD_DIM});
    *n_out = 5;
    st->ok = true;
    return WT_OK;
}

// --------------------------------------------------------------------------------------------- decode configuration
int pick_splits(int B, int H, int len) {
    // Key splits of the cross-attention launch.  Two splits are merged for free by the consuming GEMV (deferred merge), more
    // are merged by the attention kernel's last-arriving block, which costs ~2 us: measured on medium.en, ms per step at
    // B = 1: 16 splits 1.25, 8: 1.12, 4: 1.09, 2: 1.14;  B = 2: 8: 1.16, 4: 1.12, 2: 1.15;  B = 4: 4: 1.27, 2: 1.26;
    // B = 8: 2: 1.47, 3: 1.76, 4: 1.80.  So: 4 while (utterance, head) pairs are scarce (<= 64), else 2, none from 256 pairs up.
    int n = (256 + B * H - 1) / (B * H);
    n = n >= 4 ? 4 : n >= 2 ? 2 : 1;   // (tiny.en B = 8, 48 pairs: 4 splits 0.218, 2 splits 0.225; small.en B = 8, 96 pairs: 2 splits 0.693, 4: 0.706)
    while (n > 1 && len / n < 48) n >>= 1;
    return n;
}

int resolve_decode_config(const EngineDims& e, const DecodeFacts& f, const DecodeRequest& r, const wt_greedy_params* p, int rows, int pool_rows,
                          bool stream, DecodeConfig* out, char* err, size_t errlen) {
    if (!p || !out || rows < 1) return fail(err, errlen, WT_E_INVALID, "resolve_decode_config: bad arguments");
    memset(out, 0, sizeof *out);   // padding included: StepKey compares bytewise
    StepKey& k = out->key;
    const char* who = stream ? "wt_decoder_stream_begin" : "wt_decoder_begin";
    const int nb = !stream && r.beam.num_beams > 1 ? r.beam.num_beams : 1;
    int B = rows;
    if (stream) {
        if (pool_rows <= 0) pool_rows = 4 * rows;     // slots decoding + 3 x slots prepared ahead
        if (pool_rows < rows + 1 || pool_rows > STREAM_QCAP)
            return fail(err, errlen, WT_E_INVALID, "wt_decoder_stream_begin: pool of %d rows outside [slots + 1, %d]", pool_rows, STREAM_QCAP);
        if (r.ts.enabled) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: timestamp mode is a batch-decode feature (wt_decoder_begin)");
        if (r.beam.num_beams > 1) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: beam search is a batch-decode feature (wt_decoder_begin)");
        if (r.tt.n_sel > 0) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: token-level timestamps are a batch-decode feature (wt_decoder_begin)");
        if (r.lp.enabled) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: token log-probabilities are a batch-decode feature (wt_decoder_begin)");
        if (r.samp_temp > 0.f) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: temperature sampling is a batch-decode feature (wt_decoder_begin)");
        if (r.prompt_len > 0) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: decoder prompts are a batch-decode feature (wt_decoder_begin)");
        if (!r.lang_ids.empty())
            return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: per-row language tokens are a batch-decode feature (wt_decoder_begin)");
        if (p->logits_trace || p->force_eos_step >= 0 || p->force_eos_steps)
            return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: logits_trace / force_eos_step(s) belong to wt_decoder_begin (per-utterance lengths: wt_decoder_stream_submit)");
    } else {
        pool_rows = 0;
        if (nb > 1) {   // beam search: `rows` utterances decode as rows * num_beams rows, [utterance][beam]
            if (r.ts.enabled) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: beam search and timestamp mode cannot be combined");
            if (r.tt.n_sel > 0)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: beam search and token-level timestamps cannot be combined (no beam_indices)");
            if (p->logits_trace || p->force_eos_step >= 0 || p->force_eos_steps)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: logits_trace / force_eos_step(s) are not available with beam search");
            if (r.lp.enabled)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: beam search and token log-probabilities cannot be combined (wt_decoder_read_beam_scores is the beams' score)");
            if (r.samp_temp > 0.f)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: beam search and temperature sampling cannot be combined");
            if (rows * nb > MAX_ROWS) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: %d utterances x %d beams > %d rows per call", rows, nb, MAX_ROWS);
            B = rows * nb;
        }
        // per-row lengths: the batch's longest row is the prompt length every batch-wide rule counts with (0: no row of this batch has a prompt)
        int plen = r.prompt_len;
        const bool ragged = plen > 0 && !r.prompt_lens.empty();
        if (ragged) {   // (too few rows for the batch: refused below, behind the combinations that are refused whatever the rows)
            plen = 0;
            for (int b = 0; b < B && b < (int)r.prompt_lens.size(); ++b) plen = r.prompt_lens[b] > plen ? r.prompt_lens[b] : plen;
            if ((int)r.prompt_lens.size() < B) plen = r.prompt_len;
        }
        out->prompt_len = plen;
        if (plen > 0) {
            if (f.w_half || f.kv_esz != 4)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: decoder prompts need an fp32 decoder engine (the prefill's GEMMs and attention are fp32)");
            if (nb > 1) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: a decoder prompt and beam search cannot be combined");
            if (r.tt.n_sel > 0)
                return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: a decoder prompt and token-level timestamps cannot be combined (their query history is "
                                                           "indexed by step and sized by the sequence length)");
            if (ragged && (r.prompt_rows < B || (int)r.prompt_lens.size() < B))
                return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: wt_decoder_set_prompt_rows gave %d prompt rows for a batch of %d", r.prompt_rows, B);
            if (r.prompt_rows != 1 && r.prompt_rows < B)
                return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: wt_decoder_set_prompt gave %d prompt rows for a batch of %d", r.prompt_rows, B);
            if (plen + 2 > p->max_length)
                return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: %d prompt tokens + the start token + one generated token > max_length %d", plen, p->max_length);
            out->prompt_rows = r.prompt_rows == 1 ? 1 : B;
            if (ragged) {
                out->prompt_ragged = 1;
                for (int b = 0; b < B; ++b) out->prompt_lens[b] = r.prompt_lens[b];
            }
        }
        if (r.samp_temp > 0.f && r.samp_list && (int)r.samp_seeds.size() < B)
            return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: wt_decoder_set_sampling gave %d seeds for a batch of %d", (int)r.samp_seeds.size(), B);
    }
    if (B > MAX_ROWS) return fail(err, errlen, WT_E_UNSUPPORTED, "%s: batch %d > %d per call; shard the batch", who, B, MAX_ROWS);
    if (p->max_length < 2 || p->max_length > e.T) return fail(err, errlen, WT_E_INVALID, "max_length %d outside [2, max_target_positions=%d]", p->max_length, e.T);
    auto tok_ok = [&](int t) { return t >= 0 && t < e.V; };
    if (!tok_ok(p->decoder_start_token_id) || !tok_ok(p->eos_token_id) || !tok_ok(p->pad_token_id))
        return fail(err, errlen, WT_E_INVALID, "start/eos/pad token id outside the vocabulary");
    for (int i = 0; i < p->n_suppress_tokens; ++i)
        if (!tok_ok(p->suppress_tokens[i])) return fail(err, errlen, WT_E_INVALID, "suppress token %d outside the vocabulary", p->suppress_tokens[i]);
    for (int i = 0; i < p->n_begin_suppress_tokens; ++i)
        if (!tok_ok(p->begin_suppress_tokens[i])) return fail(err, errlen, WT_E_INVALID, "begin-suppress token %d outside the vocabulary", p->begin_suppress_tokens[i]);
    if (r.ts.enabled) k.ts = r.ts;
    for (int i = 0; i < p->n_forced; ++i) {
        const int idx = p->forced_decoder_ids[2 * i], tok = p->forced_decoder_ids[2 * i + 1];
        if (!tok_ok(tok)) return fail(err, errlen, WT_E_INVALID, "forced token %d outside the vocabulary", tok);
        if (k.ts.enabled && (tok == k.ts.no_timestamps_token_id || idx >= k.ts.begin_index - 1))   // Force and Timestamp must not fight
            return fail(err, errlen, WT_E_INVALID, "timestamp mode: forced token %d at %d (no <|notimestamps|>, no forced position >= begin_index - 1 = %d)",
                        tok, idx, k.ts.begin_index - 1);
        if (nb > 1 && tok == p->eos_token_id)
            return fail(err, errlen, WT_E_INVALID, "beam search: forced token %d is the EOS token (no beam could continue)", tok);
    }
    k.lang_pos = -1;
    if (!r.lang_ids.empty()) {   // per-row language tokens (wt_decoder_set_languages): row b's forced token at position prompt + 1 is its own
        const int n = (int)r.lang_ids.size();
        if (nb > 1) return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: per-row language tokens and beam search cannot be combined");
        if (r.tt.n_sel > 0)
            return fail(err, errlen, WT_E_UNSUPPORTED, "wt_decoder_begin: per-row language tokens and token-level timestamps cannot be combined");
        if (n > LANG_MAX) return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: %d language ids > %d", n, LANG_MAX);
        for (int i = 0; i < n; ++i) {
            const int tok = r.lang_ids[i];
            if (!tok_ok(tok)) return fail(err, errlen, WT_E_INVALID, "language id %d outside the vocabulary", tok);
            if (tok == p->eos_token_id) return fail(err, errlen, WT_E_INVALID, "language id %d is the EOS token", tok);
            for (int j = 0; j < i; ++j)
                if (r.lang_ids[j] == tok) return fail(err, errlen, WT_E_INVALID, "language id %d listed twice", tok);
            out->lang_ids[i] = tok;
        }
        if (!r.lang_rows.empty() && (int)r.lang_rows.size() < B)
            return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: wt_decoder_set_languages gave %d row entries for a batch of %d", (int)r.lang_rows.size(), B);
        for (int b = 0; b < B; ++b) {
            const int tok = r.lang_rows.empty() ? -1 : r.lang_rows[b];
            bool listed = tok < 0;
            for (int i = 0; i < n && !listed; ++i) listed = r.lang_ids[i] == tok;
            if (!listed) return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: row %d's language token %d is not one of the listed ids", b, tok);
            out->lang_rows[b] = tok < 0 ? -1 : tok;
            if (tok < 0) out->lang_detect = 1;
        }
        k.lang_pos = out->prompt_len + 1;   // the position behind the start token; batch-wide also for ragged prompts (left-padded rows)
        k.n_lang = n;
        if (k.lang_pos >= p->max_length)
            return fail(err, errlen, WT_E_INVALID, "wt_decoder_begin: the language position %d lies outside max_length %d", k.lang_pos, p->max_length);
        if (k.ts.enabled && k.lang_pos >= k.ts.begin_index - 1)   // Force and Timestamp must not fight
            return fail(err, errlen, WT_E_INVALID, "timestamp mode: the language position %d is not in front of begin_index - 1 = %d", k.lang_pos, k.ts.begin_index - 1);
    }
    if (r.tt.n_sel > 0) {   // the query history the cross-attention launches fill: [n_sel][B][max_length - 1][64]
        if (p->max_length - 1 > TT_MAX_TOKENS) return fail(err, errlen, WT_E_UNSUPPORTED, "token timestamps: %d steps > %d", p->max_length - 1, TT_MAX_TOKENS);
        k.tt.n_sel = r.tt.n_sel;
        memcpy(k.tt.layer, r.tt.layer, sizeof k.tt.layer);
        memcpy(k.tt.head, r.tt.head, sizeof k.tt.head);
        k.tt_rows = B; k.tt_steps = p->max_length - 1;
        out->tt_width = r.tt.width; out->tt_time_precision = r.tt.time_precision;
    }
    k.B = B; k.max_length = p->max_length; k.begin_index = p->begin_index; k.eos = p->eos_token_id; k.pad = p->pad_token_id;
    k.start_token = p->decoder_start_token_id; k.force_eos_step = p->force_eos_step; k.force_rows_on = p->force_eos_steps ? 1 : 0;
    k.logits_trace = p->logits_trace;
    k.beam = nb > 1 ? r.beam : wt_beam_params{1, 1.f, 0};
    k.lp = r.lp;
    k.samp_temp = r.samp_temp > 0.f ? r.samp_temp : 0.f;
    if (k.samp_temp > 0.f) k.lp.enabled = 1;   // temperature sampling runs the log-probability mode's kernels in their sampling form
    out->stream = stream; out->pool_rows = pool_rows; out->U = rows;
    // measured (tools/microbench.py, medium.en B=8): self attention is fastest unsplit at every length <= 448;
    // cross attention (1500 keys) with ~one block per CU
    {   // Everything a step touches is read exactly once per step: stream it non-temporally -- unless one whole step (weights + this
        // batch's K/V) fits the 256 MB Infinity Cache, where default-policy loads let step t+1 hit what step t brought in.
        // Measured ms per step, non-temporal vs default: tiny.en B=1 (136 MB) 0.171 vs 0.160; tiny.en B=8 (300 MB) 0.224 vs 0.221;
        // base.en B=8 0.324 vs 0.340; small.en B=8 0.688 vs 0.711; medium.en B=8 1.61 vs 1.66.
        const double p_step = (double)e.L * (6.0 * e.d * e.d + 2.0 * e.d * e.F) + (double)e.V * e.d;
        const double step_bytes = (f.w_half ? 2.0 : 4.0) * p_step + (double)B * 2.0 * e.L * e.H * ((double)e.S + p->max_length) * HEAD_DIM * f.kv_esz;
        k.nt_loads = step_bytes > 160e6;
    }
    // self attention: unsplit.  Two key splits with the merge deferred into BOTH halves of the pair launch (WT_NSPLIT_SELF=2) are
    // implemented and tested, and measured a wash at medium.en batch 8: self-attention 9.0 -> 7.6 us at 447 keys, the pair launch
    // 8.2 -> 9.7 us (its blocks stage and merge two partial sets), 1.659 vs 1.649 ms per step in one A/B on one box.
    {
        const bool can_defer = !f.no_defer_merge && e.d <= 1024;
        k.nsplit_self = (f.nsplit_self == 2 && can_defer) ? 2 : 1;
    }
    {   // beam search: the cross-attention form.  The shared cache rows are read once per beam through slot_row (B blocks per head).  The
        // grouped form (one block per (utterance, head, split) carrying all beams; num_beams 2 and 4) measured SLOWER at medium.en 4 x 4:
        // 28.5 against 17.6 us per launch (per-row reading of 16 rows: 32.2), profiles/beam_cost.json -- it is kept as an A/B only:
        // WT_BEAM_CROSS=grouped (read per decode, so one handle can time both: tools/beam_cost.py).
        if (f.beam_cross_grouped && (nb == 2 || nb == 4)) k.beam_group = nb;
        if (nb > 1) k.nsplit_self = 1;   // the ancestry form is unsplit
    }
    {
        const int blocks = k.beam_group > 1 ? B / k.beam_group : B;   // blocks per head and split
        k.nsplit_cross = f.nsplit_cross_set ? f.nsplit_cross : pick_splits(blocks, e.H, e.S);
    }
    return WT_OK;
}

}  // namespace wt
