// CPU test of the decode configuration (csrc/host_logic.h: resolve_decode_config, StepKey).  Stand-alone: links host_logic.cpp only, built
// with g++ -fsanitize=address,undefined by tests/test_decode_config_host.py.
//   test_decode_config table d H L F C S T V   the compatibility table and the key algebra at these decoder dimensions
//   test_decode_config derived                 nt_loads / key splits at the real model sizes (expected values: the formulas as they
//                                              stood in wt_decoder_begin before they moved into the resolver, worked out by hand below)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>

#include "../../whisper-trtllm_amd/csrc/host_logic.h"

using namespace wt;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checks;                                        \
        if (!(cond)) {                                     \
            ++g_fail;                                      \
            printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

struct Case {
    DecodeRequest r;
    wt_greedy_params p;
    DecodeFacts f;
    int rows = 2, pool = 0;
    bool stream = false;
};

static Case plain(const EngineDims& e) {
    Case c;
    memset(&c.p, 0, sizeof c.p);
    c.p.decoder_start_token_id = e.V - 4; c.p.eos_token_id = e.V - 3; c.p.pad_token_id = e.V - 3;
    c.p.max_length = e.T < 20 ? e.T : 20; c.p.begin_index = 2; c.p.force_eos_step = -1;
    return c;
}
static int resolve(const EngineDims& e, const Case& c, DecodeConfig* out, std::string* msg = nullptr) {
    char err[400] = "";
    DecodeConfig tmp;
    const int rc = resolve_decode_config(e, c.f, c.r, &c.p, c.rows, c.pool, c.stream, out ? out : &tmp, err, sizeof err);
    if (msg) *msg = err;
    return rc;
}

// the six features, as their setters store them
static void ts_on(const EngineDims& e, Case& c) { c.r.ts = wt_timestamp_params{1, e.V - 10, e.V - 9, 2, 1}; }
static void beams_on(const EngineDims&, Case& c) { c.r.beam = wt_beam_params{4, 1.f, 0}; }
static void tt_on(const EngineDims&, Case& c) { c.r.tt.n_sel = 2; c.r.tt.layer[0] = 0; c.r.tt.head[0] = 1; c.r.tt.layer[1] = 1; c.r.tt.head[1] = 0; }
static void lp_on(const EngineDims&, Case& c) { c.r.lp = wt_logprob_params{1, 7}; }
static void samp_on(const EngineDims&, Case& c) { c.r.samp_temp = 0.7f; c.r.samp_seed = 11; }
static void prompt_on(const EngineDims&, Case& c) { c.r.prompt = {5, 6, 7}; c.r.prompt_rows = 1; c.r.prompt_len = 3; }
typedef void (*Feature)(const EngineDims&, Case&);

static float g_trace_buf[1];
static const int32_t g_rows_a[MAX_ROWS] = {3, 4, 5, 6, 3, 4, 5, 6, 3, 4, 5, 6, 3, 4, 5, 6};
static const int32_t g_rows_b[MAX_ROWS] = {9, 8, 7, 6, 9, 8, 7, 6, 9, 8, 7, 6, 9, 8, 7, 6};

static void expect(const EngineDims& e, const Case& c, int code, const char* part, const char* what) {
    std::string msg;
    const int rc = resolve(e, c, nullptr, &msg);
    CHECK(rc == code, "%s: code %d, expected %d (%s)", what, rc, code, msg.c_str());
    if (rc != WT_OK) CHECK(msg.find(part) != std::string::npos, "%s: message '%s' lacks '%s'", what, msg.c_str(), part);
}

static void compatibility_table(const EngineDims& e) {
    const struct { const char* name; Feature on; } feats[] = {{"timestamp rules", ts_on}, {"beams", beams_on}, {"token timestamps", tt_on},
                                                             {"log-probabilities", lp_on}, {"sampling", samp_on}, {"prompt", prompt_on}};
    // ---- batch decodes: every single feature alone, and the allowed pairs
    expect(e, plain(e), WT_OK, "", "plain");
    for (const auto& f : feats) {
        Case c = plain(e);
        f.on(e, c);
        DecodeConfig cfg;
        CHECK(resolve(e, c, &cfg) == WT_OK, "%s alone", f.name);
        CHECK(cfg.key.B == (f.on == beams_on ? 8 : 2) && cfg.U == 2, "%s alone: B %d U %d", f.name, cfg.key.B, cfg.U);
    }
    const Feature pairs[][2] = {{ts_on, lp_on}, {samp_on, ts_on}, {prompt_on, samp_on}, {prompt_on, ts_on}};
    for (const auto& pr : pairs) {
        Case c = plain(e);
        pr[0](e, c); pr[1](e, c);
        expect(e, c, WT_OK, "", "allowed pair");
    }
    {   // sampling runs the log-probability kernels; a stream has nothing of the batch features
        Case c = plain(e);
        samp_on(e, c);
        DecodeConfig cfg;
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.key.lp.enabled == 1 && cfg.key.samp_temp == 0.7f, "sampling -> lp kernels on");
        Case s = plain(e);
        s.stream = true;
        CHECK(resolve(e, s, &cfg) == WT_OK, "plain stream");
        CHECK(cfg.stream && cfg.pool_rows == 8 && cfg.key.B == 2 && !cfg.key.ts.enabled && cfg.key.beam.num_beams == 1 && cfg.key.tt.n_sel == 0 &&
                  !cfg.key.lp.enabled && cfg.key.samp_temp == 0.f && cfg.prompt_len == 0 && !cfg.key.force_rows_on && !cfg.key.logits_trace,
              "a stream decode has every batch-only feature off, and 4 x slots pool rows by default");
    }
    // ---- beams against everything else
    const struct { Feature on; const char* part; } beam_vs[] = {
        {ts_on, "beam search and timestamp mode cannot be combined"}, {tt_on, "beam search and token-level timestamps cannot be combined"},
        {lp_on, "beam search and token log-probabilities cannot be combined"}, {samp_on, "beam search and temperature sampling cannot be combined"},
        {prompt_on, "a decoder prompt and beam search cannot be combined"}};
    for (const auto& b : beam_vs) {
        Case c = plain(e);
        beams_on(e, c); b.on(e, c);
        expect(e, c, WT_E_UNSUPPORTED, b.part, "beams x feature");
    }
    for (int k = 0; k < 3; ++k) {
        Case c = plain(e);
        beams_on(e, c);
        if (k == 0) c.p.logits_trace = g_trace_buf;
        if (k == 1) c.p.force_eos_step = 3;
        if (k == 2) c.p.force_eos_steps = g_rows_a;
        expect(e, c, WT_E_UNSUPPORTED, "logits_trace / force_eos_step(s) are not available with beam search", "beams x trace/force");
    }
    {   // first failure first: beams + timestamps + prompt reports the beam/timestamp pair
        Case c = plain(e);
        beams_on(e, c); ts_on(e, c); prompt_on(e, c);
        expect(e, c, WT_E_UNSUPPORTED, "beam search and timestamp mode", "order of the checks");
    }
    {
        Case c = plain(e);
        beams_on(e, c);
        c.rows = 5;   // 5 x 4 > 16
        expect(e, c, WT_E_UNSUPPORTED, "5 utterances x 4 beams > 16 rows per call", "U * num_beams > MAX_ROWS");
        c.rows = 4;
        expect(e, c, WT_OK, "", "4 x 4 beams");
        Case g = plain(e);
        g.rows = MAX_ROWS + 1;
        expect(e, g, WT_E_UNSUPPORTED, "wt_decoder_begin: batch 17 > 16 per call; shard the batch", "batch > MAX_ROWS");
    }
    // ---- prompts
    {
        Case c = plain(e);
        prompt_on(e, c);
        c.f.w_half = true; c.f.kv_esz = 2;
        expect(e, c, WT_E_UNSUPPORTED, "decoder prompts need an fp32 decoder engine", "prompt on a half engine");
        c = plain(e); prompt_on(e, c); tt_on(e, c);
        expect(e, c, WT_E_UNSUPPORTED, "a decoder prompt and token-level timestamps cannot be combined", "prompt x token timestamps");
        c = plain(e); prompt_on(e, c);
        c.rows = 3; c.r.prompt = {5, 6, 7, 5, 6, 7}; c.r.prompt_rows = 2;
        expect(e, c, WT_E_INVALID, "gave 2 prompt rows for a batch of 3", "prompt rows neither 1 nor >= B");
        c.r.prompt_rows = 3; c.r.prompt.resize(9, 1);
        expect(e, c, WT_OK, "", "prompt rows == B");
        c = plain(e); prompt_on(e, c);
        c.p.max_length = 4;   // 3 + 2 > 4
        expect(e, c, WT_E_INVALID, "3 prompt tokens + the start token + one generated token > max_length 4", "prompt len + 2 > max_length");
        c.p.max_length = 5;
        expect(e, c, WT_OK, "", "prompt len + 2 == max_length");
    }
    // ---- sampling seeds, lengths, token timestamps' steps, forced ids
    {
        Case c = plain(e);
        samp_on(e, c);
        c.r.samp_list = true; c.r.samp_seeds = {1};
        expect(e, c, WT_E_INVALID, "gave 1 seeds for a batch of 2", "seed list shorter than B");
        c.r.samp_seeds = {1, 2};
        expect(e, c, WT_OK, "", "seed list of B");
        for (int ml : {1, e.T + 1}) {
            c = plain(e);
            c.p.max_length = ml;
            expect(e, c, WT_E_INVALID, "outside [2, max_target_positions=", "max_length outside [2, T]");
        }
        for (int ml : {2, e.T}) {
            c = plain(e);
            c.p.max_length = ml;
            expect(e, c, WT_OK, "", "max_length at the ends of [2, T]");
        }
        EngineDims big = e;
        big.T = TT_MAX_TOKENS + 8;
        c = plain(big); tt_on(big, c);
        c.p.max_length = TT_MAX_TOKENS + 2;
        expect(big, c, WT_E_UNSUPPORTED, "token timestamps: 1025 steps > 1024", "steps above TT_MAX_TOKENS");
        c.p.max_length = TT_MAX_TOKENS + 1;
        expect(big, c, WT_OK, "", "TT_MAX_TOKENS steps");
        c = plain(e);
        c.p.decoder_start_token_id = e.V;
        expect(e, c, WT_E_INVALID, "start/eos/pad token id outside the vocabulary", "start token outside the vocabulary");
        const int32_t sup[2] = {3, e.V};
        c = plain(e); c.p.suppress_tokens = sup; c.p.n_suppress_tokens = 2;
        expect(e, c, WT_E_INVALID, "suppress token", "suppress token outside the vocabulary");
        c = plain(e); c.p.begin_suppress_tokens = sup; c.p.n_begin_suppress_tokens = 2;
        expect(e, c, WT_E_INVALID, "begin-suppress token", "begin-suppress token outside the vocabulary");
        const int32_t f_eos[2] = {1, e.V - 3}, f_nots[2] = {1, e.V - 10}, f_late[2] = {1, 9}, f_ok[2] = {0, 9}, f_bad[2] = {1, -1};
        c = plain(e); beams_on(e, c); c.p.forced_decoder_ids = f_eos; c.p.n_forced = 1;
        expect(e, c, WT_E_INVALID, "is the EOS token (no beam could continue)", "forced EOS with beams");
        c = plain(e); c.p.forced_decoder_ids = f_eos; c.p.n_forced = 1;
        expect(e, c, WT_OK, "", "forced EOS without beams");
        c = plain(e); ts_on(e, c); c.p.forced_decoder_ids = f_nots; c.p.n_forced = 1;
        expect(e, c, WT_E_INVALID, "timestamp mode: forced token", "forced <|notimestamps|> in timestamp mode");
        c = plain(e); ts_on(e, c); c.p.forced_decoder_ids = f_late; c.p.n_forced = 1;
        expect(e, c, WT_E_INVALID, "no forced position >= begin_index - 1 = 1", "forced position fights the timestamp rules");
        c = plain(e); ts_on(e, c); c.p.forced_decoder_ids = f_ok; c.p.n_forced = 1;
        expect(e, c, WT_OK, "", "forced id in front of begin_index - 1");
        c = plain(e); c.p.forced_decoder_ids = f_bad; c.p.n_forced = 1;
        expect(e, c, WT_E_INVALID, "forced token -1 outside the vocabulary", "forced token outside the vocabulary");
    }
    // ---- streams
    for (const auto& f : feats) {
        Case c = plain(e);
        c.stream = true;
        f.on(e, c);
        expect(e, c, WT_E_UNSUPPORTED, "a batch-decode feature (wt_decoder_begin)", f.name);
    }
    for (int k = 0; k < 3; ++k) {
        Case c = plain(e);
        c.stream = true;
        if (k == 0) c.p.logits_trace = g_trace_buf;
        if (k == 1) c.p.force_eos_step = 0;
        if (k == 2) c.p.force_eos_steps = g_rows_a;
        expect(e, c, WT_E_UNSUPPORTED, "logits_trace / force_eos_step(s) belong to wt_decoder_begin", "stream x trace/force");
    }
    {
        Case c = plain(e);
        c.stream = true;
        c.pool = 2;   // < slots + 1
        expect(e, c, WT_E_INVALID, "pool of 2 rows outside [slots + 1, 256]", "pool below slots + 1");
        c.pool = STREAM_QCAP + 1;
        expect(e, c, WT_E_INVALID, "pool of 257 rows outside [slots + 1, 256]", "pool above STREAM_QCAP");
        c.pool = 3;
        expect(e, c, WT_OK, "", "pool of slots + 1");
        c.pool = STREAM_QCAP;
        expect(e, c, WT_OK, "", "pool of STREAM_QCAP");
        ts_on(e, c); c.pool = 2;   // the pool bounds come first
        expect(e, c, WT_E_INVALID, "pool of 2 rows", "order of the stream's checks");
        c = plain(e); c.stream = true; c.rows = MAX_ROWS + 1;
        expect(e, c, WT_E_UNSUPPORTED, "wt_decoder_stream_begin: batch 17 > 16 per call", "slots > MAX_ROWS");
    }
}

static StepKey key_of(const EngineDims& e, const Case& c) {
    DecodeConfig cfg;
    std::string msg;
    const int rc = resolve(e, c, &cfg, &msg);
    CHECK(rc == WT_OK, "key_of: %d %s", rc, msg.c_str());
    return cfg.key;
}

static void key_algebra(const EngineDims& e) {
    typedef std::function<void(Case&)> Edit;
    auto differs = [&](const char* what, const Edit& base, const Edit& edit) {
        Case a = plain(e), b = plain(e);
        base(a); base(b); edit(b);
        const StepKey ka = key_of(e, a), ka2 = key_of(e, a), kb = key_of(e, b);
        CHECK(memcmp(&ka, &ka2, sizeof ka) == 0, "%s: the same inputs twice give byte-equal keys", what);
        CHECK(memcmp(&ka, &kb, sizeof ka) != 0 && ka != kb, "%s must change the key", what);
    };
    auto same = [&](const char* what, const Edit& base, const Edit& edit) {
        Case a = plain(e), b = plain(e);
        base(a); base(b); edit(b);
        const StepKey ka = key_of(e, a), kb = key_of(e, b);
        CHECK(memcmp(&ka, &kb, sizeof ka) == 0 && ka == kb, "%s must leave the key byte-equal", what);
    };
    const Edit none = [](Case&) {};
    const Edit ts = [&](Case& c) { ts_on(e, c); }, beams = [&](Case& c) { beams_on(e, c); }, tt = [&](Case& c) { tt_on(e, c); };
    const Edit lp = [&](Case& c) { lp_on(e, c); }, samp = [&](Case& c) { samp_on(e, c); }, prompt = [&](Case& c) { prompt_on(e, c); };
    // ---- what a captured step graph carries
    differs("B", none, [](Case& c) { c.rows = 3; });
    differs("max_length", none, [](Case& c) { c.p.max_length -= 1; });
    differs("begin_index", none, [](Case& c) { c.p.begin_index = 3; });
    differs("eos", none, [](Case& c) { c.p.eos_token_id -= 1; });
    differs("pad", none, [](Case& c) { c.p.pad_token_id -= 1; });
    differs("start_token", none, [](Case& c) { c.p.decoder_start_token_id -= 1; });
    differs("force_eos_step", none, [](Case& c) { c.p.force_eos_step = 4; });
    differs("logits_trace", none, [](Case& c) { c.p.logits_trace = g_trace_buf; });
    differs("force_rows_on", none, [](Case& c) { c.p.force_eos_steps = g_rows_a; });
    differs("timestamp rules on", none, ts);
    differs("ts.no_timestamps_token_id", ts, [](Case& c) { c.r.ts.no_timestamps_token_id -= 1; });
    differs("ts.timestamp_begin", ts, [](Case& c) { c.r.ts.timestamp_begin += 1; });
    differs("ts.begin_index", ts, [](Case& c) { c.r.ts.begin_index = 3; });
    differs("ts.max_initial_timestamp_index", ts, [](Case& c) { c.r.ts.max_initial_timestamp_index = -1; });
    differs("beams on", none, beams);
    differs("beam.num_beams", beams, [](Case& c) { c.r.beam.num_beams = 2; });
    differs("beam.length_penalty", beams, [](Case& c) { c.r.beam.length_penalty = 2.f; });
    differs("beam.early_stopping", beams, [](Case& c) { c.r.beam.early_stopping = 1; });
    differs("beam_group", beams, [](Case& c) { c.f.beam_cross_grouped = true; });
    differs("lp.enabled", none, lp);
    differs("lp.no_speech_token_id", lp, [](Case& c) { c.r.lp.no_speech_token_id = -1; });
    differs("sampling on", none, samp);
    differs("sampling temperature", samp, [](Case& c) { c.r.samp_temp = 0.9f; });
    differs("token timestamps on", none, tt);
    differs("token timestamps: head count", tt, [](Case& c) { c.r.tt.n_sel = 1; });
    differs("token timestamps: a layer", tt, [](Case& c) { c.r.tt.layer[1] = 0; c.r.tt.head[1] = 0; });
    differs("token timestamps: a head", tt, [](Case& c) { c.r.tt.head[0] = 0; });
    differs("tt_rows", tt, [](Case& c) { c.rows = 3; });
    differs("tt_steps", tt, [](Case& c) { c.p.max_length -= 1; });
    differs("nsplit_self", none, [](Case& c) { c.f.nsplit_self = 2; });
    differs("nsplit_cross", none, [](Case& c) { c.f.nsplit_cross_set = true; c.f.nsplit_cross = 3; });
    {   // nt_loads at whisper-tiny.en's size: batch 8 of an fp32 engine streams (304 MB per step), the fp16 engine's 152 MB do not
        EngineDims t;
        t.kind = WT_KIND_DECODER; t.d = 384; t.H = 6; t.L = 4; t.F = 1536; t.C = 80; t.S = 1500; t.T = 448; t.V = 51864;
        Case a = plain(t), b = plain(t);
        a.rows = b.rows = 8; a.p.max_length = b.p.max_length = 448;
        b.f.w_half = true; b.f.kv_esz = 2;
        const StepKey ka = key_of(t, a), kb = key_of(t, b);
        CHECK(ka.nt_loads == 1 && kb.nt_loads == 0 && ka != kb, "nt_loads must change the key (%d, %d)", ka.nt_loads, kb.nt_loads);
    }
    {   // the workspace generation is the engine's to fill
        StepKey a = key_of(e, plain(e)), b = a;
        b.workspace_gen += 1;
        CHECK(a != b, "workspace_gen must change the key");
    }
    CHECK(key_of(e, [&] { Case c = plain(e); beams_on(e, c); c.f.nsplit_self = 2; return c; }()).nsplit_self == 1, "beams force nsplit_self = 1");
    CHECK(key_of(e, [&] { Case c = plain(e); c.f.nsplit_self = 2; c.f.no_defer_merge = true; return c; }()).nsplit_self == 1, "no deferred merge: unsplit");
    // ---- what no captured launch carries
    static const int32_t sup_a[2] = {1, 2}, sup_b[3] = {3, 4, 5}, forced_a[2] = {1, 9}, forced_b[4] = {1, 11, 2, 12};
    same("suppress table contents", [](Case& c) { c.p.suppress_tokens = sup_a; c.p.n_suppress_tokens = 2; },
         [](Case& c) { c.p.suppress_tokens = sup_b; c.p.n_suppress_tokens = 3; });
    same("begin-suppress table contents", none, [](Case& c) { c.p.begin_suppress_tokens = sup_b; c.p.n_begin_suppress_tokens = 3; });
    same("forced table contents", [](Case& c) { c.p.forced_decoder_ids = forced_a; c.p.n_forced = 1; },
         [](Case& c) { c.p.forced_decoder_ids = forced_b; c.p.n_forced = 2; });
    same("per-row forced lengths", [](Case& c) { c.p.force_eos_steps = g_rows_a; }, [](Case& c) { c.p.force_eos_steps = g_rows_b; });
    same("seed", samp, [](Case& c) { c.r.samp_seed = 12345; });
    same("seed list", samp, [](Case& c) { c.r.samp_list = true; c.r.samp_seeds = {7, 8}; });
    same("prompt on", none, prompt);
    same("prompt ids", prompt, [](Case& c) { c.r.prompt = {9, 9, 9}; });
    same("prompt length", prompt, [](Case& c) { c.r.prompt = {9, 9, 9, 9}; c.r.prompt_len = 4; });
    same("prompt rows", prompt, [](Case& c) { c.r.prompt = {5, 6, 7, 5, 6, 7}; c.r.prompt_rows = 2; });
    same("token timestamps: median width", tt, [](Case& c) { c.r.tt.width = 5; });
    same("token timestamps: time precision", tt, [](Case& c) { c.r.tt.time_precision = 0.04; });
    same("a stream against the batch decode of as many rows", none, [](Case& c) { c.stream = true; });   // (their graphs are separate variants)
}

// nt_loads = (weights + K/V bytes of one step) > 160e6 with p_step = L (6 d^2 + 2 d F) + V d parameters and
// B * 2 L H (S + max_length) * 64 cache elements; cross splits n = ceil(256 / (B H)) -> 4 if n >= 4, 2 if n >= 2, else 1 (S = 1500 keys
// never halves it).  By hand, fp32, max_length 448:
//   tiny.en   p_step 28 173 312 -> 112.7 MB; K/V 23.9 MB per row: B = 1 136.6 MB -> 0, B = 8 304.2 MB -> 1;  B H = 6, 48 -> 4, 4
//   base.en   p_step 48 574 464 -> 194.3 MB -> 1;  B H = 64 -> ceil(256 / 64) = 4 -> 4
//   medium.en weights alone 1.4 GB -> 1;  B H = 16, 32, 64, 128 -> n = 16, 8, 4, 2 -> 4, 4, 4, 2
//   tiny.en fp16 engine (2-byte weights and caches), B = 8: 56.3 + 95.7 = 152.1 MB -> 0
static void derived_values() {
    struct Row { const char* name; int d, H, L, F, B; bool half; int nt, ns_cross; };
    const Row rows[] = {{"tiny.en", 384, 6, 4, 1536, 1, false, 0, 4},     {"tiny.en", 384, 6, 4, 1536, 8, false, 1, 4},
                        {"base.en", 512, 8, 6, 2048, 8, false, 1, 4},     {"medium.en", 1024, 16, 24, 4096, 1, false, 1, 4},
                        {"medium.en", 1024, 16, 24, 4096, 2, false, 1, 4}, {"medium.en", 1024, 16, 24, 4096, 4, false, 1, 4},
                        {"medium.en", 1024, 16, 24, 4096, 8, false, 1, 2}, {"tiny.en fp16", 384, 6, 4, 1536, 8, true, 0, 4}};
    for (const Row& r : rows) {
        EngineDims e;
        e.kind = WT_KIND_DECODER; e.d = r.d; e.H = r.H; e.L = r.L; e.F = r.F; e.C = 80; e.S = 1500; e.T = 448; e.V = 51864;
        Case c = plain(e);
        c.rows = r.B; c.p.max_length = 448;
        if (r.half) { c.f.w_half = true; c.f.kv_esz = 2; }
        const StepKey k = key_of(e, c);
        CHECK(k.nt_loads == r.nt && k.nsplit_cross == r.ns_cross && k.nsplit_self == 1 && k.beam_group == 0,
              "%s B=%d: nt_loads %d (want %d), nsplit_cross %d (want %d), nsplit_self %d", r.name, r.B, k.nt_loads, r.nt, k.nsplit_cross, r.ns_cross,
              k.nsplit_self);
        CHECK(pick_splits(r.B, r.H, 1500) == r.ns_cross, "%s B=%d: pick_splits", r.name, r.B);
    }
    CHECK(pick_splits(1, 2, 96) == 2 && pick_splits(1, 2, 95) == 1 && pick_splits(16, 16, 1500) == 1, "pick_splits: short memories halve, 256 pairs: none");
    {   // a beam decode: unsplit self attention; the grouped cross form counts blocks per utterance
        EngineDims e;
        e.kind = WT_KIND_DECODER; e.d = 1024; e.H = 16; e.L = 24; e.F = 4096; e.C = 80; e.S = 1500; e.T = 448; e.V = 51864;
        Case c = plain(e);
        c.rows = 2; c.p.max_length = 448; c.r.beam = wt_beam_params{4, 1.f, 0}; c.f.nsplit_self = 2;
        StepKey k = key_of(e, c);
        CHECK(k.B == 8 && k.nsplit_self == 1 && k.beam_group == 0 && k.nsplit_cross == 2, "4 beams x 2: B %d self %d group %d cross %d", k.B, k.nsplit_self,
              k.beam_group, k.nsplit_cross);
        c.f.beam_cross_grouped = true;
        k = key_of(e, c);
        CHECK(k.beam_group == 4 && k.nsplit_cross == 4, "grouped: group %d cross %d", k.beam_group, k.nsplit_cross);
        c.r.beam.num_beams = 3;
        CHECK(key_of(e, c).beam_group == 0, "grouped form: num_beams 2 and 4 only");
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "derived")) {
        derived_values();
    } else if (argc == 10 && !strcmp(argv[1], "table")) {
        EngineDims e;
        e.kind = WT_KIND_DECODER; e.precision = WT_F32;
        e.d = atoi(argv[2]); e.H = atoi(argv[3]); e.L = atoi(argv[4]); e.F = atoi(argv[5]); e.C = atoi(argv[6]); e.S = atoi(argv[7]);
        e.T = atoi(argv[8]); e.V = atoi(argv[9]);
        compatibility_table(e);
        key_algebra(e);
    } else {
        fprintf(stderr, "usage: %s table d H L F C S T V | derived\n", argv[0]);
        return 2;
    }
    printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
