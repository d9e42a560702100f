// CPU test of the language tables' validation (csrc/host_logic.cpp: resolve_decode_config with DecodeRequest.lang_ids / lang_rows).
// Stand-alone: links host_logic.cpp only, built with g++ -fsanitize=address,undefined by tests/test_language_host.py.
//   test_language_config d H L F C S T V
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    int rows = 3;
    bool stream = false;
};

static Case plain(const EngineDims& e) {
    Case c;
    memset(&c.p, 0, sizeof c.p);
    c.p.decoder_start_token_id = e.V - 4; c.p.eos_token_id = e.V - 3; c.p.pad_token_id = e.V - 3;
    c.p.max_length = e.T < 20 ? e.T : 20; c.p.begin_index = 4; c.p.force_eos_step = -1;
    return c;
}
static Case langs(const EngineDims& e) {
    Case c = plain(e);
    c.r.lang_ids = {40, 3, 0, e.V - 1, 17};
    return c;
}
static int resolve(const EngineDims& e, const Case& c, DecodeConfig* out, std::string* msg = nullptr) {
    char err[400] = "";
    DecodeConfig tmp;
    const int rc = resolve_decode_config(e, c.f, c.r, &c.p, c.rows, 0, c.stream, out ? out : &tmp, err, sizeof err);
    if (msg) *msg = err;
    return rc;
}
static void expect(const EngineDims& e, const Case& c, int code, const char* part, const char* what) {
    std::string msg;
    const int rc = resolve(e, c, nullptr, &msg);
    CHECK(rc == code, "%s: code %d, expected %d (%s)", what, rc, code, msg.c_str());
    if (rc != WT_OK) CHECK(msg.find(part) != std::string::npos, "%s: message '%s' lacks '%s'", what, msg.c_str(), part);
}

int main(int argc, char** argv) {
    if (argc != 9) {
        printf("usage: test_language_config d H L F C S T V\n");
        return 2;
    }
    EngineDims e;
    e.kind = 2;
    e.d = atoi(argv[1]); e.H = atoi(argv[2]); e.L = atoi(argv[3]); e.F = atoi(argv[4]); e.C = atoi(argv[5]); e.S = atoi(argv[6]);
    e.T = atoi(argv[7]); e.V = atoi(argv[8]);

    {   // off: the key says so, and equals the key of a request that never mentioned languages
        DecodeConfig a, b;
        Case c = plain(e);
        CHECK(resolve(e, c, &a) == WT_OK && a.key.lang_pos == -1 && a.key.n_lang == 0 && a.lang_detect == 0, "mode off: lang_pos %d n_lang %d", a.key.lang_pos, a.key.n_lang);
        c.r.lang_rows = {1, 2, 3};   // a row table without ids is no request
        CHECK(resolve(e, c, &b) == WT_OK && a.key == b.key, "a row table without ids leaves the key alone");
    }
    {   // detect every row
        DecodeConfig cfg;
        Case c = langs(e);
        CHECK(resolve(e, c, &cfg) == WT_OK, "detect every row");
        CHECK(cfg.key.lang_pos == 1 && cfg.key.n_lang == 5 && cfg.lang_detect == 1, "lang_pos %d n_lang %d detect %d", cfg.key.lang_pos, cfg.key.n_lang, cfg.lang_detect);
        for (int b = 0; b < 3; ++b) CHECK(cfg.lang_rows[b] == -1, "row %d: %d", b, cfg.lang_rows[b]);
        for (int i = 0; i < 5; ++i) CHECK(cfg.lang_ids[i] == c.r.lang_ids[i], "id %d kept in the caller's order", i);
        DecodeConfig off;
        Case p = plain(e);
        CHECK(resolve(e, p, &off) == WT_OK && off.key != cfg.key, "the mode is part of the step key");
    }
    {   // rows chosen by the caller: mixed, and all chosen (no detection kernel); any negative entry means detect
        DecodeConfig cfg;
        Case c = langs(e);
        c.r.lang_rows = {17, -5, 0, 999999};   // a fourth entry beyond the batch is not looked at
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.lang_detect == 1 && cfg.lang_rows[0] == 17 && cfg.lang_rows[1] == -1 && cfg.lang_rows[2] == 0,
              "mixed rows: %d %d %d", cfg.lang_rows[0], cfg.lang_rows[1], cfg.lang_rows[2]);
        c.r.lang_rows = {17, e.V - 1, 0};
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.lang_detect == 0 && cfg.key.n_lang == 5 && cfg.key.lang_pos == 1, "all rows chosen: no detection");
        DecodeConfig det;
        c.r.lang_rows.clear();
        CHECK(resolve(e, c, &det) == WT_OK && det.key == cfg.key, "the rows' contents are a device table, not part of the key");
    }
    {   // lang_pos behind prompts: the longest row's length + 1, also for ragged rows
        DecodeConfig cfg;
        Case c = langs(e);
        c.r.prompt = {5, 6, 7}; c.r.prompt_rows = 1; c.r.prompt_len = 3; c.p.begin_index = 7;
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.key.lang_pos == 4, "shared prompt of 3: lang_pos %d", cfg.key.lang_pos);
        c.r.prompt = {5, 6, 7, 8, 9, 0, 0, 0, 0, 0, 5, 6, 0, 0, 0}; c.r.prompt_rows = 3; c.r.prompt_len = 5; c.r.prompt_lens = {5, 0, 2};
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.key.lang_pos == 6 && cfg.prompt_ragged == 1, "ragged prompts 5 / 0 / 2: lang_pos %d", cfg.key.lang_pos);
        c.p.max_length = 7;
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.key.lang_pos == 6, "the language position is the last one of max_length 7");
        c.f.w_half = true;
        expect(e, c, WT_E_UNSUPPORTED, "fp32 decoder engine", "prompts stay refused on an fp16 engine");
        Case h = langs(e);
        h.f.w_half = true; h.f.kv_esz = 2;
        expect(e, h, WT_OK, "", "languages alone on an fp16 engine");
    }
    {   // the id list
        Case c = langs(e);
        c.r.lang_ids.push_back(e.V);
        expect(e, c, WT_E_INVALID, "outside the vocabulary", "id V");
        c.r.lang_ids.back() = -1;
        expect(e, c, WT_E_INVALID, "outside the vocabulary", "id -1");
        c.r.lang_ids.back() = 40;
        expect(e, c, WT_E_INVALID, "listed twice", "a repeated id");
        c.r.lang_ids.back() = c.p.eos_token_id;
        expect(e, c, WT_E_INVALID, "EOS", "the EOS id");
        Case many = plain(e);
        for (int i = 0; i < LANG_MAX; ++i) many.r.lang_ids.push_back(i);
        expect(e, many, WT_OK, "", "128 ids");
        many.r.lang_ids.push_back(LANG_MAX);
        expect(e, many, WT_E_INVALID, "language ids >", "129 ids");
        Case one = plain(e);
        one.r.lang_ids = {9};
        expect(e, one, WT_OK, "", "one id");
    }
    {   // the row table
        Case c = langs(e);
        c.r.lang_rows = {17, 41, 0};
        expect(e, c, WT_E_INVALID, "not one of the listed ids", "a row entry that is not listed");
        c.r.lang_rows = {17, 3};
        expect(e, c, WT_E_INVALID, "row entries for a batch of 3", "too few rows");
        c.rows = 2;
        expect(e, c, WT_OK, "", "two rows for a batch of two");
    }
    {   // refused combinations, the families the prompt feature refuses
        Case c = langs(e);
        c.r.beam = wt_beam_params{4, 1.f, 0};
        expect(e, c, WT_E_UNSUPPORTED, "language tokens and beam search", "beams");
        c = langs(e);
        c.r.tt.n_sel = 1;
        expect(e, c, WT_E_UNSUPPORTED, "language tokens and token-level timestamps", "token-level timestamps");
        c = langs(e);
        c.stream = true;
        expect(e, c, WT_E_UNSUPPORTED, "batch-decode feature", "the continuous mode");
        // allowed: timestamp mode (language position in front of begin_index - 1), log-probabilities, sampling
        c = langs(e);
        c.r.ts = wt_timestamp_params{1, e.V - 10, e.V - 9, 4, 1};
        c.r.lp = wt_logprob_params{1, 7};
        c.r.samp_temp = 0.5f;
        DecodeConfig cfg;
        CHECK(resolve(e, c, &cfg) == WT_OK && cfg.key.ts.enabled && cfg.key.lang_pos == 1, "timestamps + log-probabilities + sampling + languages");
        c.r.ts.begin_index = 2;   // the .en layout: <|0.00|> is forced at position 1, where the language would go
        expect(e, c, WT_E_INVALID, "language position", "timestamp rules without room for a language token");
    }
    printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
