// C-ABI of the MI355X Whisper engine (include/whisper_trtllm_amd.h): blob parsing, weight upload, workspace,
// encoder forward, the Session-compatible by-value decoder step, and the resident-KV greedy fast path with
// hipGraph replay.  Reference call sites replaced: tensorrt_llm/runtime/session.py:54-178 (Session) and
// examples/whisper/run.py:57-227 (engine wrappers + greedy_search).
#include "../../include/whisper_trtllm_amd.h"
#include "wt_common.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace wt;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
int wt_set_error(int code, const char* fmt, ...) {  // shared with frontend.hip
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return fail(WT_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                            \
    } while (0)

struct DevTensor {
    float* ptr = nullptr;
    int dtype = WT_F32;
    int ndim = 0;
    int64_t shape[4] = {0, 0, 0, 0};
};

struct EncLayerW {
    const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *o_w, *o_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    const void *qkv_w3 = nullptr, *o_w3 = nullptr, *fc1_w3 = nullptr, *fc2_w3 = nullptr;   // the same matrices as three bf16 planes (launch_gemm_x3)
};
struct DecLayerW {
    const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *o_w, *o_b;
    const float *fold_w, *fold_c, *fold_r, *fold_t;  // folded LN + cross-attention query (builder.py:_pack_decoder)
    const float *ckv_w, *ckv_b, *co_w, *co_b;
    const float *ln3_w, *ln3_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    const void* ckv_w3 = nullptr;   // cross k|v weights as three bf16 planes (launch_gemm_x3)
    // d <= 1024: columns [0, d) / [d, 2d) of fold_w as two contiguous [d][d] matrices in the engine's weight precision (build_fold_halves)
    const void *fold_wa = nullptr, *fold_wh = nullptr;
};

struct EvTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double ms = 0.0;
    long long launches = 0;
};

// The weight payload of an engine in device memory: ONE allocation, read-only after wt_engine_open, shared (reference-counted) by the
// handles wt_engine_clone makes from it -- N workers per GPU (runtime.WhisperPipeline) hold one copy of the weights and N workspaces.
struct WeightStore {
    char* base = nullptr;
    char* x3 = nullptr;    // fp32 engines: the big GEMMs' weights once more as three bf16 planes each (launch_gemm_x3), shared like `base`
    char* fold = nullptr;  // decoder engines, d <= 1024: the two halves of every layer's fold_w (build_fold_halves), shared like `base`
    int device = 0;
    ~WeightStore() {
        if (!base && !x3 && !fold) return;
        DeviceGuard guard(device);
        if (base) hipFree(base);
        if (x3) hipFree(x3);
        if (fold) hipFree(fold);
    }
};

struct wt_engine {
    const void *conv1_w3 = nullptr, *conv2_w3 = nullptr;   // conv weights as three bf16 planes (launch_gemm_x3)
    void *melT3 = nullptr, *c1_3 = nullptr;                 // x3: the convs' A operands as three bf16 planes (time-major, zero pad rows)
    size_t melT3_plane = 0, c1_3_plane = 0;                 // their plane strides: fixed by the workspace CAPACITY, so that a smaller batch finds
                                                            // utterance b's rows -- and the zero padding rows nobody ever writes -- where a larger one left them
    int kind = 0, device = 0, precision = WT_F32;
    int d = 0, H = 0, L = 0, F = 0, C = 0, S = 0, T = 0, V = 0;
    std::shared_ptr<WeightStore> weights;
    char* weights_base = nullptr;   // == weights->base
    std::map<std::string, DevTensor> w;
    // encoder
    std::vector<EncLayerW> enc_layers;
    const float *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr, *enc_pos = nullptr,
                *enc_ln_w = nullptr, *enc_ln_b = nullptr;
    int enc_cap = 0;
    char* enc_ws = nullptr;
    float *melT = nullptr, *c1 = nullptr, *hbuf = nullptr, *xbuf = nullptr, *qkv = nullptr, *ctx = nullptr, *ffn = nullptr;
    bool use_x3 = false;          // fp32 engine: the layer GEMMs / the cross-K/V projection run launch_gemm_x3 (fp32 product from bf16 MFMAs)
    void *xs3 = nullptr, *ctx3 = nullptr, *ffn3 = nullptr, *qkv3 = nullptr;   // x3 activations: three bf16 planes of [M][d] / [M][d] / [M][F] / [M][3d]
    void* enc3 = nullptr;         // decoder: three bf16 planes of the encoder memory in front of the cross-K/V projection
    void *melT_h = nullptr, *c1_h = nullptr, *x_h = nullptr, *ctx_h = nullptr, *ffn_h = nullptr;  // fp16 engines
    // decoder
    std::vector<DecLayerW> dec_layers;
    const float *tok_emb = nullptr, *pos_emb = nullptr, *proj_w = nullptr, *dec_ln_w = nullptr, *dec_ln_b = nullptr;
    int dec_cap = 0, dec_maxlen_cap = 0;
    char* dec_ws = nullptr;
    float *self_k = nullptr, *self_v = nullptr, *cross_k = nullptr, *cross_v = nullptr;  // resident caches: fp32, or IEEE half in fp16 engines
    bool w_half = false;   // fp16 decoder engine: every GEMV weight matrix (incl. the tied vocabulary / token table) is IEEE half
    int kv_esz = 4;        // bytes per element of the RESIDENT caches (2 in fp16 engines; Session-path caches are the caller's f32)
    void* enc_h = nullptr; // fp16 engines: half copy of the encoder memory [B][S][d], the A operand of the cross-K/V projection
    float *dh = nullptr, *dh2 = nullptr, *dq = nullptr, *datt = nullptr, *dffn = nullptr, *part = nullptr, *logits = nullptr;
    float* duh = nullptr;   // [B][d] residual half of the folded cross-attention query, q|k|v launch -> pair launch (enqueue_layer_part)
    int* att_cnt = nullptr;
    float* sel_val = nullptr;
    int* sel_idx = nullptr;
    DecState* st = nullptr;
    int *ids = nullptr, *unfinished = nullptr, *forced = nullptr;
    uint8_t* mask = nullptr;
    std::vector<uint8_t> h_mask;   // host images of the device rule tables (wt_decoder_begin uploads only on change)
    std::vector<int> h_forced;
    bool tables_valid = false;
    DecState* h_state = nullptr;  // pinned
    unsigned long long* mailbox = nullptr;      // pinned, coherent host word greedy_finish_kernel reports every step into (wt_decoder_run)
    unsigned long long* mailbox_dev = nullptr;  // its device address
    int epoch = 0;                // wt_decoder_begin count (tags the mailbox word: late no-op steps of the previous decode are ignored)
    int issued = 0;               // decoder steps enqueued since wt_decoder_begin
    // continuous mode (wt_decoder_stream_*): the cross caches are a POOL of rows, `B` decode slots take utterances from a device queue
    int cross_rows = 0;           // rows per layer of the resident cross caches (>= dec_cap; the pool of the continuous mode)
    int* h_ids = nullptr;         // pinned, coherent [h_pool_cap][h_ml_cap]: ids of the utterance in pool row r (written by stream_finish_kernel)
    int* h_len = nullptr;         // pinned, coherent [h_pool_cap]: its final length, 0 = still waiting / decoding
    int *h_ids_dev = nullptr, *h_len_dev = nullptr;
    int h_pool_cap = 0, h_ml_cap = 0;
    std::vector<char> pool_state; // host allocator of pool rows: 0 free, 1 submitted (waiting or decoding), 2 finished but not collected
    int submitted = 0, finished_seen = 0, admitted_seen = 0;
    int* force_rows = nullptr;    // device [16]: per-row forced-EOS steps (bench-only variable-length workload)
    std::vector<int> h_force_rows;
    // greedy session: what the wt_decoder_set_* calls asked for (resolved by the next wt_decoder_begin / wt_decoder_stream_begin) and the
    // configuration of the decode in flight (host_logic.h; valid while `begun`)
    bool begun = false;
    DecodeRequest req;
    DecodeConfig cfg = {};
    unsigned ws_gen = 1;          // bumped whenever device or pinned memory the step graphs point into moves (StepKey.workspace_gen)
    TsPart* ts_part = nullptr;    // timestamp mode: scratch [dec_cap][SELECT_CHUNKS] of ts_select_kernel
    // log-probability mode: the partial pairs of the step and the three result buffers
    float4* lp_part = nullptr;    // [dec_cap][SEL_PARTS_CAP]
    float *lp_side = nullptr, *lp_tok = nullptr, *lp_sum = nullptr, *lp_nsp = nullptr;   // [dec_cap][2], [dec_cap][cap_len], [dec_cap], [dec_cap]
    // temperature sampling (the sampling kernels are forms of the log-probability mode's, so a sampled decode runs with that mode on)
    std::vector<unsigned long long> h_seeds;    // host image of samp_seeds when the request gave one seed (seed + row)
    unsigned long long* samp_seeds = nullptr;   // [dec_cap]
    float* samp_sc = nullptr;                   // [dec_cap][SEL_PARTS_CAP]
    float4* samp_ts = nullptr;                  // [dec_cap][SELECT_CHUNKS]
    BeamParams beam_dev = {};     // beam search: device buffers of the beam state (dec_reserve; nb / U / penalty filled per decode)
    // token-level timestamps: the query history the cross-attention launches fill, and the post-pass workspace
    char* tt_buf = nullptr;       // one allocation: q_hist, the per-layer head tables, W, statistics, matrix, trace, output
    size_t tt_bytes = 0;
    float *tt_qh = nullptr, *tt_W = nullptr, *tt_mean = nullptr, *tt_sdev = nullptr, *tt_matrix = nullptr, *tt_out = nullptr;
    int* tt_sel = nullptr;        // device [L][H]: selection index of (layer, head), or -1
    uint8_t* tt_trace = nullptr;
    std::vector<int> tt_h_sel;    // host image of tt_sel
    // per-row language tokens (wt_decoder_set_languages): one device table, the rows' tokens [MAX_ROWS] in front of the listed ids [LANG_MAX]
    int *lang_tok = nullptr, *lang_ids = nullptr;
    float* lang_prob = nullptr;   // [MAX_ROWS][LANG_MAX] (rows of n_lang entries): lang_select_kernel's softmax over the listed ids
    std::vector<int> h_lang;      // host image of that table for the decode in flight (source of an async copy)
    std::vector<int> h_prompt;    // ragged decoder prompt: the right-padded id matrix + lengths of the decode in flight (source of an async copy)
    char* pf_ws = nullptr;        // decoder prompt: the prefill's workspace (allocated by the first prompt decode, grown when needed)
    size_t pf_bytes = 0;
    hipStream_t own_stream = nullptr;
    // step graphs: [0] every row attends (the only one a decode without early finishers ever replays), [1] finished rows stream no K/V,
    // [2] / [3] the same two for the continuous mode (per-slot cross-cache rows, stream_finish_kernel), [4] / [5] the first step of a
    // decode that detects languages ([0] / [1] with lang_select_kernel in front of the finish; [6] / [7] unused)
    static constexpr int N_GRAPHS = 8;
    hipGraph_t graph[N_GRAPHS] = {};
    hipGraphExec_t graph_exec[N_GRAPHS] = {};
    bool graph_ok[N_GRAPHS] = {};
    StepKey graph_key = {};       // the key the graphs were captured under (B == 0: none yet); enqueue_steps drops them when cfg.key differs
    int graph_captures = 0;       // step-graph captures of this handle so far (wt_dbg_step_graph_captures)
    bool use_graph = true;
    // Session-compat shapes (set by infer_shapes)
    bool shapes_ok = false;
    int c_B = 1, c_s = 0, c_ms = 0, c_mc = 0;
    // profiling
    bool profiling = false;
    EvTimer t_cross, t_gemm, t_enc_attn, t_skinny;
};

// ------------------------------------------------------------------------------------------------- helpers
static void timer_begin(wt_engine* e, EvTimer& t, hipStream_t s, hipEvent_t* a, hipEvent_t* b) {
    *a = *b = nullptr;
    if (!e->profiling) return;
    if (t.pool.empty()) {
        hipEvent_t x, y;
        if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return;
        t.pool.push_back({x, y});
    }
    auto pr = t.pool.back();
    t.pool.pop_back();
    *a = pr.first;
    *b = pr.second;
    hipEventRecord(*a, s);
}
static void timer_end(wt_engine* e, EvTimer& t, hipStream_t s, hipEvent_t a, hipEvent_t b) {
    if (!a) return;
    hipEventRecord(b, s);
    t.pending.push_back({a, b});
}
static void timer_collect(EvTimer& t) {
    for (auto& pr : t.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            t.ms += ms;
            t.launches += 1;
        }
        t.pool.push_back(pr);
    }
    t.pending.clear();
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
constexpr int SEL_PARTS_CAP = 4096;  // partial (max, argmax) slots per batch row: >= workgroups of the vocabulary GEMV

// ------------------------------------------------------------------------------------------------- open / close
extern "C" int wt_abi_version(void) { return WT_ABI_VERSION; }
extern "C" const char* wt_last_error(void) { return g_err; }

extern "C" void wt_engine_close(wt_engine* e) {
    if (!e) return;
    DeviceGuard guard(e->device);
    for (int v = 0; v < wt_engine::N_GRAPHS; ++v) {
        if (e->graph_exec[v]) hipGraphExecDestroy(e->graph_exec[v]);
        if (e->graph[v]) hipGraphDestroy(e->graph[v]);
    }
    for (EvTimer* t : {&e->t_cross, &e->t_gemm, &e->t_enc_attn, &e->t_skinny}) {
        timer_collect(*t);
        for (auto& pr : t->pool) {
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
    }
    if (e->own_stream) hipStreamDestroy(e->own_stream);
    if (e->h_state) hipHostFree(e->h_state);
    if (e->mailbox) hipHostFree((void*)e->mailbox);
    if (e->h_ids) hipHostFree(e->h_ids);
    if (e->h_len) hipHostFree(e->h_len);
    if (e->enc_ws) hipFree(e->enc_ws);
    if (e->dec_ws) hipFree(e->dec_ws);
    if (e->tt_buf) hipFree(e->tt_buf);
    if (e->pf_ws) hipFree(e->pf_ws);
    e->weights.reset();   // the last handle sharing the payload frees it
    delete e;
}

// Split the weight matrices of the big GEMMs into three bf16 planes each (one extra allocation, shared by clones like the payload).
static int build_x3_weights(wt_engine* e) {
    const size_t d = e->d, F = e->F;
    struct Job { const float* src; size_t n; const void** dst; };
    std::vector<Job> jobs;
    if (e->kind == WT_KIND_ENCODER && (e->C % 8) == 0 && ((3 * e->C) % 16) == 0) {
        jobs.push_back({e->conv1_w, d * 3 * (size_t)e->C, &e->conv1_w3});
        jobs.push_back({e->conv2_w, d * 3 * d, &e->conv2_w3});
    }
    if (e->kind == WT_KIND_ENCODER)
        for (EncLayerW& l : e->enc_layers) {
            jobs.push_back({l.qkv_w, 3 * d * d, &l.qkv_w3}); jobs.push_back({l.o_w, d * d, &l.o_w3});
            jobs.push_back({l.fc1_w, F * d, &l.fc1_w3}); jobs.push_back({l.fc2_w, d * F, &l.fc2_w3});
        }
    else
        for (DecLayerW& l : e->dec_layers) jobs.push_back({l.ckv_w, 2 * d * d, &l.ckv_w3});
    size_t total = 0;
    for (const Job& j : jobs) total += align_up(j.n * 6, 256);
    if (!total) return WT_OK;
    hipError_t he = hipMalloc((void**)&e->weights->x3, total);
    if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for the split weights failed: %s", total, hipGetErrorString(he));
    hipStream_t up = nullptr;
    he = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    size_t off = 0;
    for (const Job& j : jobs) {
        if (he != hipSuccess) break;
        void* dst = e->weights->x3 + off;
        he = launch_split3(j.src, dst, j.n, j.n, up);
        *j.dst = dst;
        off += align_up(j.n * 6, 256);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(up);
    if (up) hipStreamDestroy(up);
    if (he != hipSuccess) return fail(WT_E_HIP, "splitting the weights failed: %s", hipGetErrorString(he));
    e->use_x3 = true;
    return WT_OK;
}

// Decoder engines, d <= 1024: the folded cross-attention query u = fold_w . [a ; h] + fold_c is computed in two launches (enqueue_layer_part),
// each over one column half of fold_w [d][2d].  A GEMV streams contiguous rows, so the halves are repacked ONCE per engine into two
// [d][d] matrices per layer (a strided device-to-device copy; 2 d^2 weight elements per layer on top of the blob's: 8.4 MB at medium.en
// fp32), shared by the handles wt_engine_clone makes.
static int build_fold_halves(wt_engine* e) {
    if (e->kind != WT_KIND_DECODER || e->d > 1024 || e->dec_layers.empty()) return WT_OK;
    const size_t d = e->d, esz = e->w_half ? 2 : 4, half = align_up(d * d * esz, 256);
    const size_t total = half * 2 * e->dec_layers.size();
    hipError_t he = hipMalloc((void**)&e->weights->fold, total);
    if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for the folded-query halves failed: %s", total, hipGetErrorString(he));
    hipStream_t up = nullptr;
    he = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    size_t off = 0;
    for (DecLayerW& l : e->dec_layers) {
        char *wa = e->weights->fold + off, *wh = wa + half;
        const char* src = (const char*)l.fold_w;
        if (he == hipSuccess) he = hipMemcpy2DAsync(wa, d * esz, src, 2 * d * esz, d * esz, d, hipMemcpyDeviceToDevice, up);
        if (he == hipSuccess) he = hipMemcpy2DAsync(wh, d * esz, src + d * esz, 2 * d * esz, d * esz, d, hipMemcpyDeviceToDevice, up);
        l.fold_wa = wa; l.fold_wh = wh;
        off += 2 * half;
    }
    if (he == hipSuccess) he = hipStreamSynchronize(up);
    if (up) hipStreamDestroy(up);
    if (he != hipSuccess) {
        for (DecLayerW& l : e->dec_layers) l.fold_wa = l.fold_wh = nullptr;
        return fail(WT_E_HIP, "repacking the folded-query weights failed: %s", hipGetErrorString(he));
    }
    return WT_OK;
}

extern "C" int wt_engine_open(const void* blob, size_t nbytes, int device, wt_engine** out) {
    if (!blob || !out) return fail(WT_E_INVALID, "wt_engine_open: null argument");
    *out = nullptr;
    ParsedBlob pb;
    {
        char msg[400] = "";
        const int prc = parse_blob(blob, nbytes, &pb, msg, sizeof msg);  // host_logic.cpp: overflow-safe bounds, config limits
        if (prc) return fail(prc, "%s", msg);
    }
    const BlobHeader& hd = pb.hd;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(WT_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail(WT_E_HIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(guard.err));

    wt_engine* e = new wt_engine();
    e->kind = pb.dims.kind;
    e->precision = pb.dims.precision;
    e->device = device;
    e->d = pb.dims.d; e->H = pb.dims.H; e->L = pb.dims.L; e->F = pb.dims.F;
    e->C = pb.dims.C; e->S = pb.dims.S; e->T = pb.dims.T; e->V = pb.dims.V;

    // upload the tensor payload in one allocation
    const size_t payload = nbytes - hd.data_off;
    e->weights = std::make_shared<WeightStore>();
    e->weights->device = device;
    hipError_t he = hipMalloc((void**)&e->weights->base, payload ? payload : 256);
    e->weights_base = e->weights->base;
    if (he != hipSuccess) {
        int rc = fail(WT_E_NOMEM, "hipMalloc(%zu) for weights failed: %s", payload, hipGetErrorString(he));
        wt_engine_close(e);
        return rc;
    }
    {   // upload on a private non-blocking stream, not the legacy stream: a synchronous hipMemcpy is refused by the runtime while another
        // host thread (another handle's worker) is capturing its step graph
        hipStream_t up = nullptr;
        he = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
        if (he == hipSuccess) he = hipMemcpyAsync(e->weights_base, (const char*)blob + hd.data_off, payload, hipMemcpyHostToDevice, up);
        if (he == hipSuccess) he = hipStreamSynchronize(up);
        if (up) hipStreamDestroy(up);
    }
    if (he != hipSuccess) {
        int rc = fail(WT_E_HIP, "weight upload failed: %s", hipGetErrorString(he));
        wt_engine_close(e);
        return rc;
    }
    for (const BlobTensor& bt : pb.tensors) {  // entries were validated by parse_blob
        DevTensor t;
        t.ptr = (float*)(e->weights_base + (bt.offset - hd.data_off));
        t.ndim = (int)bt.ndim;
        t.dtype = (int)bt.dtype;
        for (uint32_t k = 0; k < bt.ndim; ++k) t.shape[k] = bt.shape[k];
        e->w[bt.name] = t;
    }
    // resolve the parameter tree; every lookup failure is reported by name
    g_err[0] = 0;
    auto need = [&](const std::string& name, std::initializer_list<int64_t> shape) -> const float* {
        auto it = e->w.find(name);
        if (it == e->w.end()) { if (!g_err[0]) fail(WT_E_NOTFOUND, "engine blob has no tensor '%s'", name.c_str()); return nullptr; }
        int k = 0;
        bool ok = it->second.ndim == (int)shape.size();
        for (int64_t s : shape) { ok = ok && it->second.shape[k] == s; ++k; }
        if (!ok && !g_err[0]) fail(WT_E_INVALID, "tensor '%s' has the wrong shape for this config", name.c_str());
        // fp16 engines carry their GEMM / GEMV operands (2-D *.weight, incl. the token table tied to the vocabulary projection) as
        // fp16, everything else (biases, LayerNorm parameters, position tables, the folded query's vectors) as fp32
        const bool is_gemm_w = shape.size() == 2 && name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0 &&
                               name != "embed_positions.weight";
        const int want = (e->precision == WT_F16 && is_gemm_w) ? WT_F16 : WT_F32;
        if (ok && it->second.dtype != want) {
            ok = false;
            if (!g_err[0]) fail(WT_E_INVALID, "tensor '%s' has the wrong element type for this engine precision", name.c_str());
        }
        return ok ? it->second.ptr : nullptr;
    };
    const int64_t d = e->d, F = e->F;
    if (e->kind == WT_KIND_ENCODER) {
        e->conv1_w = need("conv1.weight", {d, 3 * e->C});
        e->conv1_b = need("conv1.bias", {d});
        e->conv2_w = need("conv2.weight", {d, 3 * d});
        e->conv2_b = need("conv2.bias", {d});
        e->enc_pos = need("embed_positions", {e->S, d});
        e->enc_ln_w = need("layer_norm.weight", {d});
        e->enc_ln_b = need("layer_norm.bias", {d});
        for (int i = 0; i < e->L; ++i) {
            std::string p = "layers." + std::to_string(i) + ".";
            EncLayerW l;
            l.ln1_w = need(p + "self_attn_layer_norm.weight", {d}); l.ln1_b = need(p + "self_attn_layer_norm.bias", {d});
            l.qkv_w = need(p + "self_attn.qkv.weight", {3 * d, d}); l.qkv_b = need(p + "self_attn.qkv.bias", {3 * d});
            l.o_w = need(p + "self_attn.dense.weight", {d, d}); l.o_b = need(p + "self_attn.dense.bias", {d});
            l.ln2_w = need(p + "final_layer_norm.weight", {d}); l.ln2_b = need(p + "final_layer_norm.bias", {d});
            l.fc1_w = need(p + "fc1.weight", {F, d}); l.fc1_b = need(p + "fc1.bias", {F});
            l.fc2_w = need(p + "fc2.weight", {d, F}); l.fc2_b = need(p + "fc2.bias", {d});
            e->enc_layers.push_back(l);
        }
    } else {
        e->w_half = e->precision == WT_F16;
        e->kv_esz = e->w_half ? 2 : 4;
        e->tok_emb = need("embed_tokens.weight", {e->V, d});
        e->pos_emb = need("embed_positions.weight", {e->T, d});
        e->proj_w = hd.cfg[CFG_TIED] ? e->tok_emb : need("proj_out.weight", {e->V, d});
        e->dec_ln_w = need("layer_norm.weight", {d});
        e->dec_ln_b = need("layer_norm.bias", {d});
        for (int i = 0; i < e->L; ++i) {
            std::string p = "layers." + std::to_string(i) + ".";
            DecLayerW l;
            l.ln1_w = need(p + "self_attn_layer_norm.weight", {d}); l.ln1_b = need(p + "self_attn_layer_norm.bias", {d});
            l.qkv_w = need(p + "self_attn.qkv.weight", {3 * d, d}); l.qkv_b = need(p + "self_attn.qkv.bias", {3 * d});
            l.o_w = need(p + "self_attn.dense.weight", {d, d}); l.o_b = need(p + "self_attn.dense.bias", {d});
            l.fold_w = need(p + "encoder_attn.q_fold.weight", {d, 2 * d}); l.fold_c = need(p + "encoder_attn.q_fold.bias", {d});
            l.fold_r = need(p + "encoder_attn.q_fold.rowsum", {d}); l.fold_t = need(p + "encoder_attn.q_fold.shift", {d});
            l.ckv_w = need(p + "encoder_attn.kv.weight", {2 * d, d}); l.ckv_b = need(p + "encoder_attn.kv.bias", {2 * d});
            l.co_w = need(p + "encoder_attn.dense.weight", {d, d}); l.co_b = need(p + "encoder_attn.dense.bias", {d});
            l.ln3_w = need(p + "final_layer_norm.weight", {d}); l.ln3_b = need(p + "final_layer_norm.bias", {d});
            l.fc1_w = need(p + "fc1.weight", {F, d}); l.fc1_b = need(p + "fc1.bias", {F});
            l.fc2_w = need(p + "fc2.weight", {d, F}); l.fc2_b = need(p + "fc2.bias", {d});
            e->dec_layers.push_back(l);
        }
    }
    if (g_err[0]) {
        std::string keep = g_err;
        wt_engine_close(e);
        snprintf(g_err, sizeof g_err, "%s", keep.c_str());
        return WT_E_INVALID;
    }
    {   // fp32 engines: the weights of the big GEMMs once more as three bf16 planes (wt_common.h: launch_gemm_x3)
        static const bool x3_on = !(tuning_env("WT_GEMM_X3") && atoi(tuning_env("WT_GEMM_X3")) == 0);   // A/B switch: native fp32 MFMA GEMMs
        int rc = (x3_on && e->precision == WT_F32 && (e->d % 16) == 0 && (e->F % 16) == 0) ? build_x3_weights(e) : WT_OK;
        if (rc == WT_OK) rc = build_fold_halves(e);
        if (rc) {
            std::string keep = g_err;
            wt_engine_close(e);
            snprintf(g_err, sizeof g_err, "%s", keep.c_str());
            return rc;
        }
    }
    *out = e;
    return WT_OK;
}

extern "C" int wt_engine_clone(const wt_engine* src, wt_engine** out) {
    if (!src || !out) return fail(WT_E_INVALID, "wt_engine_clone: null argument");
    *out = nullptr;
    wt_engine* e = new wt_engine();
    e->kind = src->kind; e->device = src->device; e->precision = src->precision;
    e->d = src->d; e->H = src->H; e->L = src->L; e->F = src->F; e->C = src->C; e->S = src->S; e->T = src->T; e->V = src->V;
    e->weights = src->weights;            // shared, read-only
    e->weights_base = src->weights_base;
    e->w = src->w;
    e->enc_layers = src->enc_layers;
    e->conv1_w = src->conv1_w; e->conv1_b = src->conv1_b; e->conv2_w = src->conv2_w; e->conv2_b = src->conv2_b;
    e->enc_pos = src->enc_pos; e->enc_ln_w = src->enc_ln_w; e->enc_ln_b = src->enc_ln_b;
    e->dec_layers = src->dec_layers;
    e->tok_emb = src->tok_emb; e->pos_emb = src->pos_emb; e->proj_w = src->proj_w; e->dec_ln_w = src->dec_ln_w; e->dec_ln_b = src->dec_ln_b;
    e->w_half = src->w_half; e->kv_esz = src->kv_esz; e->use_x3 = src->use_x3; e->conv1_w3 = src->conv1_w3; e->conv2_w3 = src->conv2_w3;
    // workspace, resident caches, step graphs, streams, mailbox, timers: this handle's own, allocated on first use like a fresh engine's
    *out = e;
    return WT_OK;
}

extern "C" int wt_engine_get_info(const wt_engine* e, wt_engine_info* out) {
    if (!e || !out) return fail(WT_E_INVALID, "wt_engine_get_info: null argument");
    out->kind = e->kind; out->precision = e->precision;
    out->d_model = e->d; out->n_heads = e->H; out->n_layers = e->L; out->ffn_dim = e->F;
    out->n_mels = e->C; out->max_source_positions = e->S; out->max_target_positions = e->T; out->vocab_size = e->V;
    return WT_OK;
}

extern "C" int wt_engine_gemm_mode(const wt_engine* e) { return e && e->use_x3 ? 1 : 0; }

// ------------------------------------------------------------------------------------------------- encoder
// (workspace clears are stream-ordered on the CALLER's stream: a synchronous hipMemset runs on the legacy stream, which the runtime
// refuses while ANOTHER host thread -- another worker's handle -- is capturing its step graph)
static int enc_reserve(wt_engine* e, int B, hipStream_t s) {
    if (B <= e->enc_cap) return WT_OK;
    if (e->enc_ws) { hipFree(e->enc_ws); e->enc_ws = nullptr; e->enc_cap = 0; }
    const size_t M = (size_t)B * e->S, d = e->d;
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
    size_t n_melT, n_c1;   // elements (per plane)
    conv_ws_elems(B, e->S, e->C, e->d, n_melT, n_c1);
    const size_t o_melT = take(n_melT);
    const size_t o_c1 = take(n_c1);
    const size_t o_h = take(M * d), o_x = take(M * d), o_qkv = take(M * 3 * d), o_ctx = take(M * d), o_ffn = take(M * e->F);
    // x3 GEMMs: their A operands as three bf16 planes (6 bytes per element = 1.5 floats)
    const size_t o_xs3 = take(e->use_x3 ? (M * d * 3 + 1) / 2 : 0), o_ctx3 = take(e->use_x3 ? (M * d * 3 + 1) / 2 : 0), o_ffn3 = take(e->use_x3 ? (M * e->F * 3 + 1) / 2 : 0);
    const size_t o_qkv3 = take(e->use_x3 ? (M * 3 * d * 3 + 1) / 2 : 0);
    const size_t o_melT3 = take(e->conv1_w3 ? (n_melT * 3 + 1) / 2 : 0), o_c1_3 = take(e->conv1_w3 ? (n_c1 * 3 + 1) / 2 : 0);
    // fp16 engines reuse the fp32-sized regions for their half-precision activations (half the bytes)
    hipError_t he = hipMalloc((void**)&e->enc_ws, off);
    if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for encoder workspace (batch %d) failed: %s", off, B, hipGetErrorString(he));
    e->melT = (float*)(e->enc_ws + o_melT); e->c1 = (float*)(e->enc_ws + o_c1); e->hbuf = (float*)(e->enc_ws + o_h);
    e->xbuf = (float*)(e->enc_ws + o_x); e->qkv = (float*)(e->enc_ws + o_qkv); e->ctx = (float*)(e->enc_ws + o_ctx);
    e->ffn = (float*)(e->enc_ws + o_ffn);
    e->xs3 = e->enc_ws + o_xs3; e->ctx3 = e->enc_ws + o_ctx3; e->ffn3 = e->enc_ws + o_ffn3; e->qkv3 = e->enc_ws + o_qkv3;
    e->melT3 = e->enc_ws + o_melT3; e->c1_3 = e->enc_ws + o_c1_3;
    e->melT3_plane = n_melT; e->c1_3_plane = n_c1;
    if (e->conv1_w3) HIPCHK(conv_ws_clear(e->melT3, n_melT, e->c1_3, n_c1, 6, s));   // zero padding rows of the plane forms (a bf16 zero is all-zero bits)
    e->melT_h = e->melT; e->c1_h = e->c1; e->x_h = e->xbuf; e->ffn_h = e->ffn;
    e->ctx_h = (char*)e->ffn + M * e->F * 2;  // second half of the ffn region (M*F*2 bytes >= M*d*2)
    // conv zero-padding rows (row 0 / row F+1 of every utterance) are never written by the kernels below
    HIPCHK(conv_ws_clear(e->melT, n_melT, e->c1, n_c1, 4, s));
    // Growth is rare.  The ABI takes a stream per call: finish the clears before returning, so that a following call on this handle
    // from a DIFFERENT stream cannot overtake them (allowed while other threads capture: thread-local capture mode)
    HIPCHK(hipStreamSynchronize(s));
    e->enc_cap = B;
    return WT_OK;
}

#define LAUNCH(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return fail(WT_E_HIP, "kernel launch %s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// LAUNCH between the two event records of `timer` (no events unless the handle is profiling)
#define TIMED(e, timer, s, expr)                  \
    do {                                          \
        hipEvent_t _ta, _tb;                      \
        timer_begin(e, timer, s, &_ta, &_tb);     \
        LAUNCH(expr);                             \
        timer_end(e, timer, s, _ta, _tb);         \
    } while (0)

static int timed_gemm(wt_engine* e, const GemmParams& p, hipStream_t s) {
    TIMED(e, e->t_gemm, s, launch_gemm_f32(p, s));
    return WT_OK;
}

// fp16 encoder: fp16 GEMM operands, fp32 accumulation / residual stream / LayerNorm statistics / attention.
static int encoder_forward_f16(wt_engine* e, const float* mel, int B, float* out, hipStream_t s) {
    const int S = e->S, Fr = 2 * S, d = e->d, C = e->C, M = B * S;
    int rc;
    auto hgemm = [&](const GemmParams& q, bool out_half) {
        TIMED(e, e->t_gemm, s, launch_gemm_f16(q, out_half, s));
        return (int)WT_OK;
    };
    LAUNCH(launch_mel_transpose_h(mel, e->melT_h, B, C, Fr, s));
    {
        size_t n_melT, n_c1;
        conv_ws_elems(B, S, C, d, n_melT, n_c1);
        GemmParams c1g, c2g;
        conv_gemm_params(CONV_F16, e->melT_h, n_melT, e->c1_h, n_c1, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, e->enc_pos, e->hbuf, B, S, C, d,
                         c1g, c2g);
        if ((rc = hgemm(c1g, true))) return rc;
        if ((rc = hgemm(c2g, false))) return rc;
    }
    auto dense = [&](const void* A, int K, const float* Wt, const float* bias, int N, void* Cout, int act, const float* resid,
                     bool out_half) {
        GemmParams q;
        memset(&q, 0, sizeof q);
        q.A = (const float*)A; q.lda = K; q.a_rows_per_batch = M; q.W = Wt; q.bias = bias; q.M = M; q.N = N; q.K = K; q.act = act;
        q.C = (float*)Cout; q.ldc = N; q.c_rows_per_batch = M; q.resid = resid;
        return hgemm(q, out_half);
    };
    for (int i = 0; i < e->L; ++i) {
        const EncLayerW& l = e->enc_layers[i];
        LAUNCH(launch_layernorm_h(e->hbuf, l.ln1_w, l.ln1_b, e->x_h, M, d, s));
        if ((rc = dense(e->x_h, d, l.qkv_w, l.qkv_b, 3 * d, e->qkv, 0, nullptr, true))) return rc;   // q|k|v as fp16
        TIMED(e, e->t_enc_attn, s, launch_encoder_attention_f16(e->qkv, e->ctx_h, B, S, e->H, s));   // fp16 in/out, fp32 softmax
        if ((rc = dense(e->ctx_h, d, l.o_w, l.o_b, d, e->hbuf, 0, e->hbuf, false))) return rc;
        LAUNCH(launch_layernorm_h(e->hbuf, l.ln2_w, l.ln2_b, e->x_h, M, d, s));
        if ((rc = dense(e->x_h, d, l.fc1_w, l.fc1_b, e->F, e->ffn_h, 1, nullptr, true))) return rc;
        if ((rc = dense(e->ffn_h, e->F, l.fc2_w, l.fc2_b, d, e->hbuf, 0, e->hbuf, false))) return rc;
    }
    LAUNCH(launch_layernorm(e->hbuf, e->enc_ln_w, e->enc_ln_b, out, M, d, s));
    return WT_OK;
}

extern "C" int wt_encoder_forward(wt_engine* e, const float* mel, int B, float* out, void* stream) {
    if (!e || e->kind != WT_KIND_ENCODER) return fail(WT_E_INVALID, "wt_encoder_forward: not an encoder engine");
    if (!mel || !out || B < 1) return fail(WT_E_INVALID, "wt_encoder_forward: bad arguments (batch %d)", B);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    int rc = enc_reserve(e, B, s);
    if (rc) return rc;
    const int S = e->S, Fr = 2 * S, d = e->d, C = e->C, M = B * S;
    if (e->precision == WT_F16) return encoder_forward_f16(e, mel, B, out, s);
    bool convs_x3 = false;
    size_t n_melT, n_c1;
    conv_ws_elems(B, S, C, d, n_melT, n_c1);
    if (e->use_x3 && e->conv1_w3) {   // both convolutions as launch_gemm_x3 (operand planes; conv1's GELU output goes out as planes for conv2)
        GemmParams c1g, c2g;
        conv_gemm_params(CONV_X3, e->melT3, e->melT3_plane, e->c1_3, e->c1_3_plane, e->conv1_w3, e->conv1_b, e->conv2_w3, e->conv2_b, e->enc_pos,
                         e->hbuf, B, S, C, d, c1g, c2g);
        if (gemm_x3_usable(c1g) && gemm_x3_usable(c2g)) {
            convs_x3 = true;
            LAUNCH(launch_mel_transpose_split(mel, e->melT3, e->melT3_plane, B, C, Fr, s));
            for (const GemmParams* q : {&c1g, &c2g}) TIMED(e, e->t_gemm, s, launch_gemm_x3(*q, s));
        }
    }
    if (!convs_x3) {
        LAUNCH(launch_mel_transpose(mel, e->melT, B, C, Fr, s));
        // conv1 (k=3, pad 1) + GELU as an implicit GEMM over the time-major padded mel (model.py:78,97), then
        // conv2 (k=3, stride 2, pad 1) + GELU + embed_positions, written as [B*S, d] (model.py:79,98-102)
        GemmParams c1g, c2g;
        conv_gemm_params(CONV_F32, e->melT, n_melT, e->c1, n_c1, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, e->enc_pos, e->hbuf, B, S, C, d,
                         c1g, c2g);
        if ((rc = timed_gemm(e, c1g, s))) return rc;
        if ((rc = timed_gemm(e, c2g, s))) return rc;
    }

    auto dense = [&](const float* A, int K, const float* Wt, const float* bias, int N, float* Cout, int act,
                     const float* resid) {
        GemmParams q;
        memset(&q, 0, sizeof q);
        q.A = A; q.lda = K; q.a_rows_per_batch = M; q.W = Wt; q.bias = bias; q.M = M; q.N = N; q.K = K; q.act = act;
        q.C = Cout; q.ldc = N; q.c_rows_per_batch = M; q.resid = resid;
        return timed_gemm(e, q, s);
    };
    // launch_gemm_x3 form of a layer GEMM: A / W as three bf16 planes, fp32 (or, for fc1, three-plane) output
    auto dense3 = [&](const void* A3, int K, const void* W3, const float* bias, int N, void* Cout, int act, const float* resid, bool out_split) {
        GemmParams q;
        memset(&q, 0, sizeof q);
        q.A = (const float*)A3; q.lda = K; q.a_rows_per_batch = M; q.a_plane = (long long)M * K; q.W = (const float*)W3; q.w_plane = (long long)N * K;
        q.bias = bias; q.M = M; q.N = N; q.K = K; q.act = act; q.C = (float*)Cout; q.ldc = N; q.c_rows_per_batch = M; q.resid = resid;
        q.out_split = out_split ? 1 : 0; q.c_plane = (long long)M * N;
        TIMED(e, e->t_gemm, s, launch_gemm_x3(q, s));
        return (int)WT_OK;
    };
    if (e->use_x3) {
        // fp32 products formed from six bf16 MFMAs of exactly split operands (wt_common.h: launch_gemm_x3): every producer of a GEMM's
        // A operand -- LayerNorm, attention, fc1's GELU epilogue -- writes the three planes directly, so no extra pass splits anything
        const size_t pl_d = (size_t)M * d;
        for (int i = 0; i < e->L; ++i) {
            const EncLayerW& l = e->enc_layers[i];
            LAUNCH(launch_layernorm_split(e->hbuf, l.ln1_w, l.ln1_b, e->xs3, pl_d, M, d, s));
            static const bool attn_x3 = !(tuning_env("WT_ATTN_X3") && atoi(tuning_env("WT_ATTN_X3")) == 0);   // A/B switch: fp32-MFMA attention
            if ((rc = dense3(e->xs3, d, l.qkv_w3, l.qkv_b, 3 * d, attn_x3 ? e->qkv3 : (void*)e->qkv, 0, nullptr, attn_x3))) return rc;
            if (attn_x3) TIMED(e, e->t_enc_attn, s, launch_encoder_attention_x3(e->qkv3, (size_t)M * 3 * d, e->ctx3, pl_d, B, S, e->H, s));
            else TIMED(e, e->t_enc_attn, s, launch_encoder_attention(e->qkv, nullptr, B, S, e->H, s, e->ctx3, pl_d));
            if ((rc = dense3(e->ctx3, d, l.o_w3, l.o_b, d, e->hbuf, 0, e->hbuf, false))) return rc;
            LAUNCH(launch_layernorm_split(e->hbuf, l.ln2_w, l.ln2_b, e->xs3, pl_d, M, d, s));
            if ((rc = dense3(e->xs3, d, l.fc1_w3, l.fc1_b, e->F, e->ffn3, 1, nullptr, true))) return rc;
            if ((rc = dense3(e->ffn3, e->F, l.fc2_w3, l.fc2_b, d, e->hbuf, 0, e->hbuf, false))) return rc;
        }
        LAUNCH(launch_layernorm(e->hbuf, e->enc_ln_w, e->enc_ln_b, out, M, d, s));
        return WT_OK;
    }
    for (int i = 0; i < e->L; ++i) {
        const EncLayerW& l = e->enc_layers[i];
        LAUNCH(launch_layernorm(e->hbuf, l.ln1_w, l.ln1_b, e->xbuf, M, d, s));
        if ((rc = dense(e->xbuf, d, l.qkv_w, l.qkv_b, 3 * d, e->qkv, 0, nullptr))) return rc;
        TIMED(e, e->t_enc_attn, s, launch_encoder_attention(e->qkv, e->ctx, B, S, e->H, s));
        if ((rc = dense(e->ctx, d, l.o_w, l.o_b, d, e->hbuf, 0, e->hbuf))) return rc;
        LAUNCH(launch_layernorm(e->hbuf, l.ln2_w, l.ln2_b, e->xbuf, M, d, s));
        if ((rc = dense(e->xbuf, d, l.fc1_w, l.fc1_b, e->F, e->ffn, 1, nullptr))) return rc;
        if ((rc = dense(e->ffn, e->F, l.fc2_w, l.fc2_b, d, e->hbuf, 0, e->hbuf))) return rc;
    }
    LAUNCH(launch_layernorm(e->hbuf, e->enc_ln_w, e->enc_ln_b, out, M, d, s));
    return WT_OK;
}

// ------------------------------------------------------------------------------------------------- decoder
static int dec_reserve(wt_engine* e, int B, int max_length, hipStream_t s, int pool_rows = 0) {
    if (B <= e->dec_cap && max_length <= e->dec_maxlen_cap && pool_rows <= e->cross_rows) return WT_OK;
    if (B < e->dec_cap) B = e->dec_cap;                      // never shrink: a later, smaller call keeps what an earlier one needed
    if (max_length < e->dec_maxlen_cap) max_length = e->dec_maxlen_cap;
    if (pool_rows < e->cross_rows) pool_rows = e->cross_rows;
    if (e->dec_ws) { hipFree(e->dec_ws); e->dec_ws = nullptr; e->dec_cap = 0; e->cross_rows = 0; }
    e->ws_gen += 1;
    e->tables_valid = false;
    const int cap_len = max_length > e->T ? max_length : e->T;
    const int cross_rows = pool_rows > B ? pool_rows : B, enc_rows = B > MAX_ROWS ? B : MAX_ROWS;
    const size_t d = e->d, kv_self = (size_t)e->L * B * e->H * e->T * HEAD_DIM, kv_cross = (size_t)e->L * cross_rows * e->H * e->S * HEAD_DIM;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_sk = take(kv_self * e->kv_esz), o_sv = take(kv_self * e->kv_esz), o_ck = take(kv_cross * e->kv_esz), o_cv = take(kv_cross * e->kv_esz);
    const size_t o_ench = take(e->w_half ? (size_t)enc_rows * e->S * d * 2 : 0);
    const size_t o_enc3 = take(e->use_x3 ? (size_t)enc_rows * e->S * d * 6 : 0);
    const size_t o_h = take((size_t)B * d * 4), o_h2 = take((size_t)B * d * 4), o_q = take((size_t)B * d * 4), o_att = take((size_t)B * d * 4), o_f = take((size_t)B * e->F * 4);
    const size_t o_uh = take((size_t)B * d * 4);
    const size_t o_cnt = take((size_t)B * e->H * 4);
    const size_t o_selv = take((size_t)B * SEL_PARTS_CAP * 4), o_seli = take((size_t)B * SEL_PARTS_CAP * 4);
    const size_t o_part = take((size_t)B * e->H * 16 * PART_STRIDE * 4), o_lg = take((size_t)B * e->V * 4);
    const size_t o_st = take(sizeof(DecState)), o_ids = take((size_t)B * cap_len * 4), o_unf = take((size_t)B * 4);
    const size_t o_forced = take((size_t)(cap_len + 1) * 4), o_mask = take((size_t)e->V), o_frows = take(16 * 4);
    const size_t o_tsp = take((size_t)B * SELECT_CHUNKS * sizeof(TsPart));
    const size_t o_lpp = take((size_t)B * SEL_PARTS_CAP * sizeof(float4)), o_lps = take((size_t)B * 2 * 4), o_lpt = take((size_t)B * cap_len * 4);
    const size_t o_lpsum = take((size_t)B * 4), o_lpn = take((size_t)B * 4);
    const size_t o_sseed = take((size_t)B * 8), o_ssc = take((size_t)B * SEL_PARTS_CAP * 4), o_sts = take((size_t)B * SELECT_CHUNKS * sizeof(float4));
    // beam search state (BeamParams): sized for MAX_ROWS rows whatever B, it is small
    const size_t o_bpart = take((size_t)MAX_ROWS * SELECT_CHUNKS * sizeof(BeamPart)), o_bsc = take(MAX_ROWS * 4), o_bids2 = take((size_t)MAX_ROWS * cap_len * 4);
    const size_t o_banc = take((size_t)2 * MAX_ROWS * cap_len * 4), o_burow = take(MAX_ROWS * 4), o_bhn = take(MAX_ROWS * 4), o_bhd = take(MAX_ROWS * 4);
    const size_t o_bhw = take(MAX_ROWS * 8), o_bhs = take(MAX_ROWS * 8), o_bhl = take(MAX_ROWS * 4), o_bhi = take((size_t)MAX_ROWS * cap_len * 4);
    const size_t o_bout = take((size_t)MAX_ROWS * cap_len * 4), o_bos = take(MAX_ROWS * 4), o_btr = take((size_t)cap_len * MAX_ROWS * 4 * 4);
    const size_t o_lang = take((size_t)(MAX_ROWS + LANG_MAX) * 4), o_langp = take((size_t)MAX_ROWS * LANG_MAX * 4);
    hipError_t he = hipMalloc((void**)&e->dec_ws, off);
    if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for decoder workspace (batch %d) failed: %s", off, B, hipGetErrorString(he));
    char* b = e->dec_ws;
    e->self_k = (float*)(b + o_sk); e->self_v = (float*)(b + o_sv); e->cross_k = (float*)(b + o_ck); e->cross_v = (float*)(b + o_cv);
    e->dh = (float*)(b + o_h); e->dh2 = (float*)(b + o_h2); e->dq = (float*)(b + o_q); e->datt = (float*)(b + o_att); e->att_cnt = (int*)(b + o_cnt); e->sel_val = (float*)(b + o_selv); e->sel_idx = (int*)(b + o_seli); e->dffn = (float*)(b + o_f); e->part = (float*)(b + o_part);
    e->duh = (float*)(b + o_uh);
    e->logits = (float*)(b + o_lg); e->st = (DecState*)(b + o_st); e->ids = (int*)(b + o_ids); e->unfinished = (int*)(b + o_unf);
    e->forced = (int*)(b + o_forced); e->mask = (uint8_t*)(b + o_mask); e->force_rows = (int*)(b + o_frows); e->ts_part = (TsPart*)(b + o_tsp);
    e->lp_part = (float4*)(b + o_lpp); e->lp_side = (float*)(b + o_lps); e->lp_tok = (float*)(b + o_lpt); e->lp_sum = (float*)(b + o_lpsum); e->lp_nsp = (float*)(b + o_lpn);
    e->lang_tok = (int*)(b + o_lang); e->lang_ids = e->lang_tok + MAX_ROWS; e->lang_prob = (float*)(b + o_langp);
    e->samp_seeds = (unsigned long long*)(b + o_sseed); e->samp_sc = (float*)(b + o_ssc); e->samp_ts = (float4*)(b + o_sts);
    {
        BeamParams& bp = e->beam_dev;
        memset(&bp, 0, sizeof bp);
        bp.part = (BeamPart*)(b + o_bpart); bp.scores = (float*)(b + o_bsc); bp.ids2 = (int*)(b + o_bids2); bp.anc = (int*)(b + o_banc); bp.anc_ld = cap_len;
        bp.urow = (int*)(b + o_burow); bp.hyp_n = (int*)(b + o_bhn); bp.hyp_done = (int*)(b + o_bhd); bp.hyp_worst = (double*)(b + o_bhw);
        bp.hyp_score = (double*)(b + o_bhs); bp.hyp_len = (int*)(b + o_bhl); bp.hyp_ids = (int*)(b + o_bhi); bp.hyp_ld = cap_len;
        bp.out_ids = (int*)(b + o_bout); bp.out_scores = (float*)(b + o_bos); bp.trace = (int*)(b + o_btr);
    }
    e->h_force_rows.clear();
    e->enc_h = e->w_half ? (void*)(b + o_ench) : nullptr;
    e->enc3 = e->use_x3 ? (void*)(b + o_enc3) : nullptr;
    HIPCHK(hipMemsetAsync(e->att_cnt, 0, (size_t)B * e->H * 4, s));  // arrival tickets start (and are left) at zero; stream-ordered (see enc_reserve)
    if (!e->h_state) HIPCHK(hipHostMalloc((void**)&e->h_state, sizeof(DecState), hipHostMallocDefault));
    if (!e->mailbox) {
        HIPCHK(hipHostMalloc((void**)&e->mailbox, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *e->mailbox = 0;
        HIPCHK(hipHostGetDevicePointer((void**)&e->mailbox_dev, (void*)e->mailbox, 0));
    }
    if (!e->own_stream) {
        HIPCHK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    }
    HIPCHK(hipStreamSynchronize(s));   // as in enc_reserve: the ticket clear above is ordered before any later call on any stream
    e->dec_cap = B;
    e->cross_rows = cross_rows;
    e->dec_maxlen_cap = cap_len;
    return WT_OK;
}

// one decoder step over the resident (or caller-provided) caches; every step-dependent quantity comes from *st
struct StepIO {
    const int* ids; int ids_ld;            // token fed to row b = ids[b*ids_ld + st->cur_len-1]
    float *self_k, *self_v; int self_cap;  // layer stride = B*H*self_cap*64 elements
    float *cross_k, *cross_v;              // layer stride = cross_rows*H*S*64 elements
    int cross_rows;                        // cache rows per layer (the engine's resident pool; 1 on the Session path)
    const int* slot_row;                   // continuous mode: slot b attends over cache row slot_row[b] (DecAttnParams.slot_row)
    int group = 0;                         // beam search: grouped cross attention (DecAttnParams.group) instead of slot_row
    const int* anc = nullptr;              // beam search: ancestry table of the self-attention (DecAttnParams.anc), row stride anc_ld
    int anc_ld = 0;
    float* qh = nullptr;                   // token-level timestamps: query history of the cross attention (DecAttnParams.qh), [n_sel][qh_rows][qh_steps][64]
    const int* qh_sel = nullptr;           // [L][H] selection index or -1
    int qh_rows = 0, qh_steps = 0;
    int kv_esz;                            // bytes per cache element: 4 (fp32; always on the Session path), 2 (resident caches of an fp16 engine)
    float* logits;                         // [B][V]
    int B, nsplit_self, nsplit_cross;
    int nt;                                // stream weights and K/V with non-temporal loads (StepKey.nt_loads)
    const int* alive;                      // skip-finished-rows graph of the fast path: per-row "unfinished" flags (DecAttnParams.alive)
    bool embed;                            // launch the input-embedding kernel (the fast path gets it from greedy_finish)
    // greedy fast path: masked argmax fused into the vocabulary GEMV (logits == nullptr: they never reach HBM unless traced)
    const SelectParams* argmax;            // or nullptr: write plain logits
    int* argmax_parts;                     // out: partial results per batch row (workgroups of the GEMV)
    bool lang = false;                     // language detection: lang_select_kernel on the final hidden state, beside the vocabulary stage
};

// The seven dependent launches of decoder layer i (model.py:321-369).  h = residual stream in, h1 = the other buffer of the
// two-buffer stream (the layer's output ends up in h1).  `part` selects one launch: the decode step enqueues 0..6 in order,
// wt_decoder_time_kernel replays one kind over all layers.
enum { LP_QKV = 0, LP_SELF_ATTN, LP_PAIR, LP_CROSS_ATTN, LP_CROSS_OUT, LP_FC1, LP_FC2, LP_COUNT };
static int enqueue_layer_part(wt_engine* e, const StepIO& io, int i, float* h, float* h1, int part, hipStream_t s) {
    static const bool defer = tuning_env("WT_NO_DEFER_MERGE") == nullptr;  // A/B switch
    // A/B switch: WT_QFOLD_HOIST=0 keeps the whole folded query in the pair launch (K = 2d over [a ; h], x_direct / half-staged)
    static const bool hoist_on = !(tuning_env("WT_QFOLD_HOIST") && atoi(tuning_env("WT_QFOLD_HOIST")) == 0);
    const int d = e->d, B = io.B, H = e->H;
    const DecLayerW& l = e->dec_layers[i];
    // The half of the folded query that multiplies the layer input h does not depend on the self-attention: it rides in the q|k|v launch
    // (whose workgroups leave compute units idle) and reaches the pair launch as a residual.  Where the repacked halves exist: d <= 1024.
    const bool hoist = hoist_on && l.fold_wa && l.fold_wh && d <= 1024;
    const size_t self_layer = (size_t)i * B * H * io.self_cap * HEAD_DIM * io.kv_esz, cross_layer = (size_t)i * io.cross_rows * H * e->S * HEAD_DIM * io.kv_esz;
    float* sk = (float*)((char*)io.self_k + self_layer);
    float* sv = (float*)((char*)io.self_v + self_layer);
    const float* ck = (const float*)((const char*)io.cross_k + cross_layer);
    const float* cv = (const float*)((const char*)io.cross_v + cross_layer);
    const int wh = e->w_half ? 1 : 0, kvh = io.kv_esz == 2 ? 1 : 0;
    SkinnyParams k, k2;
    DecAttnParams a;
    memset(&k, 0, sizeof k);
    memset(&k2, 0, sizeof k2);
    memset(&a, 0, sizeof a);
    switch (part) {
    case LP_QKV:  // self attention (model.py:273-281, 283-304): LN -> q|k|v, append k/v row in place
        k = qkv_append_skinny_params(h, l.ln1_w, l.ln1_b, l.qkv_w, l.qkv_b, e->dq, sk, sv, e->st, B, d, io.self_cap, io.nt, wh, kvh);
        if (hoist) {   // + uh = fold_wh . h + fold_c on the raw row, in the same launch
            k2 = qfold_resid_skinny_params(h, l.fold_wh, l.fold_c, e->duh, e->st, B, d, io.nt, wh);
            LAUNCH(launch_skinny_qkv_hoist(k, k2, s));
        } else {
            LAUNCH(launch_skinny(k, s));
        }
        break;
    case LP_SELF_ATTN:
        a.q = e->dq; a.kcache = sk; a.vcache = sv; a.part = e->part; a.cnt = e->att_cnt; a.out = e->datt; a.st = e->st; a.B = B; a.H = H; a.s_cap = io.self_cap;
        a.n_split = io.nsplit_self; a.fixed_len = 0; a.nt = io.nt; a.kv_half = kvh; a.alive = io.alive;
        a.anc = io.anc; a.anc_ld = io.anc_ld;
        a.defer_merge = defer && io.nsplit_self == 2;   // both halves of the pair launch below merge the two partials while staging
        LAUNCH(launch_dec_attn(a, s));
        break;
    case LP_PAIR:
        // ONE launch: out-projection + residual (h1 = h + Wo.a + bo) and the folded cross-attention query
        // u = s.Wq.diag(gamma2).(h + Wo.a + bo) = fold_w.[a ; h] + fold_c; LayerNorm statistics of h1 are applied
        // by the cross-attention kernel (model.py:261-272 semantics, one dependent launch fewer per layer)
        k.X = e->datt; k.xmode = XMODE_PLAIN; k.W = l.o_w; k.bias = l.o_b; k.resid = h;
        k.Y = h1; k.st = e->st; k.B = B; k.N = d; k.K = d; k.q_scale = 1.f; k.w_nt = io.nt; k.w_half = wh;
        if (hoist) {   // u = fold_wa . a + uh: both halves of the launch read only `a`, staged (and merged) once per workgroup
            k2 = qfold_ctx_skinny_params(e->datt, defer && io.nsplit_self == 2 ? e->part : nullptr, l.fold_wa, e->duh, e->dq, e->st, B, d,
                                         io.nt, wh);
        } else {
            k2.X = e->datt; k2.X2 = h; k2.xmode = XMODE_PLAIN; k2.x_direct = 1; k2.W = l.fold_w; k2.bias = l.fold_c;
            k2.Y = e->dq; k2.st = e->st; k2.B = B; k2.N = d; k2.K = 2 * d; k2.q_scale = 1.f; k2.w_nt = io.nt; k2.w_half = wh;
        }
        if (defer && io.nsplit_self == 2) {   // the self-attention context `a` arrives as two split partials per (utterance, head)
            k.parts = e->part; k.parts_nsplit = 2; k.parts_H = H;
            if (!hoist) { k2.parts = e->part; k2.parts_nsplit = 2; k2.parts_H = H; }
        }
        LAUNCH(launch_skinny_pair(k, k2, s));
        break;
    case LP_CROSS_ATTN: {  // cross attention over the encoder memory: K/V already resident
        a.q = e->dq; a.kcache = ck; a.vcache = cv; a.part = e->part; a.cnt = e->att_cnt; a.out = e->datt; a.st = e->st; a.B = B; a.H = H; a.s_cap = e->S;
        a.n_split = io.nsplit_cross; a.fixed_len = e->S; a.nt = io.nt; a.ln_h = h1; a.ln_r = l.fold_r; a.ln_t = l.fold_t; a.kv_half = kvh;
        a.alive = io.alive; a.slot_row = io.slot_row;
        if (io.group > 1) { a.group = io.group; a.slot_row = nullptr; }
        if (io.qh) { a.qh = io.qh; a.qh_sel = io.qh_sel + (size_t)i * H; a.qh_rows = io.qh_rows; a.qh_steps = io.qh_steps; }
        a.defer_merge = defer && io.nsplit_cross == 2;  // the out-projection below merges the two split partials while staging them
                                                        // (more splits, i.e. batch < 8: the attention kernel merges its own, by ticket)
        TIMED(e, e->t_cross, s, launch_dec_attn(a, s));
        break;
    }
    case LP_CROSS_OUT:
        k.X = e->datt; k.xmode = XMODE_PLAIN; k.W = l.co_w; k.bias = l.co_b; k.resid = h1;
        k.Y = h1; k.st = e->st; k.B = B; k.N = d; k.K = d; k.q_scale = 1.f; k.w_nt = io.nt; k.w_half = wh;
        if (defer && io.nsplit_cross == 2) { k.parts = e->part; k.parts_nsplit = io.nsplit_cross; k.parts_H = H; }
        LAUNCH(launch_skinny(k, s));
        break;
    case LP_FC1:  // FFN (model.py:363-367)
        k.X = h1; k.ln_w = l.ln3_w; k.ln_b = l.ln3_b; k.xmode = XMODE_LAYERNORM; k.W = l.fc1_w; k.bias = l.fc1_b;
        k.Y = e->dffn; k.st = e->st; k.B = B; k.N = e->F; k.K = d; k.act = 1; k.q_scale = 1.f; k.w_nt = io.nt; k.w_half = wh;
        LAUNCH(launch_skinny(k, s));
        break;
    case LP_FC2:
        k.X = e->dffn; k.xmode = XMODE_PLAIN; k.W = l.fc2_w; k.bias = l.fc2_b; k.resid = h1; k.Y = h1; k.st = e->st;
        k.B = B; k.N = d; k.K = e->F; k.q_scale = 1.f; k.w_nt = io.nt; k.w_half = wh;
        LAUNCH(launch_skinny(k, s));
        break;
    default:
        return fail(WT_E_INVALID, "enqueue_layer_part: bad part %d", part);
    }
    return WT_OK;
}

static int enqueue_step(wt_engine* e, const StepIO& io, hipStream_t s) {
    const int d = e->d, B = io.B;
    if (io.embed) LAUNCH(launch_dec_embed(io.ids, io.ids_ld, e->tok_emb, e->pos_emb, e->dh, B, d, e->st, s, e->w_half));
    SkinnyParams k;
    // The residual stream ping-pongs between two buffers once per layer: the self-attention out-projection (h1 = h + Wo.a)
    // and the folded cross-attention query (which still reads h) share one launch, so h1 cannot overwrite h in place.
    float *h = e->dh, *h1 = e->dh2;
    for (int i = 0; i < e->L; ++i) {
        for (int part = 0; part < LP_COUNT; ++part) {
            const int rc = enqueue_layer_part(e, io, i, h, h1, part, s);
            if (rc) return rc;
        }
        std::swap(h, h1);
    }
    // final LN + vocabulary projection (model.py:455-457; logits are the engine's 'hidden_states' output)
    k = vocab_skinny_params(h, e->dec_ln_w, e->dec_ln_b, e->proj_w, io.logits, e->st, B, e->V, d, io.nt, e->w_half);
    if (io.argmax) {  // Suppress -> SuppressAtBegin -> argmax in the epilogue (Force / pad / EOS rules: greedy_finish_kernel)
        const int grid = vocab_skinny_fuse_argmax(k, *io.argmax);
        if (grid < 1 || grid > SEL_PARTS_CAP) return fail(WT_E_UNSUPPORTED, "vocabulary GEMV plan has %d workgroups (cap %d)", grid, SEL_PARTS_CAP);
        *io.argmax_parts = grid;
    }
    TIMED(e, e->t_skinny, s, launch_skinny(k, s));
    if (io.lang) {   // the first step of a decode that detects languages: the rows' language tokens, in front of the finish kernel that appends them
        const LangSelectParams lp = lang_select_params(h, e->dec_ln_w, e->dec_ln_b, e->proj_w, e->w_half, e->lang_ids, e->cfg.key.n_lang, B, d,
                                                       e->lang_tok, e->lang_prob);
        LAUNCH(launch_lang_select(lp, s));
    }
    return WT_OK;
}

static int cross_kv_project(wt_engine* e, const float* enc_hidden, int B, int rows, int seq_off, float* ck, float* cv, int kv_esz,
                            hipStream_t s, int layer_rows = 0, int row0 = 0) {
    // K/V projection of encoder rows [0, rows) of every utterance into cache rows [seq_off, seq_off+rows).  fp16 engines: the encoder
    // memory is rounded to fp16 once (the MFMA's A operand), the product accumulates in fp32 and lands in the caches as `kv_esz` says.
    // The caches hold `layer_rows` utterance rows per layer (default B); the B utterances land in rows [row0, row0 + B).
    const int d = e->d;
    if (layer_rows <= 0) layer_rows = B;
    if (row0 < 0 || row0 + B > layer_rows) return fail(WT_E_INVALID, "cross_kv_project: rows [%d, %d) outside a cache of %d rows per layer", row0, row0 + B, layer_rows);
    const size_t row_bytes = (size_t)e->H * e->S * HEAD_DIM * kv_esz;
    if (e->w_half) LAUNCH(launch_cast_h(enc_hidden, e->enc_h, (size_t)B * e->S * d, s));
    const size_t enc_plane = (size_t)B * e->S * d;
    const void* A = e->w_half ? (const void*)e->enc_h : (const void*)enc_hidden;
    bool x3 = e->use_x3 && !e->w_half && B <= (e->dec_cap > MAX_ROWS ? e->dec_cap : MAX_ROWS);
    if (x3) {   // the encoder memory as three bf16 planes (the x3 GEMM's A operand)
        GemmParams t = cross_kv_gemm_params(A, e->S, e->dec_layers[0].ckv_w, e->dec_layers[0].ckv_b, ck, cv, kv_esz, B, rows, e->H, e->S, seq_off, row0);
        cross_kv_x3(t, e->enc3, enc_plane, e->dec_layers[0].ckv_w3);
        x3 = gemm_x3_usable(t);
        if (x3) LAUNCH(launch_split3(enc_hidden, e->enc3, enc_plane, enc_plane, s));
    }
    for (int i = 0; i < e->L; ++i) {
        const DecLayerW& l = e->dec_layers[i];
        const size_t layer = (size_t)i * layer_rows * row_bytes;
        GemmParams g = cross_kv_gemm_params(A, e->S, l.ckv_w, l.ckv_b, (char*)ck + layer, (char*)cv + layer, kv_esz, B, rows, e->H, e->S, seq_off, row0);
        if (e->w_half) {
            TIMED(e, e->t_gemm, s, launch_gemm_f16(g, kv_esz == 2, s));
        } else if (x3) {
            cross_kv_x3(g, e->enc3, enc_plane, l.ckv_w3);
            TIMED(e, e->t_gemm, s, launch_gemm_x3(g, s));
        } else {
            int rc = timed_gemm(e, g, s);
            if (rc) return rc;
        }
    }
    return WT_OK;
}

// token-level timestamps: (re)allocate the query history and the post-pass workspace for `B` rows of `max_length - 1` steps and upload the
// per-layer head tables.  The buffer only grows; its layout is recomputed per decode.
static int tt_reserve(wt_engine* e, const StepKey& k, hipStream_t s) {
    const int n = k.tt.n_sel, B = k.tt_rows, steps = k.tt_steps, max_length = k.max_length, S = e->S, ld = tt_trace_ld(S);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    // the head table comes first: its address does not depend on the decode's dimensions
    const size_t o_sel = take((size_t)e->L * e->H * 4), o_qh = take((size_t)n * B * steps * HEAD_DIM * 4), o_W = take((size_t)n * steps * S * 4);
    const size_t o_mean = take((size_t)n * S * 4), o_sdev = take((size_t)n * S * 4), o_mat = take((size_t)B * steps * S * 4);
    const size_t o_tr = take((size_t)B * steps * ld), o_out = take((size_t)B * max_length * 4);
    if (off > e->tt_bytes) {
        HIPCHK(hipStreamSynchronize(s));   // nothing of an earlier decode may still use the old buffer
        if (e->tt_buf) { hipFree(e->tt_buf); e->tt_buf = nullptr; e->tt_bytes = 0; }
        hipError_t he = hipMalloc((void**)&e->tt_buf, off);
        if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for the token-timestamp workspace failed: %s", off, hipGetErrorString(he));
        e->tt_bytes = off;
        e->ws_gen += 1;
        e->tt_h_sel.clear();   // the table moved: whatever lies there is not the table, upload it again
    }
    char* b = e->tt_buf;
    e->tt_qh = (float*)(b + o_qh); e->tt_sel = (int*)(b + o_sel); e->tt_W = (float*)(b + o_W); e->tt_mean = (float*)(b + o_mean); e->tt_sdev = (float*)(b + o_sdev);
    e->tt_matrix = (float*)(b + o_mat); e->tt_trace = (uint8_t*)(b + o_tr); e->tt_out = (float*)(b + o_out);
    std::vector<int> tab((size_t)e->L * e->H, -1);
    for (int i = 0; i < n; ++i) tab[(size_t)k.tt.layer[i] * e->H + k.tt.head[i]] = i;
    if (tab != e->tt_h_sel) {
        e->tt_h_sel.swap(tab);
        HIPCHK(hipMemcpyAsync(e->tt_sel, e->tt_h_sel.data(), e->tt_h_sel.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));   // pageable source
    }
    // a row that is never stepped (a decode read before its first step) must not hand stale queries to the post-pass
    HIPCHK(hipMemsetAsync(e->tt_qh, 0, (size_t)n * B * steps * HEAD_DIM * 4, s));
    return WT_OK;
}

static EngineDims engine_dims(const wt_engine* e) {
    EngineDims dims;
    dims.kind = e->kind; dims.precision = e->precision; dims.d = e->d; dims.H = e->H; dims.L = e->L; dims.F = e->F;
    dims.C = e->C; dims.S = e->S; dims.T = e->T; dims.V = e->V;
    return dims;
}

// the pinned report area of the continuous mode: ids and final lengths per pool row
static int stream_reserve(wt_engine* e, int pool_rows, hipStream_t s) {
    if (pool_rows <= e->h_pool_cap && e->dec_maxlen_cap <= e->h_ml_cap) return WT_OK;
    HIPCHK(hipStreamSynchronize(s));   // no step of an earlier stream may still write the old area
    const int rows = pool_rows > e->h_pool_cap ? pool_rows : e->h_pool_cap;
    if (e->h_ids) { hipHostFree(e->h_ids); e->h_ids = nullptr; }
    if (e->h_len) { hipHostFree(e->h_len); e->h_len = nullptr; }
    e->h_pool_cap = 0;
    HIPCHK(hipHostMalloc((void**)&e->h_ids, (size_t)rows * e->dec_maxlen_cap * 4, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostMalloc((void**)&e->h_len, (size_t)rows * 4, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&e->h_ids_dev, e->h_ids, 0));
    HIPCHK(hipHostGetDevicePointer((void**)&e->h_len_dev, e->h_len, 0));
    e->h_pool_cap = rows;
    e->h_ml_cap = e->dec_maxlen_cap;
    e->ws_gen += 1;   // the step graph carries these addresses
    return WT_OK;
}

// Everything wt_decoder_begin and wt_decoder_stream_begin share: the decode configuration (resolve_decode_config: every check, cache
// policy and key splits), workspace and token-rule tables.  `rows` = utterances of the batch / decode slots of the stream; `pool_rows` =
// cross-cache rows of the stream.  e->cfg changes only when all of it succeeded.
static int decode_setup(wt_engine* e, int rows, const wt_greedy_params* p, int pool_rows, bool stream, hipStream_t s) {
    DecodeFacts f;
    f.w_half = e->w_half; f.kv_esz = e->kv_esz;
    f.no_defer_merge = tuning_env("WT_NO_DEFER_MERGE") != nullptr;
    if (tuning_env("WT_NSPLIT_SELF")) f.nsplit_self = atoi(tuning_env("WT_NSPLIT_SELF"));
    if (tuning_env("WT_NSPLIT_CROSS")) { f.nsplit_cross_set = true; f.nsplit_cross = atoi(tuning_env("WT_NSPLIT_CROSS")); }
    f.beam_cross_grouped = tuning_env("WT_BEAM_CROSS") && !strcmp(tuning_env("WT_BEAM_CROSS"), "grouped");
    DecodeConfig cfg;
    char msg[400] = "";
    int rc = resolve_decode_config(engine_dims(e), f, e->req, p, rows, pool_rows, stream, &cfg, msg, sizeof msg);   // host_logic.cpp
    if (rc) return fail(rc, "%s", msg);
    const StepKey& k = cfg.key;
    rc = dec_reserve(e, k.B, k.max_length, s, cfg.pool_rows);
    if (rc) return rc;
    // token rules -> device tables (SuppressTokens / SuppressTokensAtBegin / ForceTokens; the ids were checked by the resolver).  The
    // host images live in the engine: when the rules are the ones of the previous decode (the usual case: one rule set per checkpoint)
    // nothing is uploaded and the call stays asynchronous; only a CHANGED rule set is uploaded, followed by one stream synchronisation.
    std::vector<uint8_t> mask(e->V, 0);
    for (int i = 0; i < p->n_suppress_tokens; ++i) mask[p->suppress_tokens[i]] |= 1;
    for (int i = 0; i < p->n_begin_suppress_tokens; ++i) mask[p->begin_suppress_tokens[i]] |= 2;
    std::vector<int> forced(e->dec_maxlen_cap + 1, -1);
    for (int i = 0; i < p->n_forced; ++i) {
        const int idx = p->forced_decoder_ids[2 * i];
        if (idx >= 0 && idx <= e->dec_maxlen_cap) forced[idx] = p->forced_decoder_ids[2 * i + 1];
    }
    if (!e->tables_valid || mask != e->h_mask || forced != e->h_forced) {
        e->tables_valid = false;   // a failed upload below must not leave "valid" tables whose host images already hold the new rules
        e->h_mask.swap(mask);
        e->h_forced.swap(forced);
        HIPCHK(hipMemcpyAsync(e->mask, e->h_mask.data(), e->h_mask.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->forced, e->h_forced.data(), e->h_forced.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));  // pageable sources: make sure the copies have left the host images before they can change
        e->tables_valid = true;
    }
    if (k.force_rows_on) {   // bench-only per-row transcript lengths: uploaded (with one synchronisation) only when they change
        std::vector<int> lens(p->force_eos_steps, p->force_eos_steps + k.B);
        if (lens != e->h_force_rows) {
            e->h_force_rows.swap(lens);
            HIPCHK(hipMemcpyAsync(e->force_rows, e->h_force_rows.data(), (size_t)k.B * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    if (k.tt.n_sel > 0 && (rc = tt_reserve(e, k, s))) return rc;   // token-level timestamps: workspace and head tables of this decode
    if (stream && (rc = stream_reserve(e, cfg.pool_rows, s))) return rc;
    e->epoch = e->epoch % 0xffff + 1;   // 1..65535: never the value of a freshly zeroed mailbox
    e->issued = 0;
    e->cfg = cfg;
    return WT_OK;
}

extern "C" int wt_decoder_set_timestamp_rules(wt_engine* e, const wt_timestamp_params* t) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_timestamp_rules: not a decoder engine");
    if (!t || !t->enabled) {
        e->req.ts = wt_timestamp_params{0, 0, 0, 0, 0};
        return WT_OK;
    }
    if (t->timestamp_begin <= 0 || t->timestamp_begin >= e->V)
        return fail(WT_E_INVALID, "wt_decoder_set_timestamp_rules: timestamp_begin %d outside (0, V=%d)", t->timestamp_begin, e->V);
    if (t->no_timestamps_token_id < 0 || t->no_timestamps_token_id >= t->timestamp_begin)
        return fail(WT_E_INVALID, "wt_decoder_set_timestamp_rules: no_timestamps_token_id %d outside [0, timestamp_begin=%d)", t->no_timestamps_token_id, t->timestamp_begin);
    if (t->begin_index < 2) return fail(WT_E_INVALID, "wt_decoder_set_timestamp_rules: begin_index %d < 2 (the prompt holds the start token)", t->begin_index);
    e->req.ts = *t;
    e->req.ts.enabled = 1;
    return WT_OK;
}

extern "C" int wt_decoder_set_beam_search(wt_engine* e, const wt_beam_params* b) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_beam_search: not a decoder engine");
    if (!b || b->num_beams <= 1) {
        e->req.beam = wt_beam_params{1, 1.f, 0};
        return WT_OK;
    }
    if (b->num_beams > MAX_BEAMS) return fail(WT_E_UNSUPPORTED, "wt_decoder_set_beam_search: num_beams %d > %d", b->num_beams, MAX_BEAMS);
    if (b->early_stopping != 0 && b->early_stopping != 1)
        return fail(WT_E_UNSUPPORTED, "wt_decoder_set_beam_search: early_stopping %d (0 or 1; \"never\" is not supported)", b->early_stopping);
    if (!(b->length_penalty == b->length_penalty) || fabsf(b->length_penalty) > 1e3f)
        return fail(WT_E_INVALID, "wt_decoder_set_beam_search: length_penalty %g", (double)b->length_penalty);
    e->req.beam = *b;
    return WT_OK;
}

extern "C" int wt_decoder_set_token_timestamps(wt_engine* e, const wt_token_timestamp_params* t) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: not a decoder engine");
    if (!t || t->n_heads <= 0) {
        e->req.tt = DecodeRequest::TokTs{};
        return WT_OK;
    }
    if (t->n_heads > TT_MAX_HEADS) return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: %d alignment heads > %d", t->n_heads, TT_MAX_HEADS);
    if (!t->heads) return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: null head list");
    if (t->median_filter_width < 1 || t->median_filter_width > TT_MAX_WIDTH || !(t->median_filter_width & 1))
        return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: median_filter_width %d (odd, 1 .. %d)", t->median_filter_width, TT_MAX_WIDTH);
    if (!(t->time_precision > 0.0) || !(t->time_precision < 1e6))
        return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: time_precision %g", t->time_precision);
    DecodeRequest::TokTs tt;
    tt.n_sel = t->n_heads; tt.width = t->median_filter_width; tt.time_precision = t->time_precision;
    for (int i = 0; i < t->n_heads; ++i) {
        const int l = t->heads[2 * i], h = t->heads[2 * i + 1];
        if (l < 0 || l >= e->L || h < 0 || h >= e->H)
            return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: alignment head (%d, %d) outside %d layers x %d heads", l, h, e->L, e->H);
        for (int j = 0; j < i; ++j)
            if (tt.layer[j] == l && tt.head[j] == h) return fail(WT_E_INVALID, "wt_decoder_set_token_timestamps: alignment head (%d, %d) listed twice", l, h);
        tt.layer[i] = l; tt.head[i] = h;
    }
    e->req.tt = tt;
    return WT_OK;
}

extern "C" int wt_decoder_set_logprobs(wt_engine* e, const wt_logprob_params* p) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_logprobs: not a decoder engine");
    if (!p || !p->enabled) {
        e->req.lp = wt_logprob_params{0, -1};
        return WT_OK;
    }
    if (p->no_speech_token_id < -1 || p->no_speech_token_id >= e->V)
        return fail(WT_E_INVALID, "wt_decoder_set_logprobs: no_speech_token_id %d outside [-1, V=%d)", p->no_speech_token_id, e->V);
    e->req.lp = wt_logprob_params{1, p->no_speech_token_id};
    return WT_OK;
}

extern "C" int wt_decoder_set_sampling(wt_engine* e, const wt_sampling_params* p) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_sampling: not a decoder engine");
    if (p && !(fabsf(p->temperature) <= 3.4028235e38f)) return fail(WT_E_INVALID, "wt_decoder_set_sampling: temperature is not finite");
    if (!p || !(p->temperature > 0.f)) {
        e->req.samp_temp = 0.f;
        e->req.samp_list = false;
        e->req.samp_seeds.clear();
        return WT_OK;
    }
    if (p->seeds && p->n_seeds < 1) return fail(WT_E_INVALID, "wt_decoder_set_sampling: a seed list of %d entries", p->n_seeds);
    e->req.samp_temp = p->temperature;
    e->req.samp_seed = p->seed;
    e->req.samp_list = p->seeds != nullptr;
    e->req.samp_seeds.clear();
    if (p->seeds) e->req.samp_seeds.assign(p->seeds, p->seeds + p->n_seeds);
    return WT_OK;
}

extern "C" int wt_decoder_set_prompt(wt_engine* e, const wt_prompt_params* p) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_prompt: not a decoder engine");
    if (!p || p->len <= 0) {
        e->req.prompt.clear();
        e->req.prompt_lens.clear();
        e->req.prompt_rows = e->req.prompt_len = 0;
        return WT_OK;
    }
    if (!p->ids || p->n_rows < 1) return fail(WT_E_INVALID, "wt_decoder_set_prompt: null ids or %d rows", p->n_rows);
    if (p->len >= e->T) return fail(WT_E_INVALID, "wt_decoder_set_prompt: %d prompt tokens >= max_target_positions %d", p->len, e->T);
    const size_t n = (size_t)p->n_rows * p->len;
    for (size_t i = 0; i < n; ++i)
        if (p->ids[i] < 0 || p->ids[i] >= e->V)
            return fail(WT_E_INVALID, "wt_decoder_set_prompt: token %d (row %zu, position %zu) outside the vocabulary", p->ids[i], i / p->len, i % p->len);
    e->req.prompt.assign(p->ids, p->ids + n);
    e->req.prompt_rows = p->n_rows;
    e->req.prompt_len = p->len;
    e->req.prompt_lens.clear();
    return WT_OK;
}

extern "C" int wt_decoder_set_prompt_rows(wt_engine* e, const int32_t* ids, int n_rows, int ld, const int32_t* lens) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_prompt_rows: not a decoder engine");
    int lmax = 0;
    if (ids && lens) {
        if (n_rows < 1 || ld < 1) return fail(WT_E_INVALID, "wt_decoder_set_prompt_rows: %d rows of leading dimension %d", n_rows, ld);
        for (int b = 0; b < n_rows; ++b) {
            if (lens[b] < 0 || lens[b] > ld) return fail(WT_E_INVALID, "wt_decoder_set_prompt_rows: row %d holds %d tokens, outside [0, %d]", b, lens[b], ld);
            lmax = lens[b] > lmax ? lens[b] : lmax;
        }
    }
    if (lmax == 0) {
        e->req.prompt.clear();
        e->req.prompt_lens.clear();
        e->req.prompt_rows = e->req.prompt_len = 0;
        return WT_OK;
    }
    if (lmax >= e->T) return fail(WT_E_INVALID, "wt_decoder_set_prompt_rows: %d prompt tokens >= max_target_positions %d", lmax, e->T);
    for (int b = 0; b < n_rows; ++b)
        for (int j = 0; j < lens[b]; ++j) {
            const int tok = ids[(size_t)b * ld + j];
            if (tok < 0 || tok >= e->V) return fail(WT_E_INVALID, "wt_decoder_set_prompt_rows: token %d (row %d, position %d) outside the vocabulary", tok, b, j);
        }
    e->req.prompt.assign((size_t)n_rows * lmax, 0);   // [n_rows][lmax]; what lies behind a row's tokens is never read
    for (int b = 0; b < n_rows; ++b) memcpy(e->req.prompt.data() + (size_t)b * lmax, ids + (size_t)b * ld, (size_t)lens[b] * 4);
    e->req.prompt_lens.assign(lens, lens + n_rows);
    e->req.prompt_rows = n_rows;
    e->req.prompt_len = lmax;
    return WT_OK;
}

extern "C" int wt_decoder_set_languages(wt_engine* e, const int32_t* lang_ids, int n_lang, const int32_t* row_tok, int n_rows) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_set_languages: not a decoder engine");
    if (n_lang <= 0 || !lang_ids) {
        e->req.lang_ids.clear();
        e->req.lang_rows.clear();
        return WT_OK;
    }
    if (n_lang > LANG_MAX) return fail(WT_E_INVALID, "wt_decoder_set_languages: %d language ids > %d", n_lang, LANG_MAX);
    if (row_tok && n_rows < 1) return fail(WT_E_INVALID, "wt_decoder_set_languages: a row table of %d entries", n_rows);
    e->req.lang_ids.assign(lang_ids, lang_ids + n_lang);   // (the ids themselves are checked against the next decode's rules: resolve_decode_config)
    e->req.lang_rows.clear();
    if (row_tok) e->req.lang_rows.assign(row_tok, row_tok + n_rows);
    return WT_OK;
}

extern "C" int wt_decoder_read_languages(wt_engine* e, int32_t* tok, float* prob, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.n_lang == 0)
        return fail(WT_E_STATE, "wt_decoder_read_languages: no decode with per-row language tokens in flight (wt_decoder_set_languages, then wt_decoder_begin)");
    if (!tok && !prob) return fail(WT_E_INVALID, "wt_decoder_read_languages: null outputs");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    if (tok) HIPCHK(hipMemcpyAsync(tok, e->lang_tok, (size_t)e->cfg.key.B * 4, hipMemcpyDeviceToDevice, s));
    if (prob) HIPCHK(hipMemcpyAsync(prob, e->lang_prob, (size_t)e->cfg.key.B * e->cfg.key.n_lang * 4, hipMemcpyDeviceToDevice, s));
    return WT_OK;
}

// The prefill (DESIGN.md "Decoder prompts"): positions 0..len-1 of all B rows through the decoder layers in one pass over M = B * len rows
// (utterance-major), leaving their keys and values in rows 0..len-1 of the resident self caches.  The kernels are the encoder's
// (launch_layernorm, launch_gemm_f32) and kernels_prefill.hip's; the cross K/V of this decode must be enqueued on `s` before.  The last
// layer stops behind its k|v projection: nothing reads a prompt position's output (no vocabulary projection runs for it).
static int prefill_reserve(wt_engine* e, int B, int len, hipStream_t s, float** bufs, int** ids_dev) {
    const size_t M = (size_t)B * len, d = e->d;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    // h, h1, x, q: [M][d]; ah: [M][2d] (self-attention context | layer input); ffn: [M][F]; the prompt ids
    const size_t o_h = take(M * d * 4), o_h1 = take(M * d * 4), o_x = take(M * d * 4), o_q = take(M * d * 4), o_ah = take(M * 2 * d * 4);
    const size_t o_f = take(M * e->F * 4), o_ids = take(((size_t)MAX_ROWS * e->T + MAX_ROWS) * 4);   // (+ the per-row lengths of the ragged form)
    if (off > e->pf_bytes) {
        HIPCHK(hipStreamSynchronize(s));   // nothing of an earlier decode may still use the old buffer
        if (e->pf_ws) { hipFree(e->pf_ws); e->pf_ws = nullptr; e->pf_bytes = 0; }
        hipError_t he = hipMalloc((void**)&e->pf_ws, off);
        if (he != hipSuccess) return fail(WT_E_NOMEM, "hipMalloc(%zu) for the prompt prefill workspace failed: %s", off, hipGetErrorString(he));
        e->pf_bytes = off;
    }
    char* b = e->pf_ws;
    bufs[0] = (float*)(b + o_h); bufs[1] = (float*)(b + o_h1); bufs[2] = (float*)(b + o_x); bufs[3] = (float*)(b + o_q);
    bufs[4] = (float*)(b + o_ah); bufs[5] = (float*)(b + o_f);
    *ids_dev = (int*)(b + o_ids);
    return WT_OK;
}

static int enqueue_prefill(wt_engine* e, int B, int len, float* const* bufs, const int* ids_dev, int n_rows, hipStream_t s) {
    const int d = e->d, H = e->H, M = B * len;
    float *h = bufs[0], *h1 = bufs[1], *x = bufs[2], *q = bufs[3], *ah = bufs[4], *ffn = bufs[5];
    int rc;
    auto dense = [&](const float* A, int lda, int K, const float* Wt, const float* bias, int N, float* Cout, int act, const float* resid) {
        GemmParams g;
        memset(&g, 0, sizeof g);
        g.A = A; g.lda = lda; g.a_rows_per_batch = M; g.W = Wt; g.bias = bias; g.M = M; g.N = N; g.K = K; g.act = act;
        g.C = Cout; g.ldc = N; g.c_rows_per_batch = M; g.resid = resid;
        return timed_gemm(e, g, s);
    };
    LAUNCH(launch_prefill_embed(ids_dev, n_rows, len, e->tok_emb, e->pos_emb, h, B, d, s));
    for (int i = 0; i < e->L; ++i) {
        const DecLayerW& l = e->dec_layers[i];
        const size_t self_layer = (size_t)i * B * H * e->T * HEAD_DIM, cross_layer = (size_t)i * e->cross_rows * H * e->S * HEAD_DIM;
        float *sk = e->self_k + self_layer, *sv = e->self_v + self_layer;
        LAUNCH(launch_layernorm(h, l.ln1_w, l.ln1_b, x, M, d, s));
        {   // k|v: rows [d, 3d) of qkv_w, split by head straight into cache rows [0, len) of every utterance (the cross-K/V projection's epilogue)
            GemmParams g = cross_kv_gemm_params(x, len, l.qkv_w + (size_t)d * d, l.qkv_b + d, sk, sv, 4, B, len, H, e->T, 0, 0);
            if ((rc = timed_gemm(e, g, s))) return rc;
        }
        if (i == e->L - 1) break;
        if ((rc = dense(x, d, d, l.qkv_w, l.qkv_b, d, q, 0, nullptr))) return rc;
        PrefillAttnParams a;
        memset(&a, 0, sizeof a);
        a.q = q; a.k = sk; a.v = sv; a.ctx = ah; a.B = B; a.H = H; a.nq = len; a.nk = len; a.cap = e->T; a.ldq = d; a.ldc = 2 * d;
        a.causal = 1; a.q_scale = 0.125f;
        LAUNCH(launch_prefill_attention(a, s));
        // [a ; h] side by side: the folded query multiplies both (the blob holds fold_w as one [d][2d] matrix)
        HIPCHK(hipMemcpy2DAsync(ah + d, (size_t)2 * d * 4, h, (size_t)d * 4, (size_t)d * 4, M, hipMemcpyDeviceToDevice, s));
        if ((rc = dense(ah, 2 * d, d, l.o_w, l.o_b, d, h1, 0, h))) return rc;                       // h1 = h + Wo.a + bo
        if ((rc = dense(ah, 2 * d, 2 * d, l.fold_w, l.fold_c, d, q, 0, nullptr))) return rc;        // u = fold_w.[a ; h] + fold_c
        LAUNCH(launch_prefill_query_finish(q, h1, l.fold_r, l.fold_t, q, M, d, s));
        memset(&a, 0, sizeof a);
        a.q = q; a.k = e->cross_k + cross_layer; a.v = e->cross_v + cross_layer; a.ctx = x; a.B = B; a.H = H; a.nq = len; a.nk = e->S; a.cap = e->S;
        a.ldq = d; a.ldc = d; a.causal = 0; a.q_scale = 1.f;
        LAUNCH(launch_prefill_attention(a, s));
        if ((rc = dense(x, d, d, l.co_w, l.co_b, d, h1, 0, h1))) return rc;
        LAUNCH(launch_layernorm(h1, l.ln3_w, l.ln3_b, x, M, d, s));
        if ((rc = dense(x, d, d, l.fc1_w, l.fc1_b, e->F, ffn, 1, nullptr))) return rc;
        if ((rc = dense(ffn, e->F, e->F, l.fc2_w, l.fc2_b, d, h1, 0, h1))) return rc;
        std::swap(h, h1);
    }
    return WT_OK;
}

static void fill_select_params(wt_engine* e, SelectParams& sp);

extern "C" int wt_decoder_begin(wt_engine* e, const float* enc_hidden, int B, const wt_greedy_params* p, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_begin: not a decoder engine");
    if (!enc_hidden || !p || B < 1) return fail(WT_E_INVALID, "wt_decoder_begin: bad arguments");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    int rc = decode_setup(e, B, p, 0, false, s);
    if (rc) return rc;
    const DecodeConfig& c = e->cfg;
    const StepKey& k = c.key;
    B = k.B;   // beam search: the utterances decode as U * num_beams rows, [utterance][beam]
    if (k.samp_temp > 0.f) {   // (pageable sources kept alive by the handle: the copy below may read them later)
        if (!e->req.samp_list) {
            e->h_seeds.resize(B);
            for (int b = 0; b < B; ++b) e->h_seeds[b] = e->req.samp_seed + (unsigned long long)b;
        }
        const std::vector<unsigned long long>& h = e->req.samp_list ? e->req.samp_seeds : e->h_seeds;
        HIPCHK(hipMemcpyAsync(e->samp_seeds, h.data(), (size_t)B * 8, hipMemcpyHostToDevice, s));
    }
    if (k.lp.enabled) {   // position 0, the positions behind an EOS and the sums start at zero
        HIPCHK(hipMemsetAsync(e->lp_tok, 0, (size_t)B * k.max_length * 4, s));
        HIPCHK(hipMemsetAsync(e->lp_sum, 0, (size_t)B * 4, s));
        HIPCHK(hipMemsetAsync(e->lp_nsp, 0, (size_t)B * 4, s));
        HIPCHK(hipMemsetAsync(e->lp_side, 0, (size_t)B * 2 * 4, s));
    }
    if (k.n_lang > 0) {   // the rows' language tokens (-1: lang_select_kernel fills it in the first step) and the listed ids
        e->h_lang.assign(MAX_ROWS + LANG_MAX, -1);
        memcpy(e->h_lang.data(), c.lang_rows, (size_t)B * 4);
        memcpy(e->h_lang.data() + MAX_ROWS, c.lang_ids, (size_t)k.n_lang * 4);
        HIPCHK(hipMemcpyAsync(e->lang_tok, e->h_lang.data(), e->h_lang.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(e->lang_prob, 0, (size_t)B * k.n_lang * 4, s));   // (rows all chosen by the caller: no kernel runs, the probabilities read 0)
    }
    LAUNCH(launch_dec_init(e->st, e->ids, e->unfinished, B, k.max_length, k.start_token, e->epoch, s));
    if (k.beam.num_beams > 1) {
        SelectParams sp;
        fill_select_params(e, sp);
        LAUNCH(launch_beam_init(sp, s));
    }
    const int plen = c.prompt_len;
    float* pf_bufs[6];
    int* pf_ids = nullptr;
    if (plen > 0) {   // the prompt's ids and the state behind it; the step-0 input below is then the start token at position plen
        rc = prefill_reserve(e, B, plen, s, pf_bufs, &pf_ids);
        if (rc) return rc;
        // (pageable source kept alive by the handle, as the sampling seeds above)
        if (c.prompt_ragged) {   // the pass's own id matrix [B][plen]: the rows' tokens, right-padded with the pad id; the lengths ride behind it
            e->h_prompt.assign((size_t)B * plen + MAX_ROWS, k.pad);
            for (int b = 0; b < B; ++b) {
                memcpy(e->h_prompt.data() + (size_t)b * plen, e->req.prompt.data() + (size_t)b * e->req.prompt_len, (size_t)c.prompt_lens[b] * 4);
                e->h_prompt[(size_t)B * plen + b] = c.prompt_lens[b];
            }
            HIPCHK(hipMemcpyAsync(pf_ids, e->h_prompt.data(), ((size_t)B * plen + MAX_ROWS) * 4, hipMemcpyHostToDevice, s));
            LAUNCH(launch_prefill_state_rows(e->st, e->ids, pf_ids, pf_ids + (size_t)B * plen, plen, B, k.max_length, k.start_token, k.pad, s));
        } else {
            HIPCHK(hipMemcpyAsync(pf_ids, e->req.prompt.data(), (size_t)c.prompt_rows * plen * 4, hipMemcpyHostToDevice, s));
            LAUNCH(launch_prefill_state(e->st, e->ids, pf_ids, c.prompt_rows, plen, B, k.max_length, k.start_token, s));
        }
    }
    LAUNCH(launch_dec_embed(e->ids, k.max_length, e->tok_emb, e->pos_emb, e->dh, B, e->d, e->st, s, e->w_half));  // input of step 0
    // the beams of an utterance attend over the same encoder memory: its cross K/V are projected once, into cache row u
    rc = cross_kv_project(e, enc_hidden, c.U, e->S, 0, e->cross_k, e->cross_v, e->kv_esz, s, e->cross_rows, 0);
    if (rc) return rc;
    if (plen > 0) {   // behind the cross K/V projection: the prefill's cross attention reads this decode's cross caches
        rc = enqueue_prefill(e, B, plen, pf_bufs, pf_ids, c.prompt_rows, s);
        if (rc) return rc;
    }
    e->begun = true;
    return WT_OK;
}

static void fill_select_params(wt_engine* e, SelectParams& sp) {
    const StepKey& k = e->cfg.key;
    greedy_select_params(sp, e->logits, e->mask, e->forced, e->ids, e->unfinished, e->st, k.logits_trace, e->sel_val, e->sel_idx, e->tok_emb, e->pos_emb,
                         e->dh, e->d, e->w_half, k.B, e->V, k.max_length, k.begin_index, k.eos, k.pad, k.force_eos_step,
                         k.force_rows_on ? e->force_rows : nullptr, e->mailbox_dev, k.start_token);
    if (k.ts.enabled) {
        sp.ts_on = 1; sp.no_ts = k.ts.no_timestamps_token_id; sp.tb = k.ts.timestamp_begin;
        sp.ts_begin_index = k.ts.begin_index; sp.max_init = k.ts.max_initial_timestamp_index; sp.ts_part = e->ts_part;
    }
    if (k.beam.num_beams > 1) {
        sp.beam_on = 1; sp.beam = e->beam_dev;
        sp.beam.nb = k.beam.num_beams; sp.beam.U = e->cfg.U; sp.beam.length_penalty = k.beam.length_penalty;
        sp.beam.early_stopping = k.beam.early_stopping;
    }
    if (k.lp.enabled) {
        sp.lp_on = 1; sp.lp_ns = k.lp.no_speech_token_id; sp.lp_part = e->lp_part; sp.lp_side = e->lp_side; sp.lp_tok = e->lp_tok;
        sp.lp_sum = e->lp_sum; sp.lp_nsp = e->lp_nsp;
        if (k.samp_temp > 0.f) {
            sp.samp_on = 1; sp.samp_temp = k.samp_temp; sp.samp_seeds = e->samp_seeds; sp.samp_sc = e->samp_sc; sp.samp_ts = e->samp_ts;
            sp.samp_K = e->d; sp.samp_parts_cap = SEL_PARTS_CAP;
        }
    }
    if (k.lang_pos > 0) { sp.lang_pos = k.lang_pos; sp.lang_tok = e->lang_tok; }
    if (e->cfg.stream) {
        sp.stream = 1; sp.host_ids = e->h_ids_dev; sp.host_len = e->h_len_dev; sp.force_eos_step = -1;
    }
}

// the StepIO of one step of the decode in flight over the resident caches.  variant bit 0: finished / idle rows stream no K/V (`alive`);
// bit 1: the continuous mode's graph (per-slot cross-cache rows and state); bit 2: the first step of a decode that detects languages
static StepIO step_io(const wt_engine* e, int variant) {
    const StepKey& k = e->cfg.key;
    StepIO io;
    io.alive = (variant & 1) ? e->unfinished : nullptr;
    io.ids = e->ids; io.ids_ld = k.max_length; io.self_k = e->self_k; io.self_v = e->self_v; io.self_cap = e->T;
    io.cross_k = e->cross_k; io.cross_v = e->cross_v; io.cross_rows = e->cross_rows; io.logits = e->logits; io.B = k.B; io.kv_esz = e->kv_esz;
    io.slot_row = (variant & 2) ? e->st->slot_row : nullptr;   // (address arithmetic on a device pointer: nothing is dereferenced here)
    if (k.beam.num_beams > 1) { io.slot_row = e->beam_dev.urow; io.anc = e->beam_dev.anc; io.anc_ld = e->beam_dev.anc_ld; io.group = k.beam_group; }
    if (k.tt.n_sel > 0) { io.qh = e->tt_qh; io.qh_sel = e->tt_sel; io.qh_rows = k.tt_rows; io.qh_steps = k.tt_steps; }
    io.nsplit_self = k.nsplit_self; io.nsplit_cross = k.nsplit_cross; io.nt = k.nt_loads;
    io.embed = false;  // dh already holds this step's input: written by wt_decoder_begin (step 0) or by the previous greedy_finish
    io.argmax = nullptr; io.argmax_parts = nullptr;
    io.lang = (variant & 4) != 0;
    return io;
}

static int enqueue_fast_step(wt_engine* e, hipStream_t s, int variant = 0) {
    StepIO io = step_io(e, variant);
    static const bool fuse = tuning_env("WT_NO_FUSED_ARGMAX") == nullptr;  // A/B switch: logits to HBM + greedy_select_kernel
    SelectParams sp;
    fill_select_params(e, sp);
    const bool fused = fuse && !sp.ts_on && !sp.beam_on;   // timestamp mode / beam search: plain logits to HBM, then their select kernels
    int parts = 0;
    io.argmax = fused ? &sp : nullptr;
    io.argmax_parts = &parts;
    int rc = enqueue_step(e, io, s);
    if (rc) return rc;
    if (fused) greedy_select_fused(sp, parts);
    LAUNCH(launch_greedy_select(sp, s));
    return WT_OK;
}

// Captures and instantiations are rare (once per engine and decode configuration) and serialised process-wide: several host threads
// drive their own handles concurrently (runtime.WhisperPipeline), and a multi-worker run under rocprofv3 aborted inside the runtime
// while captures overlapped.  Replays (hipGraphLaunch) stay concurrent.  (What that does and does not explain of the round-3 abort:
// DESIGN.md "The four-worker abort under rocprofv3".)
static std::mutex g_capture_mutex;

// enqueue n_steps decoder steps on `s` (the caller holds the device guard).  variant 1: the step graph in which finished rows stream
// no K/V (wt_decoder_run switches to it once the mailbox reports a finished row; never with a logits trace, which records every
// row's logits at every step as the reference computes them).  The continuous mode replays variants 2 / 3.
static int enqueue_steps(wt_engine* e, int n_steps, hipStream_t s, int variant = 0) {
    if (e->cfg.lang_detect && e->issued == 0 && n_steps > 0 && !(variant & 4)) {   // the first step behind wt_decoder_begin detects the languages:
        const int rc = enqueue_steps(e, 1, s, variant | 4);                            // its own graph; every later step is what it is without the mode
        if (rc || n_steps == 1) return rc;
        n_steps -= 1;
    }
    StepKey k = e->cfg.key;
    k.workspace_gen = e->ws_gen;   // as it stands NOW: a (re)allocation behind the last begin must not replay graphs into freed memory
    const int lang_bit = variant & 4;
    variant &= 3;
    if (k.logits_trace || k.beam.num_beams > 1) variant = 0;   // (beam search: one graph; a finished utterance's rows keep attending)
    if (k.tt.n_sel > 0) variant = 0;   // token-level timestamps: finished rows keep stepping on pad input, their steps are part of the alignment
    if (e->cfg.stream) variant |= 2;
    variant |= lang_bit;
    if (e->profiling || !e->use_graph) {  // eager: per-kernel event timers need real launches
        for (int i = 0; i < n_steps; ++i) {
            int rc = enqueue_fast_step(e, s, variant);
            if (rc) return rc;
            e->issued += 1;
        }
        return WT_OK;
    }
    // The step graph is CAPTURED on the engine's own stream (the caller's may be the NULL stream, which cannot be captured;
    // capturing executes nothing) and REPLAYED on the caller's stream: a replay on a second stream measured 5 % slower
    // per step (1.69 vs 1.60 ms, medium.en B=8) than on the stream the rest of the pass already runs on.
    if (k != e->graph_key) {   // the graphs bake in exactly what the key holds (host_logic.h: StepKey)
        for (int v = 0; v < wt_engine::N_GRAPHS; ++v) {
            if (e->graph_exec[v]) { hipGraphExecDestroy(e->graph_exec[v]); e->graph_exec[v] = nullptr; }
            if (e->graph[v]) { hipGraphDestroy(e->graph[v]); e->graph[v] = nullptr; }
            e->graph_ok[v] = false;
        }
        e->graph_key = k;
    }
    if (!e->graph_ok[variant]) {
        std::lock_guard<std::mutex> lock(g_capture_mutex);
        if (e->graph[variant]) { hipGraphDestroy(e->graph[variant]); e->graph[variant] = nullptr; }   // left by a failed attempt
        HIPCHK(hipStreamBeginCapture(e->own_stream, hipStreamCaptureModeThreadLocal));
        int rc = enqueue_fast_step(e, e->own_stream, variant);
        hipError_t ce = hipStreamEndCapture(e->own_stream, &e->graph[variant]);
        if (rc != WT_OK || ce != hipSuccess) {
            if (e->graph[variant]) { hipGraphDestroy(e->graph[variant]); e->graph[variant] = nullptr; }
            return rc != WT_OK ? rc : fail(WT_E_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
        }
        const hipError_t ie = hipGraphInstantiate(&e->graph_exec[variant], e->graph[variant], nullptr, nullptr, 0);
        if (ie != hipSuccess) {
            hipGraphDestroy(e->graph[variant]);
            e->graph[variant] = nullptr;
            e->graph_exec[variant] = nullptr;
            return fail(WT_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
        }
        e->graph_ok[variant] = true;
        e->graph_captures += 1;
    }
    for (int i = 0; i < n_steps; ++i) {
        HIPCHK(hipGraphLaunch(e->graph_exec[variant], s));
        e->issued += 1;   // counted only once it is really in the queue: wt_decoder_run compares it with the steps the mailbox reports
    }
    return WT_OK;
}

// ------------------------------------------------------------------------------------------------- continuous decoding
// The reference transcribes one clip at a time, so every utterance stops at its own EOS (run.py:219-226; dataset loop cal_wer.py:249-287).
// A batch started by wt_decoder_begin runs to its LONGEST row.  The continuous mode keeps `slots` rows busy instead: utterances are
// SUBMITTED (their cross K/V projected into a free row of a cache pool, any number ahead of time), wait in a device queue, and the
// kernel that sees a row stop puts the next waiting utterance into that slot in the same step -- no finished row is ever stepped, no
// host round trip sits between an EOS and the next utterance's first token.  Finished utterances report through pinned host memory.
extern "C" int wt_decoder_stream_begin(wt_engine* e, int slots, int pool_rows, const wt_greedy_params* p, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_stream_begin: not a decoder engine");
    if (!p || slots < 1) return fail(WT_E_INVALID, "wt_decoder_stream_begin: bad arguments");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    int rc = decode_setup(e, slots, p, pool_rows, true, s);
    if (rc) return rc;
    pool_rows = e->cfg.pool_rows;
    e->pool_state.assign(pool_rows, 0);
    e->submitted = e->finished_seen = e->admitted_seen = 0;
    for (int r = 0; r < pool_rows; ++r) __atomic_store_n(e->h_len + r, 0, __ATOMIC_RELAXED);
    LAUNCH(launch_stream_init(e->st, e->unfinished, slots, e->epoch, s));
    e->begun = true;
    return WT_OK;
}

extern "C" int wt_decoder_stream_submit(wt_engine* e, const float* enc_hidden, int n, const int32_t* force_eos_steps, int32_t* handles,
                                        void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || !e->cfg.stream) return fail(WT_E_STATE, "wt_decoder_stream_submit: no stream open (wt_decoder_stream_begin)");
    if (!enc_hidden || !handles || n < 1 || n > MAX_ROWS) return fail(WT_E_INVALID, "wt_decoder_stream_submit: 1 .. %d utterances per call", MAX_ROWS);
    if (e->submitted - e->admitted_seen + n > STREAM_QCAP) return fail(WT_E_STATE, "wt_decoder_stream_submit: waiting queue full");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    // pool rows for the n utterances: as few contiguous runs as the free list allows (one batched K/V projection per run and layer)
    std::vector<int> rows;
    for (int r = 0; r < e->cfg.pool_rows && (int)rows.size() < n; ++r)
        if (e->pool_state[r] == 0) rows.push_back(r);
    if ((int)rows.size() < n) return fail(WT_E_STATE, "wt_decoder_stream_submit: %d free cache rows for %d utterances (collect finished ones first)", (int)rows.size(), n);
    StreamPublish pub;
    memset(&pub, 0, sizeof pub);
    pub.n = n;
    for (int i = 0; i < n; ++i) {
        pub.rows[i] = rows[i];
        pub.force[i] = force_eos_steps ? force_eos_steps[i] : -1;
        handles[i] = rows[i];
    }
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && rows[j] == rows[j - 1] + 1) ++j;
        const int rc = cross_kv_project(e, enc_hidden + (size_t)i * e->S * e->d, j - i, e->S, 0, e->cross_k, e->cross_v, e->kv_esz, s, e->cross_rows, rows[i]);
        if (rc) return rc;
        i = j;
    }
    for (int i = 0; i < n; ++i) {
        __atomic_store_n(e->h_len + rows[i], 0, __ATOMIC_RELAXED);   // (the row is free: no kernel writes it before the publish below)
        e->pool_state[rows[i]] = 1;
    }
    SelectParams sp;
    fill_select_params(e, sp);
    LAUNCH(launch_stream_publish(sp, pub, s));
    e->submitted += n;
    return WT_OK;
}

// newly finished utterances (their pinned length word has become non-zero): state 1 -> 2
static int stream_scan_finished(wt_engine* e) {
    int n = 0;
    for (int r = 0; r < e->cfg.pool_rows; ++r)
        if (e->pool_state[r] == 1 && __atomic_load_n(e->h_len + r, __ATOMIC_ACQUIRE) != 0) {
            e->pool_state[r] = 2;
            ++n;
        }
    e->finished_seen += n;
    return n;
}

// Steps until (a) every submitted utterance has finished, or (b) fewer than `min_waiting` submitted utterances are still waiting for a
// slot (min_waiting > 0: the caller has more to submit and wants the queue topped up).  Follows the mailbox like wt_decoder_run.
extern "C" int wt_decoder_stream_run(wt_engine* e, int min_waiting, int lookahead, int* n_finished, int* n_waiting, int* n_steps, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || !e->cfg.stream) return fail(WT_E_STATE, "wt_decoder_stream_run: no stream open (wt_decoder_stream_begin)");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    if (lookahead <= 0) lookahead = e->cfg.key.nt_loads ? 1 : 3;
    if (lookahead > 64) lookahead = 64;
    int spins = 0, slices = 0;
    unsigned long long last = ~0ull;
    for (;;) {
        const unsigned long long mb = __atomic_load_n(e->mailbox, __ATOMIC_ACQUIRE);
        const bool mine = (int)(mb >> 48) == e->epoch;
        const int retired = mine ? e->issued - (int)((unsigned)(e->issued - (int)((mb >> 32) & 0xffff)) & 0xffffu) : 0;
        if (mine) {   // admitted utterances: the word carries the low 15 bits of the device's count
            const int adm = (int)((mb >> 16) & 0x7fff);
            e->admitted_seen += (int)((unsigned)(adm - e->admitted_seen) & 0x7fffu);
            if (e->admitted_seen > e->submitted) e->admitted_seen = e->submitted;
        }
        if (mb != last) {
            last = mb;
            stream_scan_finished(e);
        }
        const int waiting_ub = e->submitted - e->admitted_seen;   // upper bound: admissions by the publish kernel show up with the next step's word
        if (e->finished_seen >= e->submitted) break;
        if (min_waiting > 0 && waiting_ub < min_waiting) break;
        if (e->issued - retired <= lookahead) {
            // idle slots with nothing waiting (the tail of the workload): the graph whose attention skips them
            const unsigned full = (1u << e->cfg.key.B) - 1u;
            const int variant = (mine && retired > 0 && ((unsigned)mb & 0xffffu) != full && waiting_ub == 0) ? 1 : 0;
            const int rc = enqueue_steps(e, 1, s, variant);
            if (rc) return rc;
            spins = slices = 0;
            continue;
        }
        if (spins < 2000) {
            ++spins;
            __builtin_ia32_pause();
            continue;
        }
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
        if (++slices % 64 == 0) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(WT_E_HIP, "wt_decoder_stream_run: stream failed: %s", hipGetErrorString(q));
            if (q == hipSuccess && slices > 4096) {
                stream_scan_finished(e);
                if (e->finished_seen >= e->submitted) break;
                const unsigned long long m2 = __atomic_load_n(e->mailbox, __ATOMIC_ACQUIRE);
                if (m2 == mb) return fail(WT_E_STATE, "wt_decoder_stream_run: idle stream, %d of %d utterances finished", e->finished_seen, e->submitted);
            }
        }
    }
    if (n_finished) *n_finished = e->finished_seen;
    if (n_waiting) *n_waiting = e->submitted - e->admitted_seen;
    if (n_steps) *n_steps = e->issued;
    return WT_OK;
}

// Finished utterance `handle` (from wt_decoder_stream_submit): *len = its length (start token and EOS included), 0 while it is still
// waiting or decoding (ids_out untouched).  With ids_out != NULL a finished utterance's ids are copied to HOST memory (capacity `cap`
// >= max_length int32) and its cache row is released for the next submit.
extern "C" int wt_decoder_stream_collect(wt_engine* e, int handle, int32_t* ids_out, int cap, int* len) {
    if (!e || e->kind != WT_KIND_DECODER || !e->cfg.stream) return fail(WT_E_STATE, "wt_decoder_stream_collect: no stream open");
    if (handle < 0 || handle >= e->cfg.pool_rows || !len) return fail(WT_E_INVALID, "wt_decoder_stream_collect: bad handle %d", handle);
    if (e->pool_state[handle] == 0) return fail(WT_E_STATE, "wt_decoder_stream_collect: row %d holds no utterance", handle);
    const int n = __atomic_load_n(e->h_len + handle, __ATOMIC_ACQUIRE);
    *len = n;
    if (n == 0 || !ids_out) return WT_OK;
    if (cap < n) return fail(WT_E_INVALID, "wt_decoder_stream_collect: %d ids, capacity %d", n, cap);
    if (e->pool_state[handle] == 1) { e->pool_state[handle] = 2; e->finished_seen += 1; }
    memcpy(ids_out, e->h_ids + (size_t)handle * e->cfg.key.max_length, (size_t)n * 4);   // row stride of stream_finish_kernel: this stream's max_length
    e->pool_state[handle] = 0;
    return WT_OK;
}

extern "C" int wt_decoder_steps(wt_engine* e, int n_steps, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_steps: not a decoder engine");
    if (!e->begun) return fail(WT_E_STATE, "wt_decoder_steps called before wt_decoder_begin");
    if (n_steps <= 0) return WT_OK;
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    return enqueue_steps(e, n_steps, (hipStream_t)stream);
}

// Run the decode in flight to its stop test WITHOUT synchronising the stream per chunk: greedy_finish_kernel reports
// (epoch, steps retired, done, length, unfinished rows) into a pinned host word after every step, and this loop keeps exactly
// `lookahead` steps queued behind the one the GPU is running.  The GPU never waits for the host (the next step is already in its
// queue when one retires) and at most `lookahead` steps are enqueued past the stop -- they are no-ops for the token state but
// stream the weights, which is what the old "8 steps, then hipStreamSynchronize" loop paid up to 7 times per utterance batch.
extern "C" int wt_decoder_run(wt_engine* e, int lookahead, int* cur_len, int* n_unfinished, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER) return fail(WT_E_INVALID, "wt_decoder_run: not a decoder engine");
    if (!e->begun) return fail(WT_E_STATE, "wt_decoder_run called before wt_decoder_begin");
    if (e->cfg.stream) return fail(WT_E_STATE, "wt_decoder_run: a continuous decode is open on this handle (wt_decoder_stream_run)");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    if (lookahead <= 0) lookahead = e->cfg.key.nt_loads ? 1 : 3;   // small models: a step is 0.15-0.3 ms, keep more of them queued
    if (lookahead > 64) lookahead = 64;
    const int max_steps = e->cfg.key.max_length - 1 - e->cfg.prompt_len;   // MaxLengthCriteria fires at the latest after this many steps
    unsigned long long mb = 0;
    int spins = 0, slices = 0;   // since the last launch: busy-wait iterations, then 20 us sleep slices
    for (;;) {
        mb = __atomic_load_n(e->mailbox, __ATOMIC_ACQUIRE);
        const bool mine = (int)(mb >> 48) == e->epoch;
        // the word carries the low 16 bits of the retired count: compare modulo 2^16 (a caller may have enqueued thousands of no-op
        // steps through wt_decoder_steps before handing over to this loop)
        const int retired = mine ? e->issued - (int)((unsigned)(e->issued - (int)((mb >> 32) & 0xffff)) & 0xffffu) : 0;
        if (mine && ((mb >> 31) & 1)) break;
        if (e->issued < max_steps && e->issued - retired <= lookahead) {
            // a row has finished (the word's unfinished mask lost a bit): from here on replay the graph whose attention skips such rows
            const unsigned full = (1u << e->cfg.key.B) - 1u;
            const int variant = (mine && retired > 0 && ((unsigned)mb & 0xffffu) != full) ? 1 : 0;
            int rc = enqueue_steps(e, 1, s, variant);
            if (rc) return rc;
            spins = slices = 0;
            continue;
        }
        if (e->issued >= max_steps && retired >= e->issued) break;   // every possible step has retired (done is set with the last)
        // Wait for the word: spin briefly (it often lands within microseconds of a check), then sleep in 20 us slices -- a whole step
        // (0.15-1.5 ms) is queued behind the running one, so the host has that long to enqueue the next, and N workers per GPU
        // (runtime.WhisperPipeline) x 8 ranks need not burn N x 8 host cores.
        if (spins < 2000) {
            ++spins;
            __builtin_ia32_pause();
            continue;
        }
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
        if (++slices % 64 == 0) {   // every few ms of waiting: is the stream still alive?
            const hipError_t q = hipStreamQuery(s);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(WT_E_HIP, "wt_decoder_run: stream failed: %s", hipGetErrorString(q));
            if (q == hipSuccess && slices > 4096) {   // an idle stream for > 0.1 s and the steps still unreported: they died without a word
                mb = __atomic_load_n(e->mailbox, __ATOMIC_ACQUIRE);
                const int r2 = (int)(mb >> 48) == e->epoch ? e->issued - (int)((unsigned)(e->issued - (int)((mb >> 32) & 0xffff)) & 0xffffu) : 0;
                if (r2 < e->issued && !((mb >> 31) & 1)) return fail(WT_E_STATE, "wt_decoder_run: %d steps enqueued, %d reported", e->issued, r2);
            }
        }
    }
    if (cur_len) *cur_len = (int)((mb >> 16) & 0x7fff);
    if (n_unfinished) *n_unfinished = __builtin_popcountll(mb & 0xffff);
    for (EvTimer* t : {&e->t_cross, &e->t_gemm, &e->t_enc_attn, &e->t_skinny}) timer_collect(*t);
    return WT_OK;
}

extern "C" int wt_decoder_poll(wt_engine* e, int* cur_len, int* n_unfinished, int* done, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun) return fail(WT_E_STATE, "wt_decoder_poll: no decode in flight");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->h_state, e->st, sizeof(DecState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cur_len) *cur_len = e->h_state->cur_len[0];
    if (n_unfinished) *n_unfinished = e->h_state->n_unfinished;
    if (done) *done = e->h_state->done;
    for (EvTimer* t : {&e->t_cross, &e->t_gemm, &e->t_enc_attn, &e->t_skinny}) timer_collect(*t);
    return WT_OK;
}

extern "C" int wt_decoder_read_ids(wt_engine* e, int32_t* ids_out, int ld, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun) return fail(WT_E_STATE, "wt_decoder_read_ids: no decode in flight");
    if (!ids_out || ld < e->cfg.key.max_length) return fail(WT_E_INVALID, "wt_decoder_read_ids: row stride %d < max_length %d", ld, e->cfg.key.max_length);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    if (e->cfg.key.beam.num_beams > 1) {   // the best hypothesis of every utterance: finalize runs on the stream, behind the steps
        SelectParams sp;
        fill_select_params(e, sp);
        LAUNCH(launch_beam_finalize(sp, (hipStream_t)stream));
        HIPCHK(hipMemcpy2DAsync(ids_out, (size_t)ld * 4, e->beam_dev.out_ids, (size_t)e->cfg.key.max_length * 4, (size_t)e->cfg.key.max_length * 4, e->cfg.U,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return WT_OK;
    }
    HIPCHK(hipMemcpy2DAsync(ids_out, (size_t)ld * 4, e->ids, (size_t)e->cfg.key.max_length * 4, (size_t)e->cfg.key.max_length * 4, e->cfg.key.B,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}

extern "C" int wt_decoder_read_beam_scores(wt_engine* e, float* scores_out, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.beam.num_beams <= 1) return fail(WT_E_STATE, "wt_decoder_read_beam_scores: no beam decode in flight");
    if (!scores_out) return fail(WT_E_INVALID, "wt_decoder_read_beam_scores: null output");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    SelectParams sp;
    fill_select_params(e, sp);
    LAUNCH(launch_beam_finalize(sp, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(scores_out, e->beam_dev.out_scores, (size_t)e->cfg.U * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}

extern "C" int wt_decoder_read_logprobs(wt_engine* e, float* token_logprobs, int ld, float* sum_logprob, float* no_speech_prob, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || !e->cfg.key.lp.enabled)
        return fail(WT_E_STATE, "wt_decoder_read_logprobs: no decode with token log-probabilities in flight (wt_decoder_set_logprobs, then wt_decoder_begin)");
    if (!token_logprobs || !sum_logprob || ld < e->cfg.key.max_length)
        return fail(WT_E_INVALID, "wt_decoder_read_logprobs: null output or row stride %d < max_length %d", ld, e->cfg.key.max_length);
    if (no_speech_prob && e->cfg.key.lp.no_speech_token_id < 0)
        return fail(WT_E_INVALID, "wt_decoder_read_logprobs: no_speech_prob was not requested (no_speech_token_id -1)");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpy2DAsync(token_logprobs, (size_t)ld * 4, e->lp_tok, (size_t)e->cfg.key.max_length * 4, (size_t)e->cfg.key.max_length * 4, e->cfg.key.B, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sum_logprob, e->lp_sum, (size_t)e->cfg.key.B * 4, hipMemcpyDeviceToDevice, s));
    if (no_speech_prob) HIPCHK(hipMemcpyAsync(no_speech_prob, e->lp_nsp, (size_t)e->cfg.key.B * 4, hipMemcpyDeviceToDevice, s));
    return WT_OK;
}

// the post-pass of the token-level timestamps over the decode in flight: q_hist x resident cross-K -> matrix -> DTW -> seconds
static void tt_fill(const wt_engine* e, TokTsParams& p) {
    memset(&p, 0, sizeof p);
    const StepKey& k = e->cfg.key;
    p.q_hist = e->tt_qh; p.qh_rows = e->cfg.key.tt_rows; p.qh_steps = e->cfg.key.tt_steps;
    p.cross_k = e->cross_k; p.kv_half = e->kv_esz == 2 ? 1 : 0; p.cross_rows = e->cross_rows; p.H = e->H; p.S = e->S;
    p.n_sel = k.tt.n_sel;
    memcpy(p.layer, k.tt.layer, sizeof p.layer);
    memcpy(p.head, k.tt.head, sizeof p.head);
    p.width = e->cfg.tt_width; p.time_precision = e->cfg.tt_time_precision;
    p.st = e->st; p.n_cap = e->cfg.key.tt_steps; p.B = e->cfg.key.B;
    p.W = e->tt_W; p.mean = e->tt_mean; p.sdev = e->tt_sdev; p.matrix = e->tt_matrix; p.trace = e->tt_trace; p.trace_ld = tt_trace_ld(e->S);
    p.out = e->tt_out; p.out_ld = e->cfg.key.max_length;
}
extern "C" int wt_decoder_read_token_timestamps(wt_engine* e, float* out, int ld, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.tt.n_sel == 0)
        return fail(WT_E_STATE, "wt_decoder_read_token_timestamps: no decode with token-level timestamps in flight");
    if (!out || ld < e->cfg.key.max_length) return fail(WT_E_INVALID, "wt_decoder_read_token_timestamps: row stride %d < max_length %d", ld, e->cfg.key.max_length);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    TokTsParams p;
    tt_fill(e, p);
    for (int b = 0; b < e->cfg.key.B; ++b) LAUNCH(launch_tt_matrix(p, b, s));
    LAUNCH(launch_tt_dtw(p, s));
    HIPCHK(hipMemcpy2DAsync(out, (size_t)ld * 4, e->tt_out, (size_t)e->cfg.key.max_length * 4, (size_t)e->cfg.key.max_length * 4, e->cfg.key.B, hipMemcpyDeviceToDevice, s));
    return WT_OK;
}
// the two halves of the post-pass alone, for timing (tools/token_timestamp_cost.py): which = 1 the matrix launches of every utterance,
// 2 the DTW launch (over the matrix as it stands); and the bytes of the mode's device allocation
extern "C" int wt_dbg_token_timestamp_postpass(wt_engine* e, int which, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.tt.n_sel == 0) return fail(WT_E_STATE, "wt_dbg_token_timestamp_postpass: mode off");
    if (which != 1 && which != 2) return fail(WT_E_INVALID, "wt_dbg_token_timestamp_postpass: which = %d", which);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    TokTsParams p;
    tt_fill(e, p);
    if (which == 1) for (int b = 0; b < e->cfg.key.B; ++b) LAUNCH(launch_tt_matrix(p, b, s));
    else LAUNCH(launch_tt_dtw(p, s));
    return WT_OK;
}
extern "C" size_t wt_dbg_token_timestamp_bytes(const wt_engine* e) { return e ? e->tt_bytes : 0; }
// debug read-backs (whisper_trtllm_amd_debug.h): the captured queries [n_sel][B][max_length - 1][64] and, after
// wt_decoder_read_token_timestamps, the matrix [B][max_length - 1][S] (rows >= cur_len - 1 are not written)
extern "C" int wt_dbg_token_timestamp_q_hist(wt_engine* e, float* out, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.tt.n_sel == 0) return fail(WT_E_STATE, "wt_dbg_token_timestamp_q_hist: mode off");
    if (!out) return fail(WT_E_INVALID, "wt_dbg_token_timestamp_q_hist: null output");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    HIPCHK(hipMemcpyAsync(out, e->tt_qh, (size_t)e->cfg.key.tt.n_sel * e->cfg.key.tt_rows * e->cfg.key.tt_steps * HEAD_DIM * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}
extern "C" int wt_dbg_token_timestamp_matrix(wt_engine* e, float* out, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.tt.n_sel == 0) return fail(WT_E_STATE, "wt_dbg_token_timestamp_matrix: mode off");
    if (!out) return fail(WT_E_INVALID, "wt_dbg_token_timestamp_matrix: null output");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    HIPCHK(hipMemcpyAsync(out, e->tt_matrix, (size_t)e->cfg.key.tt_rows * e->cfg.key.tt_steps * e->S * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}
// the resident cross-K rows of one (layer, head): [B][S][64] widened to float (fp16 engines keep them in half) -- host staging, synchronises
extern "C" int wt_dbg_cross_k_head(wt_engine* e, int layer, int head, float* out_host, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun) return fail(WT_E_STATE, "wt_dbg_cross_k_head: no decode in flight");
    if (!out_host || layer < 0 || layer >= e->L || head < 0 || head >= e->H) return fail(WT_E_INVALID, "wt_dbg_cross_k_head: bad arguments");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    const size_t n = (size_t)e->S * HEAD_DIM;
    std::vector<char> tmp(n * e->kv_esz);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (int b = 0; b < e->cfg.key.B; ++b) {
        const char* src = (const char*)e->cross_k + ((((size_t)layer * e->cross_rows + b) * e->H + head) * n) * e->kv_esz;
        HIPCHK(hipMemcpy(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost));
        if (e->kv_esz == 4) memcpy(out_host + b * n, tmp.data(), n * 4);
        else for (size_t i = 0; i < n; ++i) out_host[b * n + i] = (float)((const _Float16*)tmp.data())[i];
    }
    return WT_OK;
}

// the resident self-K / self-V rows of one (layer, head): [B][T][64] -- host staging, synchronises
extern "C" int wt_dbg_self_kv_head(wt_engine* e, int layer, int head, int which, float* out_host, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.stream) return fail(WT_E_STATE, "wt_dbg_self_kv_head: no batch decode in flight");
    if (!out_host || layer < 0 || layer >= e->L || head < 0 || head >= e->H || (which != 0 && which != 1))
        return fail(WT_E_INVALID, "wt_dbg_self_kv_head: bad arguments");
    if (e->kv_esz != 4) return fail(WT_E_UNSUPPORTED, "wt_dbg_self_kv_head: fp32 decoder engines only");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    const size_t n = (size_t)e->T * HEAD_DIM;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const float* cache = which ? e->self_v : e->self_k;
    for (int b = 0; b < e->cfg.key.B; ++b)
        HIPCHK(hipMemcpy(out_host + b * n, cache + (((size_t)layer * e->cfg.key.B + b) * e->H + head) * n, n * 4, hipMemcpyDeviceToHost));
    return WT_OK;
}

// debug read-back: the plain logits [rows][V] the last executed step of a beam decode left in HBM
extern "C" int wt_dbg_beam_logits(wt_engine* e, float* logits_out, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.beam.num_beams <= 1) return fail(WT_E_STATE, "wt_dbg_beam_logits: no beam decode in flight");
    if (!logits_out) return fail(WT_E_INVALID, "wt_dbg_beam_logits: null output");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    HIPCHK(hipMemcpyAsync(logits_out, e->logits, (size_t)e->cfg.key.B * e->V * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}

// debug read-back (whisper_trtllm_amd_debug.h): per executed step and row (token, source beam within the utterance, score bits, utterance done)
extern "C" int wt_dbg_beam_trace(wt_engine* e, int32_t* trace_out, int steps, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !e->begun || e->cfg.key.beam.num_beams <= 1) return fail(WT_E_STATE, "wt_dbg_beam_trace: no beam decode in flight");
    if (!trace_out || steps < 1 || steps > e->cfg.key.max_length - 1) return fail(WT_E_INVALID, "wt_dbg_beam_trace: %d steps outside [1, max_length - 1]", steps);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    HIPCHK(hipMemcpyAsync(trace_out, e->beam_dev.trace, (size_t)steps * e->cfg.key.B * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WT_OK;
}

extern "C" int wt_decoder_greedy(wt_engine* e, const float* enc_hidden, int B, const wt_greedy_params* p, int32_t* ids_out,
                                 int* out_len, void* stream) {
    int rc = wt_decoder_begin(e, enc_hidden, B, p, stream);
    if (rc) return rc;
    int cur = 1, nu = B;
    if ((rc = wt_decoder_run(e, 0, &cur, &nu, stream))) return rc;
    if (ids_out && (rc = wt_decoder_read_ids(e, ids_out, p->max_length, stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (out_len) *out_len = cur;
    return WT_OK;
}

// ------------------------------------------------------------------------------------------------- Session surface
extern "C" int wt_engine_infer_shapes(wt_engine* e, const wt_tensor_desc* in, int n_in, wt_tensor_desc* out, int* n_out) {
    if (!e) return fail(WT_E_INVALID, "wt_engine_infer_shapes: null argument");
    const EngineDims dims = engine_dims(e);
    ShapeState st;
    char msg[400] = "";
    const int rc = infer_shapes(dims, in, n_in, out, n_out, &st, msg, sizeof msg);  // host_logic.cpp
    e->shapes_ok = st.ok;
    if (rc) return fail(rc, "%s", msg);
    e->c_B = st.c_B; e->c_s = st.c_s; e->c_ms = st.c_ms; e->c_mc = st.c_mc;
    return WT_OK;
}

extern "C" int wt_engine_run(wt_engine* e, const wt_binding* in, int n_in, const wt_binding* out, int n_out, void* stream) {
    if (!e) return fail(WT_E_INVALID, "wt_engine_run: null engine");
    if (!e->shapes_ok) return fail(WT_E_STATE, "wt_engine_run: call wt_engine_infer_shapes with the current input shapes first");
    auto get = [&](const wt_binding* arr, int n, const char* name) -> void* {
        for (int i = 0; i < n; ++i)
            if (arr[i].name && strcmp(arr[i].name, name) == 0) return arr[i].ptr;
        return nullptr;
    };
    hipStream_t s = (hipStream_t)stream;
    if (e->kind == WT_KIND_ENCODER) {
        const float* data = (const float*)get(in, n_in, "data");
        float* hs = (float*)get(out, n_out, "hidden_states");
        if (!data || !hs) return fail(WT_E_INVALID, "encoder run needs bindings 'data' and 'hidden_states'");
        return wt_encoder_forward(e, data, e->c_B, hs, stream);
    }
    // ---- decoder, by-value cache protocol of run.py:103-148 / model.py:407-470 (batch 1) ----
    const int* data = (const int*)get(in, n_in, "data");
    const float* enc = (const float*)get(in, n_in, "encoder_hidden_states");
    const float* spk = (const float*)get(in, n_in, "self_past_key");
    const float* spv = (const float*)get(in, n_in, "self_past_value");
    const float* cpk = (const float*)get(in, n_in, "cross_past_key");
    const float* cpv = (const float*)get(in, n_in, "cross_past_value");
    float* logits = (float*)get(out, n_out, "hidden_states");
    float* nsk = (float*)get(out, n_out, "next_self_keys");
    float* nsv = (float*)get(out, n_out, "next_self_values");
    float* nck = (float*)get(out, n_out, "next_cross_keys");
    float* ncv = (float*)get(out, n_out, "next_cross_values");
    if (!data || !enc || !spk || !spv || !cpk || !cpv || !logits || !nsk || !nsv || !nck || !ncv)
        return fail(WT_E_INVALID, "decoder run is missing a binding (need 7 input tensors besides the two masks and 5 outputs)");
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    int rc = dec_reserve(e, 1, e->T, (hipStream_t)stream);
    if (rc) return rc;
    const int LH = e->L * e->H, S = e->S;
    const int cache_len = e->c_ms - 1 < e->c_s ? e->c_ms - 1 : e->c_s;  // model.py:278
    const int cross_len = e->c_mc - 1;                                    // model.py:264
    // next_* start as copies of the used part of past_* (the reference's concat), then the step runs in place on them
    LAUNCH(launch_copy_cache_rows(spk, nsk, LH, e->c_s, cache_len + 1, cache_len, s));
    LAUNCH(launch_copy_cache_rows(spv, nsv, LH, e->c_s, cache_len + 1, cache_len, s));
    LAUNCH(launch_copy_cache_rows(cpk, nck, LH, S, S, cross_len, s));
    LAUNCH(launch_copy_cache_rows(cpv, ncv, LH, S, S, cross_len, s));
    if (cross_len < S) {  // cur = proj(enc[0 : S - cross_len]) lands behind the kept rows (model.py:265-272)
        rc = cross_kv_project(e, enc, 1, S - cross_len, cross_len, nck, ncv, 4, s);   // Session I/O caches are f32 in every engine (model.py:464-468)
        if (rc) return rc;
    }
    LAUNCH(launch_set_state(e->st, /*cur_len=*/1, /*pos=*/e->c_ms - 1, /*self_len=*/cache_len, s));
    StepIO io;
    io.ids = data; io.ids_ld = 1; io.self_k = nsk; io.self_v = nsv; io.self_cap = cache_len + 1;
    io.cross_k = nck; io.cross_v = ncv; io.cross_rows = 1; io.slot_row = nullptr; io.logits = logits; io.B = 1; io.kv_esz = 4;
    io.nsplit_self = 1; io.nsplit_cross = pick_splits(1, e->H, S); io.nt = 1;
    io.alive = nullptr;
    io.embed = true;
    io.argmax = nullptr; io.argmax_parts = nullptr;
    e->begun = false;  // the resident greedy state is clobbered by this call
    return enqueue_step(e, io, s);
}

// ------------------------------------------------------------------------------------------------- profiling
// Replays graph `g` (captured by the caller; consumed here) `iters` times between two hipEvents on `s`; every exit path releases
// the graph, its executable and the events.
static int replay_and_time(hipGraph_t g, int iters, int launches_per_replay, float* avg_us, hipStream_t s) {
    hipGraphExec_t ge = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    float ms = 0.f;
    hipError_t he;
    {
        std::lock_guard<std::mutex> lock(g_capture_mutex);
        he = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    }
    if (he == hipSuccess) he = hipEventCreate(&a);
    if (he == hipSuccess) he = hipEventCreate(&b);
    if (he == hipSuccess) he = hipGraphLaunch(ge, s);  // warm-up replay (replayed on the caller's stream, like the decode step)
    if (he == hipSuccess) he = hipEventRecord(a, s);
    for (int i = 0; i < iters && he == hipSuccess; ++i) he = hipGraphLaunch(ge, s);
    if (he == hipSuccess) he = hipEventRecord(b, s);
    if (he == hipSuccess) he = hipEventSynchronize(b);
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, a, b);
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
    if (ge) hipGraphExecDestroy(ge);
    hipGraphDestroy(g);
    if (he != hipSuccess) return fail(WT_E_HIP, "timing replay failed: %s", hipGetErrorString(he));
    *avg_us = ms * 1e3f / ((float)iters * launches_per_replay);
    return WT_OK;
}

extern "C" int wt_decoder_time_cross_attention(wt_engine* e, int iters, float* avg_us, void* stream) {
    return wt_decoder_time_kernel(e, "cross_attn", iters, avg_us, stream);
}

// Average launch time (us) of ONE kind of decode-step launch (LP_* above), measured the way the decode step runs it: the L
// per-layer launches of that kind (each layer's own weights / caches, so nothing is cache-resident that would not be in the real
// step) are captured into a hipGraph and replayed `iters` times between two hipEvents recorded on the launch stream.  (Events
// cannot bracket single kernels inside the step graph; an eager pass adds dispatch gaps.)  The residual stream is not advanced:
// every launch reads the current buffers, which is what its duration depends on.  Only to be called BETWEEN steps of a decode:
// the launches scribble on the step scratch (dq, duh, datt, dh2, dffn, the attention partials and the self-cache row at self_len),
// all of which the next step rewrites before reading.
extern "C" int wt_decoder_time_kernel(wt_engine* e, const char* which, int iters, float* avg_us, void* stream) {
    if (!e || e->kind != WT_KIND_DECODER || !which || !avg_us || iters < 1) return fail(WT_E_INVALID, "wt_decoder_time_kernel: bad arguments");
    if (!e->begun) return fail(WT_E_STATE, "wt_decoder_time_kernel needs a decode in flight (wt_decoder_begin)");
    static const char* names[LP_COUNT] = {"qkv", "self_attn", "pair", "cross_attn", "cross_out", "fc1", "fc2"};
    int part = -1;
    for (int i = 0; i < LP_COUNT; ++i)
        if (!strcmp(which, names[i])) part = i;
    if (part < 0) return fail(WT_E_NOTFOUND, "unknown decode kernel '%s' (qkv, self_attn, pair, cross_attn, cross_out, fc1, fc2)", which);
    DeviceGuard guard(e->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    StepIO io = step_io(e, 0);   // variant 0: no `alive`, no stream slot_row (a beam decode keeps its row table, as the beam step runs them)
    io.qh = nullptr;             // and no query history: this entry point times the launches without those three
    struct ProfilingOff {   // no event records inside the capture; the caller's setting comes back on every exit path
        wt_engine* e; bool was;
        explicit ProfilingOff(wt_engine* e_) : e(e_), was(e_->profiling) { e->profiling = false; }
        ~ProfilingOff() { e->profiling = was; }
    } profiling_off(e);
    hipGraph_t g = nullptr;
    {   // captures / instantiations are serialised process-wide (enqueue_steps)
        std::lock_guard<std::mutex> lock(g_capture_mutex);
        HIPCHK(hipStreamBeginCapture(e->own_stream, hipStreamCaptureModeThreadLocal));
        int rc = WT_OK;
        for (int i = 0; i < e->L && rc == WT_OK; ++i) rc = enqueue_layer_part(e, io, i, e->dh, e->dh2, part, e->own_stream);
        hipError_t ce = hipStreamEndCapture(e->own_stream, &g);
        if (rc != WT_OK || ce != hipSuccess) {
            if (g) hipGraphDestroy(g);
            return fail(WT_E_HIP, "capturing the timing graph of '%s' failed", which);
        }
    }
    return replay_and_time(g, iters, e->L, avg_us, s);
}

extern "C" int wt_dbg_step_graph_captures(const wt_engine* e) { return e ? e->graph_captures : 0; }

extern "C" int wt_engine_set_profiling(wt_engine* e, int enabled) {
    if (!e) return fail(WT_E_INVALID, "null engine");
    e->profiling = enabled != 0;
    for (EvTimer* t : {&e->t_cross, &e->t_gemm, &e->t_enc_attn, &e->t_skinny}) {
        timer_collect(*t);
        t->ms = 0.0;
        t->launches = 0;
    }
    return WT_OK;
}
extern "C" int wt_engine_get_timer(wt_engine* e, const char* which, wt_kernel_timer* out) {
    if (!e || !which || !out) return fail(WT_E_INVALID, "null argument");
    EvTimer* t = nullptr;
    if (!strcmp(which, "dec_cross_attn")) t = &e->t_cross;
    else if (!strcmp(which, "gemm_f32")) t = &e->t_gemm;
    else if (!strcmp(which, "enc_attn")) t = &e->t_enc_attn;
    else if (!strcmp(which, "vocab_proj")) t = &e->t_skinny;
    else return fail(WT_E_NOTFOUND, "unknown timer '%s'", which);
    timer_collect(*t);
    out->ms_total = (float)t->ms;
    out->launches = t->launches;
    return WT_OK;
}
