// Kernel-level test hooks (include/whisper_trtllm_amd_debug.h); thin wrappers over the launchers.
#include "../../include/whisper_trtllm_amd_debug.h"
#include "wt_common.h"

#include <string.h>

#include <vector>

using namespace wt;

static int rc_of(hipError_t e) { return e == hipSuccess ? 0 : -5; }

extern "C" int wt_dbg_gemm(const float* A, int lda, const float* W, const float* bias, const float* resid, float* C, int M,
                           int N, int K, int act, void* stream) {
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = lda; g.a_rows_per_batch = M; g.W = W; g.bias = bias; g.resid = resid; g.C = C; g.ldc = N;
    g.c_rows_per_batch = M; g.M = M; g.N = N; g.K = K; g.act = act;
    return rc_of(launch_gemm_f32(g, (hipStream_t)stream));
}
extern "C" int wt_dbg_gemm_stamps(const float* A, int lda, const float* W, const float* bias, const float* resid, float* C, int M,
                                  int N, int K, int act, long long* stamps, void* stream) {
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = lda; g.a_rows_per_batch = M; g.W = W; g.bias = bias; g.resid = resid; g.C = C; g.ldc = N;
    g.c_rows_per_batch = M; g.M = M; g.N = N; g.K = K; g.act = act; g.dbg_stamps = stamps;
    return rc_of(launch_gemm_f32(g, (hipStream_t)stream));
}
// fp32 GEMM on the bf16 matrix cores (launch_gemm_x3): the hook splits A and W into the caller's scratch planes (3 * M * K and 3 * N * K
// bf16) and multiplies; flags bit 0: C receives three bf16 planes of [M][N] instead of fp32; bit 1: skip the splitting (planes in place)
extern "C" int wt_dbg_gemm_x3_tile(const float* A, const float* W, const float* bias, const float* resid, void* C, int M, int N, int K, int act,
                                   void* a_planes, void* w_planes, int flags, int tile, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int out_split = flags & 1;
    int rc = 0;
    if (!(flags & 2)) {   // bit 1: the planes are in place already (timing of the product alone)
        if ((rc = rc_of(launch_split3(A, a_planes, (size_t)M * K, (size_t)M * K, s)))) return rc;
        if ((rc = rc_of(launch_split3(W, w_planes, (size_t)N * K, (size_t)N * K, s)))) return rc;
    }
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = (const float*)a_planes; g.lda = K; g.a_rows_per_batch = M; g.a_plane = (long long)M * K; g.W = (const float*)w_planes; g.w_plane = (long long)N * K;
    g.bias = bias; g.resid = resid; g.C = (float*)C; g.ldc = N; g.c_rows_per_batch = M; g.M = M; g.N = N; g.K = K; g.act = act;
    g.out_split = out_split; g.c_plane = (long long)M * N;
    return rc_of(launch_gemm_x3(g, s, tile));
}
extern "C" int wt_dbg_gemm_x3(const float* A, const float* W, const float* bias, const float* resid, void* C, int M, int N, int K, int act,
                              void* a_planes, void* w_planes, int flags, void* stream) {
    return wt_dbg_gemm_x3_tile(A, W, bias, resid, C, M, N, K, act, a_planes, w_planes, flags, 0, stream);
}
extern "C" int wt_dbg_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int d, void* stream) {
    return rc_of(launch_layernorm(x, w, b, y, rows, d, (hipStream_t)stream));
}
extern "C" int wt_dbg_layernorm_split(const float* x, const float* w, const float* b, void* planes, int rows, int d, void* stream) {
    return rc_of(launch_layernorm_split(x, w, b, planes, (size_t)rows * d, rows, d, (hipStream_t)stream));
}

// ---- the encoder's two convolutions and the cross-K/V projection, parameterised by the engine's own helpers (wt_common.h) ----
static size_t conv_scratch_layout(int B, int S, int C, int d, int mode, size_t& n_melT, size_t& n_c1, size_t& c1_off) {
    conv_ws_elems(B, S, C, d, n_melT, n_c1);
    const size_t esz = mode == CONV_X3 ? 6 : 4;
    c1_off = (n_melT * esz + 255) & ~(size_t)255;
    return c1_off + n_c1 * esz;
}
extern "C" size_t wt_dbg_encoder_convs_scratch_bytes(int B, int C, int S, int d, int mode) {
    size_t n_melT, n_c1, c1_off;
    return conv_scratch_layout(B, S, C, d, mode, n_melT, n_c1, c1_off);
}
extern "C" int wt_dbg_encoder_convs(const float* mel, const void* conv1_w, const float* conv1_b, const void* conv2_w, const float* conv2_b,
                                    const float* pos, float* out, void* scratch, int B, int C, int S, int d, int mode, int tile, void* stream) {
    if (B < 1 || S < 1 || C < 1 || C > 128 || d < 1 || mode < CONV_F32 || mode > CONV_F16 || (tile && mode != CONV_X3)) return -22;
    hipStream_t s = (hipStream_t)stream;
    size_t n_melT, n_c1, c1_off;
    conv_scratch_layout(B, S, C, d, mode, n_melT, n_c1, c1_off);
    char* melT = (char*)scratch;
    char* c1 = melT + c1_off;
    GemmParams c1g, c2g;
    conv_gemm_params(mode, melT, n_melT, c1, n_c1, conv1_w, conv1_b, conv2_w, conv2_b, pos, out, B, S, C, d, c1g, c2g);
    if (mode == CONV_X3 && !(gemm_x3_usable(c1g) && gemm_x3_usable(c2g))) return -22;
    int rc = rc_of(conv_ws_clear(melT, n_melT, c1, n_c1, mode == CONV_X3 ? 6 : 4, s));
    if (rc) return rc;
    const int Fr = 2 * S;
    if (mode == CONV_X3) {
        if ((rc = rc_of(launch_mel_transpose_split(mel, melT, n_melT, B, C, Fr, s)))) return rc;
        if ((rc = rc_of(launch_gemm_x3(c1g, s, tile)))) return rc;
        return rc_of(launch_gemm_x3(c2g, s, tile));
    }
    if (mode == CONV_F16) {
        if ((rc = rc_of(launch_mel_transpose_h(mel, melT, B, C, Fr, s)))) return rc;
        if ((rc = rc_of(launch_gemm_f16(c1g, true, s)))) return rc;
        return rc_of(launch_gemm_f16(c2g, false, s));
    }
    if ((rc = rc_of(launch_mel_transpose(mel, (float*)melT, B, C, Fr, s)))) return rc;
    if ((rc = rc_of(launch_gemm_f32(c1g, s)))) return rc;
    return rc_of(launch_gemm_f32(c2g, s));
}
extern "C" int wt_dbg_cross_kv(const float* A, int rows_total, const float* W, const float* bias, float* kcache, float* vcache, void* scratch,
                               int B, int rows, int H, int cap, int seq_off, int layer_rows, int row0, int mode, int tile, void* stream) {
    if (B < 1 || rows < 1 || rows > rows_total || seq_off < 0 || seq_off + rows > cap || row0 < 0 || row0 + B > layer_rows || mode < 0 || mode > 1 ||
        (tile && mode != 1))
        return -22;
    hipStream_t s = (hipStream_t)stream;
    const int d = H * HEAD_DIM;
    GemmParams g = cross_kv_gemm_params(A, rows_total, W, bias, kcache, vcache, 4, B, rows, H, cap, seq_off, row0);
    if (mode == 0) return rc_of(launch_gemm_f32(g, s));
    const size_t a_plane = (size_t)B * rows_total * d;
    char* w3 = (char*)scratch + ((a_plane * 6 + 255) & ~(size_t)255);
    int rc = rc_of(launch_split3(A, scratch, a_plane, a_plane, s));
    if (rc || (rc = rc_of(launch_split3(W, w3, 2 * (size_t)d * d, 2 * (size_t)d * d, s)))) return rc;
    cross_kv_x3(g, scratch, a_plane, w3);
    if (!gemm_x3_usable(g)) return -22;
    return rc_of(launch_gemm_x3(g, s, tile));
}

extern "C" int wt_dbg_encoder_attention(const float* qkv, float* ctx, int B, int S, int H, void* stream) {
    return rc_of(launch_encoder_attention(qkv, ctx, B, S, H, (hipStream_t)stream));
}
extern "C" int wt_dbg_encoder_attention_occupancy(void) { return encoder_attention_blocks_per_cu(); }
extern "C" int wt_dbg_encoder_attention_split(const float* qkv, void* ctx_planes, int B, int S, int H, void* stream) {
    return rc_of(launch_encoder_attention(qkv, nullptr, B, S, H, (hipStream_t)stream, ctx_planes, (size_t)B * S * H * 64));
}
// x3 attention: the hook splits fp32 q|k|v [B*S][3d] into the caller's scratch planes (3 * B*S * 3d bf16) and attends; context out as planes
extern "C" int wt_dbg_encoder_attention_x3(const float* qkv, void* qkv_planes, void* ctx_planes, int B, int S, int H, int skip_split, void* stream) {
    const size_t n = (size_t)B * S * 3 * H * 64;
    int rc = skip_split ? 0 : rc_of(launch_split3(qkv, qkv_planes, n, n, (hipStream_t)stream));
    if (rc) return rc;
    return rc_of(launch_encoder_attention_x3(qkv_planes, n, ctx_planes, (size_t)B * S * H * 64, B, S, H, (hipStream_t)stream));
}
extern "C" int wt_dbg_skinny(const float* X, const float* ln_w, const float* ln_b, const float* W, const float* bias,
                             const float* resid, float* Y, int B, int N, int K, int xmode, int act, float scale,
                             void* stream) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = X; k.ln_w = ln_w; k.ln_b = ln_b; k.W = W; k.bias = bias; k.resid = resid; k.Y = Y; k.B = B; k.N = N; k.K = K;
    k.xmode = xmode & 1; k.x_direct = (xmode >> 1) & 1; k.w_nt = (xmode >> 2) & 1; k.act = act; k.q_scale = scale; k.ymode = YMODE_PLAIN;
    return rc_of(launch_skinny(k, (hipStream_t)stream));
}
// probe (tools/microbench.py fold_fc1): fc2 with the GELU / LayerNorm finish of a folded fc1 in its prologue; timing only
extern "C" int wt_dbg_skinny_gelu_in(const float* X, const float* r, const float* t, const float* W, const float* bias, const float* resid,
                                     float* Y, int B, int N, int K, void* stream) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = X; k.ln_w = r; k.ln_b = t; k.W = W; k.bias = bias; k.resid = resid; k.Y = Y; k.B = B; k.N = N; k.K = K; k.w_nt = 1; k.q_scale = 1.f;
    return rc_of(launch_skinny_gelu_in_probe(k, (hipStream_t)stream));
}
extern "C" int wt_dbg_decode_attention(const float* q, const float* kcache, const float* vcache, float* part, int* cnt,
                                       float* out, int B, int H, int s_cap, int len, int n_split, void* stream) {
    if (len < 1 || len > s_cap || n_split < 1 || n_split > 16) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = kcache; a.vcache = vcache; a.part = part; a.cnt = cnt; a.out = out; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = n_split;
    a.fixed_len = len; a.nt = 1;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_decode_attention_folded(const float* u, const float* kcache, const float* vcache, float* part, int* cnt,
                                              float* out, const float* ln_h, const float* ln_r, const float* ln_t, int B, int H,
                                              int s_cap, int len, int n_split, void* stream) {
    if (len < 1 || len > s_cap || n_split < 1 || n_split > 16 || !ln_h || !ln_r || !ln_t || H * 64 > 1024) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = u; a.kcache = kcache; a.vcache = vcache; a.part = part; a.cnt = cnt; a.out = out; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = n_split;
    a.fixed_len = len; a.nt = 1; a.ln_h = ln_h; a.ln_r = ln_r; a.ln_t = ln_t;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_attention_then_projection(const float* q, const float* kcache, const float* vcache, float* part, const float* W,
                                               const float* bias, const float* resid, float* Y, int B, int H, int s_cap, int len,
                                               int n_split, void* stream) {
    if (len < 1 || len > s_cap || n_split != 2 || H * 64 > 1024) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = kcache; a.vcache = vcache; a.part = part; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = n_split;
    a.fixed_len = len; a.nt = 1; a.defer_merge = 1;
    int rc = rc_of(launch_dec_attn(a, (hipStream_t)stream));
    if (rc) return rc;
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.parts = part; k.parts_nsplit = n_split; k.parts_H = H; k.W = W; k.bias = bias; k.resid = resid; k.Y = Y; k.B = B; k.N = H * 64;
    k.K = H * 64; k.q_scale = 1.f; k.w_nt = 1;
    return rc_of(launch_skinny(k, (hipStream_t)stream));
}
extern "C" int wt_dbg_skinny_pair(const float* Xa, const float* Wa, const float* bias_a, const float* resid_a, float* Ya, int Na, int Ka,
                                  const float* Xb, const float* Xb2, const float* Wb, const float* bias_b, float* Yb, int Nb, int Kb,
                                  int B, void* stream) {
    SkinnyParams a, b;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    a.X = Xa; a.W = Wa; a.bias = bias_a; a.resid = resid_a; a.Y = Ya; a.B = B; a.N = Na; a.K = Ka; a.q_scale = 1.f; a.w_nt = 1;
    b.X = Xb; b.X2 = Xb2; b.x_direct = 1; b.W = Wb; b.bias = bias_b; b.Y = Yb; b.B = B; b.N = Nb; b.K = Kb; b.q_scale = 1.f; b.w_nt = 1;
    return rc_of(launch_skinny_pair(a, b, (hipStream_t)stream));
}

extern "C" int wt_dbg_self_attention_then_pair(const float* q, const float* kcache, const float* vcache, float* part, const float* Wo,
                                              const float* bo, const float* h, float* h1, const float* Wf, const float* c, float* u, int B, int H,
                                              int s_cap, int len, void* stream) {
    if (len < 1 || len > s_cap || H * 64 > 1024) return -22;
    const int d = H * 64;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = kcache; a.vcache = vcache; a.part = part; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = 2;
    a.fixed_len = len; a.nt = 1; a.defer_merge = 1;
    int rc = rc_of(launch_dec_attn(a, (hipStream_t)stream));
    if (rc) return rc;
    SkinnyParams k, k2;
    memset(&k, 0, sizeof k);
    memset(&k2, 0, sizeof k2);
    k.parts = part; k.parts_nsplit = 2; k.parts_H = H; k.W = Wo; k.bias = bo; k.resid = h; k.Y = h1; k.B = B; k.N = d; k.K = d; k.q_scale = 1.f; k.w_nt = 1;
    k2.parts = part; k2.parts_nsplit = 2; k2.parts_H = H; k2.X2 = h; k2.x_direct = 1; k2.W = Wf; k2.bias = c; k2.Y = u; k2.B = B; k2.N = d; k2.K = 2 * d;
    k2.q_scale = 1.f; k2.w_nt = 1;
    return rc_of(launch_skinny_pair(k, k2, (hipStream_t)stream));
}

extern "C" int wt_dbg_gemm_f16(const void* A, int lda, const void* W, const float* bias, const float* resid, void* C, int M, int N,
                               int K, int act, int out_half, void* stream) {
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = (const float*)A; g.lda = lda; g.a_rows_per_batch = M; g.W = (const float*)W; g.bias = bias; g.resid = resid;
    g.C = (float*)C; g.ldc = N; g.c_rows_per_batch = M; g.M = M; g.N = N; g.K = K; g.act = act;
    return rc_of(launch_gemm_f16(g, out_half != 0, (hipStream_t)stream));
}

extern "C" int wt_dbg_gemm_f16_variant(const void* A, int lda, const void* W, const float* bias, const float* resid, void* C, int M, int N,
                                       int K, int act, int out_half, int variant, void* stream) {
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = (const float*)A; g.lda = lda; g.a_rows_per_batch = M; g.W = (const float*)W; g.bias = bias; g.resid = resid;
    g.C = (float*)C; g.ldc = N; g.c_rows_per_batch = M; g.M = M; g.N = N; g.K = K; g.act = act;
    return rc_of(launch_gemm_f16(g, out_half != 0, (hipStream_t)stream, variant));
}

extern "C" int wt_dbg_encoder_attention_f16(const void* qkv, void* ctx, int B, int S, int H, void* stream) {
    return rc_of(launch_encoder_attention_f16(qkv, ctx, B, S, H, (hipStream_t)stream));
}


// ---- fp16 decoder engines: half weights (skinny GEMVs) and half K/V caches (decode attention); everything else fp32 ----
extern "C" int wt_dbg_skinny_f16(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias,
                                 const float* resid, float* Y, int B, int N, int K, int xmode, int act, float scale, void* stream) {
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = X; k.ln_w = ln_w; k.ln_b = ln_b; k.W = (const float*)W; k.w_half = 1; k.bias = bias; k.resid = resid; k.Y = Y; k.B = B; k.N = N; k.K = K;
    k.xmode = xmode & 1; k.x_direct = (xmode >> 1) & 1; k.w_nt = (xmode >> 2) & 1; k.act = act; k.q_scale = scale; k.ymode = YMODE_PLAIN;
    return rc_of(launch_skinny(k, (hipStream_t)stream));
}
extern "C" int wt_dbg_decode_attention_f16(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out,
                                           const float* ln_h, const float* ln_r, const float* ln_t, int B, int H, int s_cap, int len,
                                           int n_split, void* stream) {
    if (len < 1 || len > s_cap || n_split < 1 || n_split > 16 || H * 64 > 1024) return -22;
    if ((ln_h || ln_r || ln_t) && !(ln_h && ln_r && ln_t)) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.kv_half = 1; a.part = part; a.cnt = cnt; a.out = out;
    a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = n_split; a.fixed_len = len; a.nt = 1; a.ln_h = ln_h; a.ln_r = ln_r; a.ln_t = ln_t;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_attention_then_projection_f16(const float* q, const void* kcache, const void* vcache, float* part, const void* W,
                                                   const float* bias, const float* resid, float* Y, int B, int H, int s_cap, int len,
                                                   void* stream) {
    if (len < 1 || len > s_cap || H * 64 > 1024) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.kv_half = 1; a.part = part; a.B = B; a.H = H; a.s_cap = s_cap;
    a.n_split = 2; a.fixed_len = len; a.nt = 1; a.defer_merge = 1;
    int rc = rc_of(launch_dec_attn(a, (hipStream_t)stream));
    if (rc) return rc;
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.parts = part; k.parts_nsplit = 2; k.parts_H = H; k.W = (const float*)W; k.w_half = 1; k.bias = bias; k.resid = resid; k.Y = Y; k.B = B;
    k.N = H * 64; k.K = H * 64; k.q_scale = 1.f; k.w_nt = 1;
    return rc_of(launch_skinny(k, (hipStream_t)stream));
}
extern "C" int wt_dbg_skinny_pair_f16(const float* Xa, const void* Wa, const float* bias_a, const float* resid_a, float* Ya, int Na, int Ka,
                                      const float* Xb, const float* Xb2, const void* Wb, const float* bias_b, float* Yb, int Nb, int Kb,
                                      int B, void* stream) {
    SkinnyParams a, b;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    a.X = Xa; a.W = (const float*)Wa; a.w_half = 1; a.bias = bias_a; a.resid = resid_a; a.Y = Ya; a.B = B; a.N = Na; a.K = Ka; a.q_scale = 1.f; a.w_nt = 1;
    b.X = Xb; b.X2 = Xb2; b.x_direct = 1; b.W = (const float*)Wb; b.w_half = 1; b.bias = bias_b; b.Y = Yb; b.B = B; b.N = Nb; b.K = Kb; b.q_scale = 1.f; b.w_nt = 1;
    return rc_of(launch_skinny_pair(a, b, (hipStream_t)stream));
}
// cross-K/V projection of an fp16 decoder engine: A half [B][rows_total][d] (first `rows` rows of every utterance are projected),
// W half [2d][d], bias f32 [2d] -> K / V caches [B][H][kv_cap][64] rows [seq_off, seq_off + rows), half (out_half) or f32
extern "C" int wt_dbg_gemm_f16_kv(const void* A, int rows_total, const void* W, const float* bias, void* kcache, void* vcache, int B, int rows,
                                  int H, int kv_cap, int seq_off, int out_half, void* stream) {
    const int d = H * 64;
    if (rows < 1 || rows > rows_total || seq_off < 0 || seq_off + rows > kv_cap) return -22;
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = (const float*)A; g.lda = d; g.a_rows_per_batch = rows; g.a_batch_stride = (long long)rows_total * d;
    g.W = (const float*)W; g.bias = bias; g.M = B * rows; g.N = 2 * d; g.K = d;
    g.epi = EPI_KV_HEADS; g.C = (float*)kcache; g.C2 = (float*)vcache; g.c_rows_per_batch = rows; g.kv_heads = H; g.kv_cap = kv_cap; g.kv_seq_off = seq_off;
    return rc_of(launch_gemm_f16(g, out_half != 0, (hipStream_t)stream));
}

// ---- timestamp mode: the engine's two launches (launch_greedy_select with ts_on) over crafted logits and histories ----
struct TsScratch { size_t st, unf, mask, forced, part, total; };
static TsScratch ts_scratch_layout(int B, int V, int max_length) {
    TsScratch l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    l.st = take(sizeof(DecState)); l.unf = take((size_t)B * 4); l.mask = take((size_t)V); l.forced = take((size_t)(max_length + 1) * 4);
    l.part = take((size_t)B * SELECT_CHUNKS * sizeof(TsPart));
    l.total = off;
    return l;
}
extern "C" size_t wt_dbg_timestamp_select_scratch_bytes(int B, int V, int max_length) {
    if (B < 1 || V < 1 || max_length < 2) return 0;
    return ts_scratch_layout(B, V, max_length).total;
}
extern "C" int wt_dbg_timestamp_select(const float* logits, int B, int V, int32_t* ids, int max_length, const int32_t* cur_len,
                                       const wt_timestamp_params* t, int eos, int32_t* tok_out, float* stats_out, void* scratch, void* stream) {
    if (!logits || !ids || !cur_len || !t || !tok_out || !stats_out || !scratch || B < 1 || B > MAX_ROWS || V < 1 || max_length < 2) return -22;
    for (int b = 0; b < B; ++b)
        if (cur_len[b] < 1 || cur_len[b] >= max_length) return -22;
    if (eos < 0 || eos >= V) return -22;
    hipStream_t s = (hipStream_t)stream;
    const TsScratch l = ts_scratch_layout(B, V, max_length);
    char* base = (char*)scratch;
    DecState h;
    memset(&h, 0, sizeof h);
    for (int b = 0; b < B; ++b) {
        h.cur_len[b] = cur_len[b];
        h.pos[b] = cur_len[b] - 1;
        h.self_len[b] = cur_len[b] - 1;
    }
    int unf[MAX_ROWS];
    for (int b = 0; b < MAX_ROWS; ++b) unf[b] = 1;
    int rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.st, &h, sizeof h, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.unf, unf, (size_t)B * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.mask, 0, (size_t)V, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.forced, 0xff, (size_t)(max_length + 1) * 4, s)))) return rc;   // -1: nothing forced
    if ((rc = rc_of(hipStreamSynchronize(s)))) return rc;   // pageable sources
    SelectParams p;
    memset(&p, 0, sizeof p);
    p.logits = logits; p.mask = (const uint8_t*)(base + l.mask); p.forced = (const int*)(base + l.forced); p.ids = ids;
    p.unfinished = (int*)(base + l.unf); p.st = (DecState*)(base + l.st);
    p.n_parts = SELECT_CHUNKS; p.B = B; p.V = V; p.max_length = max_length; p.begin_index = -1; p.eos = eos; p.pad = eos; p.force_eos_step = -1;
    p.ts_on = 1; p.no_ts = t->no_timestamps_token_id; p.tb = t->timestamp_begin; p.ts_begin_index = t->begin_index;
    p.max_init = t->max_initial_timestamp_index; p.ts_part = (TsPart*)(base + l.part); p.ts_tok = tok_out; p.ts_stats = stats_out;
    return rc_of(launch_greedy_select(p, s));
}

// ---- beam search: the engine's launches (launch_greedy_select with beam_on, launch_beam_finalize) over crafted logits and histories ----
struct BeamScratch { size_t st, unf, mask, forced, part, sc, ids0, ids2, anc, urow, hn, hd, hw, hs, hl, hi, total; };
static BeamScratch beam_scratch_layout(int V, int max_length) {
    BeamScratch l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t R = MAX_ROWS;
    l.st = take(sizeof(DecState)); l.unf = take(R * 4); l.mask = take((size_t)V); l.forced = take((size_t)(max_length + 1) * 4);
    l.part = take(R * SELECT_CHUNKS * sizeof(BeamPart)); l.sc = take(R * 4); l.ids0 = take(R * max_length * 4); l.ids2 = take(R * max_length * 4);
    l.anc = take(2 * R * max_length * 4); l.urow = take(R * 4); l.hn = take(R * 4); l.hd = take(R * 4); l.hw = take(R * 8); l.hs = take(R * 8);
    l.hl = take(R * 4); l.hi = take(R * max_length * 4);
    l.total = off;
    return l;
}
extern "C" size_t wt_dbg_beam_select_scratch_bytes(int U, int nb, int V, int max_length) {
    if (U < 1 || nb < 2 || nb > MAX_BEAMS || U * nb > MAX_ROWS || V < 1 || max_length < 2) return 0;
    return beam_scratch_layout(V, max_length).total;
}
extern "C" int wt_dbg_beam_select(const float* logits, const float* beam_scores, const unsigned char* mask, int U, int nb, int V, const int32_t* ids,
                                  int max_length, int cur_len, int begin_index, int forced_token, int eos, int pad, const wt_beam_params* b,
                                  int32_t* cand_out, int32_t* next_out, int32_t* fin_ids, float* fin_scores, void* scratch, void* stream) {
    if (!logits || !beam_scores || !ids || !b || !cand_out || !next_out || !fin_ids || !fin_scores || !scratch) return -22;
    if (U < 1 || nb < 2 || nb > MAX_BEAMS || U * nb > MAX_ROWS || V < 1 || max_length < 2 || cur_len < 1 || cur_len >= max_length) return -22;
    if (eos < 0 || eos >= V || pad < 0 || pad >= V || forced_token >= V || forced_token == eos || b->num_beams != nb) return -22;
    hipStream_t s = (hipStream_t)stream;
    const int R = U * nb;
    const BeamScratch l = beam_scratch_layout(V, max_length);
    char* base = (char*)scratch;
    DecState h;
    memset(&h, 0, sizeof h);
    for (int r = 0; r < MAX_ROWS; ++r) {
        h.cur_len[r] = cur_len;
        h.pos[r] = cur_len - 1;
        h.self_len[r] = cur_len - 1;
    }
    int unf[MAX_ROWS];
    for (int r = 0; r < MAX_ROWS; ++r) unf[r] = 1;
    std::vector<int> forced(max_length + 1, -1);
    forced[cur_len] = forced_token < 0 ? -1 : forced_token;
    int rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.st, &h, sizeof h, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.unf, unf, sizeof unf, hipMemcpyHostToDevice, s)))) return rc;
    if (mask) rc = rc_of(hipMemcpyAsync(base + l.mask, mask, (size_t)V, hipMemcpyDeviceToDevice, s));
    else rc = rc_of(hipMemsetAsync(base + l.mask, 0, (size_t)V, s));
    if (rc) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.forced, forced.data(), forced.size() * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.anc, 0, 2 * (size_t)MAX_ROWS * max_length * 4, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.ids0, ids, (size_t)R * max_length * 4, hipMemcpyDeviceToDevice, s)))) return rc;
    if ((rc = rc_of(hipStreamSynchronize(s)))) return rc;   // pageable sources
    SelectParams p;
    memset(&p, 0, sizeof p);
    p.logits = logits; p.mask = (const uint8_t*)(base + l.mask); p.forced = (const int*)(base + l.forced); p.ids = (int*)(base + l.ids0);
    p.unfinished = (int*)(base + l.unf); p.st = (DecState*)(base + l.st);
    p.n_parts = SELECT_CHUNKS; p.B = R; p.V = V; p.max_length = max_length; p.begin_index = begin_index; p.eos = eos; p.pad = pad; p.force_eos_step = -1;
    p.beam_on = 1;
    BeamParams& bp = p.beam;
    bp.nb = nb; bp.U = U; bp.length_penalty = b->length_penalty; bp.early_stopping = b->early_stopping;
    bp.part = (BeamPart*)(base + l.part); bp.scores = (float*)(base + l.sc); bp.ids2 = (int*)(base + l.ids2); bp.anc = (int*)(base + l.anc); bp.anc_ld = max_length;
    bp.urow = (int*)(base + l.urow); bp.hyp_n = (int*)(base + l.hn); bp.hyp_done = (int*)(base + l.hd); bp.hyp_worst = (double*)(base + l.hw);
    bp.hyp_score = (double*)(base + l.hs); bp.hyp_len = (int*)(base + l.hl); bp.hyp_ids = (int*)(base + l.hi); bp.hyp_ld = max_length;
    bp.out_ids = fin_ids; bp.out_scores = fin_scores; bp.trace = next_out; bp.dbg_cand = cand_out;
    if ((rc = rc_of(launch_beam_init(p, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(bp.scores, beam_scores, (size_t)R * 4, hipMemcpyDeviceToDevice, s)))) return rc;
    if ((rc = rc_of(launch_greedy_select(p, s)))) return rc;
    if ((rc = rc_of(launch_beam_finalize(p, s)))) return rc;
    return rc_of(hipStreamSynchronize(s));
}
extern "C" int wt_dbg_decode_attention_beam(const float* q, const void* kcache, const void* vcache, const int32_t* anc, float* out, int B, int H, int s_cap,
                                            int len, int kv_half, void* stream) {
    if (!q || !kcache || !vcache || !anc || !out || B < 1 || B > MAX_ROWS || len < 1 || len > s_cap) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.out = out; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = 1;
    a.fixed_len = len; a.nt = 1; a.kv_half = kv_half ? 1 : 0; a.anc = anc; a.anc_ld = s_cap;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_decode_attention_rows(const float* q, const void* kcache, const void* vcache, const int32_t* slot_row, float* part, int* cnt, float* out,
                                            int B, int H, int s_cap, int len, int n_split, int kv_half, void* stream) {
    if (!q || !kcache || !vcache || !slot_row || !out || B < 1 || B > MAX_ROWS || len < 1 || len > s_cap || n_split < 1 || n_split > 16) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.part = part; a.cnt = cnt; a.out = out; a.B = B; a.H = H; a.s_cap = s_cap;
    a.n_split = n_split; a.fixed_len = len; a.nt = 1; a.kv_half = kv_half ? 1 : 0; a.slot_row = slot_row;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_decode_attention_grouped(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out, int B, int H,
                                               int s_cap, int len, int n_split, int group, int kv_half, void* stream) {
    if (!q || !kcache || !vcache || !out || B < 1 || B > MAX_ROWS || len < 1 || len > s_cap || n_split < 1 || n_split > 16) return -22;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.part = part; a.cnt = cnt; a.out = out; a.B = B; a.H = H; a.s_cap = s_cap;
    a.n_split = n_split; a.fixed_len = len; a.nt = 1; a.kv_half = kv_half ? 1 : 0; a.group = group;
    return rc_of(launch_dec_attn(a, (hipStream_t)stream));
}

// ---- the greedy step's fused launches, parameterised by the engine's own helpers (wt_common.h): the vocabulary GEMV with the argmax
// epilogue, the q|k|v projection with the in-place cache append, greedy_select_kernel + greedy_finish_kernel<false>, dec_embed_kernel ----
static size_t dbg_align(size_t n) { return (n + 255) & ~(size_t)255; }
// upload a host DecState to `dst`; synchronises (pageable source)
static int upload_state(void* dst, const DecState& h, hipStream_t s) {
    int rc = rc_of(hipMemcpyAsync(dst, &h, sizeof h, hipMemcpyHostToDevice, s));
    return rc ? rc : rc_of(hipStreamSynchronize(s));
}
static SkinnyParams dbg_vocab_params(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* logits,
                                     const DecState* st, int B, int N, int K, int xmode, int w_half, int w_nt) {
    SkinnyParams k = vocab_skinny_params(X, ln_w, ln_b, W, logits, st, B, N, K, w_nt ? 1 : 0, w_half ? 1 : 0);
    if (!xmode) k.xmode = XMODE_PLAIN;   // the engine always normalises and has no bias; the exact-integer cases need neither / both
    k.bias = bias;
    return k;
}
extern "C" int wt_dbg_vocab_argmax_parts(int B, int N, int K, int w_half) {
    if (B < 1 || B > MAX_ROWS || N < 1 || K < 8 || K > 1024) return -1;
    return skinny_grid(dbg_vocab_params(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, N, K, 1, w_half, 0));
}
extern "C" size_t wt_dbg_vocab_argmax_scratch_bytes(void) { return dbg_align(sizeof(DecState)); }
extern "C" int wt_dbg_vocab_argmax(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, const unsigned char* mask,
                                   const int32_t* cur_len, int begin_index, int B, int N, int K, int xmode, int w_half, int w_nt, int fused,
                                   float* logits, float* part_val, int32_t* part_idx, void* scratch, void* stream) {
    if (!X || !W || !cur_len || !scratch || B < 1 || B > MAX_ROWS || N < 1 || K < 8 || K > 1024 || (K & 7)) return -22;
    if (xmode && (!ln_w || !ln_b)) return -22;
    if (fused ? (!mask || !part_val || !part_idx) : !logits) return -22;
    hipStream_t s = (hipStream_t)stream;
    DecState h;
    memset(&h, 0, sizeof h);
    for (int b = 0; b < B; ++b) h.cur_len[b] = cur_len[b];
    int rc = upload_state(scratch, h, s);
    if (rc) return rc;
    SkinnyParams k = dbg_vocab_params(X, ln_w, ln_b, W, bias, fused ? nullptr : logits, (const DecState*)scratch, B, N, K, xmode, w_half, w_nt);
    if (fused) {
        SelectParams sp;
        memset(&sp, 0, sizeof sp);
        sp.mask = mask; sp.part_val = part_val; sp.part_idx = part_idx; sp.begin_index = begin_index; sp.trace = logits;
        sp.max_length = 2;   // one trace row per batch row: [B][1][N], step 0
        if (vocab_skinny_fuse_argmax(k, sp) < 1) return -22;
    }
    return rc_of(launch_skinny(k, s));
}

extern "C" size_t wt_dbg_skinny_qkv_append_scratch_bytes(void) { return dbg_align(sizeof(DecState)); }
extern "C" int wt_dbg_skinny_qkv_append(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* q, void* kcache,
                                        void* vcache, const int32_t* self_len, int B, int d, int s_cap, int w_half, int kv_half, int w_nt, float scale,
                                        void* scratch, void* stream) {
    if (!X || !ln_w || !ln_b || !W || !q || !kcache || !vcache || !self_len || !scratch) return -22;
    if (B < 1 || B > MAX_ROWS || d < 64 || d > 1024 || (d & 63) || s_cap < 1) return -22;
    for (int b = 0; b < B; ++b)
        if (self_len[b] < 0 || self_len[b] >= s_cap) return -22;
    hipStream_t s = (hipStream_t)stream;
    DecState h;
    memset(&h, 0, sizeof h);
    for (int b = 0; b < B; ++b) h.self_len[b] = self_len[b];
    int rc = upload_state(scratch, h, s);
    if (rc) return rc;
    SkinnyParams k = qkv_append_skinny_params(X, ln_w, ln_b, W, bias, q, kcache, vcache, (const DecState*)scratch, B, d, s_cap, w_nt ? 1 : 0,
                                              w_half ? 1 : 0, kv_half ? 1 : 0);
    k.q_scale = scale;
    return rc_of(launch_skinny(k, s));
}

// ---- the q|k|v and pair launches with the residual half of the folded query hoisted (engine.hip: enqueue_layer_part, d <= 1024) ----
extern "C" int wt_dbg_skinny_qkv_hoist(const float* X, const float* ln_w, const float* ln_b, const void* W, const float* bias, float* q, void* kcache,
                                       void* vcache, const int32_t* self_len, const void* Wh, const float* c, float* uh, int B, int d, int s_cap,
                                       int w_half, int kv_half, int w_nt, float scale, void* scratch, void* stream) {
    if (!X || !ln_w || !ln_b || !W || !q || !kcache || !vcache || !self_len || !scratch || !Wh || !c || !uh) return -22;
    if (B < 1 || B > MAX_ROWS || d < 64 || d > 1024 || (d & 63) || s_cap < 1) return -22;
    for (int b = 0; b < B; ++b)
        if (self_len[b] < 0 || self_len[b] >= s_cap) return -22;
    hipStream_t s = (hipStream_t)stream;
    DecState h;
    memset(&h, 0, sizeof h);
    for (int b = 0; b < B; ++b) h.self_len[b] = self_len[b];
    int rc = upload_state(scratch, h, s);
    if (rc) return rc;
    SkinnyParams k = qkv_append_skinny_params(X, ln_w, ln_b, W, bias, q, kcache, vcache, (const DecState*)scratch, B, d, s_cap, w_nt ? 1 : 0,
                                              w_half ? 1 : 0, kv_half ? 1 : 0);
    k.q_scale = scale;
    const SkinnyParams k2 = qfold_resid_skinny_params(X, Wh, c, uh, (const DecState*)scratch, B, d, w_nt ? 1 : 0, w_half ? 1 : 0);
    return rc_of(launch_skinny_qkv_hoist(k, k2, s));
}
extern "C" int wt_dbg_skinny_pair_hoisted(const float* a, const float* part, const void* Wo, const float* bo, const float* h, float* h1,
                                          const void* Wa, const float* uh, float* u, int B, int d, int w_half, void* stream) {
    if ((a != nullptr) == (part != nullptr) || !Wo || !bo || !h || !h1 || !Wa || !uh || !u) return -22;   // exactly one source of the context
    if (B < 1 || B > MAX_ROWS || d < 64 || d > 1024 || (d & 63)) return -22;
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.X = a; k.xmode = XMODE_PLAIN; k.W = (const float*)Wo; k.bias = bo; k.resid = h; k.Y = h1; k.B = B; k.N = d; k.K = d; k.q_scale = 1.f;
    k.w_nt = 1; k.w_half = w_half ? 1 : 0;   // (the pair launch streams its weights non-temporally whatever w_nt says)
    if (part) { k.parts = part; k.parts_nsplit = 2; k.parts_H = d / HEAD_DIM; }
    const SkinnyParams k2 = qfold_ctx_skinny_params(a, part, Wa, uh, u, nullptr, B, d, 1, w_half ? 1 : 0);
    return rc_of(launch_skinny_pair(k, k2, (hipStream_t)stream));
}

// ---- decode attention as the step graph launches it: the length per row from a device DecState (fixed_len = 0), the skip-finished-rows
// and slot_row forms, either load policy ----
// a host DecState with self_len[b] = self_len[b] (b < B), refusing a length outside the cache
static bool dbg_self_len_state(DecState& h, const int32_t* self_len, int B, int s_cap) {
    memset(&h, 0, sizeof h);
    for (int b = 0; b < MAX_ROWS; ++b) { h.slot_row[b] = -1; h.row_force[b] = -1; }
    for (int b = 0; b < B; ++b) {
        if (self_len[b] < 0 || self_len[b] >= s_cap) return false;
        h.self_len[b] = self_len[b];
    }
    return true;
}
extern "C" size_t wt_dbg_decode_attention_state_scratch_bytes(void) { return dbg_align(sizeof(DecState)); }
extern "C" int wt_dbg_decode_attention_state(const float* q, const void* kcache, const void* vcache, float* part, int* cnt, float* out,
                                             const int32_t* self_len, int fixed_len, const int32_t* alive, const int32_t* slot_row, int rows,
                                             const float* ln_h, const float* ln_r, const float* ln_t, int B, int H, int s_cap, int n_split,
                                             int kv_half, int nt, int defer_merge, void* scratch, void* stream) {
    if (!q || !kcache || !vcache || B < 1 || B > MAX_ROWS || H < 1 || H * 64 > 1024 || s_cap < 1 || n_split < 1 || n_split > 16) return -22;
    if ((nt != 0 && nt != 1) || (kv_half != 0 && kv_half != 1) || (defer_merge != 0 && defer_merge != 1)) return -22;
    if ((ln_h || ln_r || ln_t) && !(ln_h && ln_r && ln_t)) return -22;
    if ((self_len != nullptr) == (fixed_len > 0) || fixed_len < 0 || fixed_len > s_cap) return -22;   // exactly one source of the length
    if (self_len && !scratch) return -22;
    if (defer_merge ? (n_split < 2 || !part) : (!out || (n_split > 1 && (!part || !cnt)))) return -22;
    if (rows < 1 || (!slot_row && rows < B)) return -22;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (slot_row) {   // device table: checked on the host before anything is launched
        int32_t host_rows[MAX_ROWS];
        if ((rc = rc_of(hipMemcpyAsync(host_rows, slot_row, (size_t)B * 4, hipMemcpyDeviceToHost, s)))) return rc;
        if ((rc = rc_of(hipStreamSynchronize(s)))) return rc;
        for (int b = 0; b < B; ++b)
            if (host_rows[b] < -1 || host_rows[b] >= rows) return -22;
    }
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    if (self_len) {
        DecState h;
        if (!dbg_self_len_state(h, self_len, B, s_cap)) return -22;
        if ((rc = upload_state(scratch, h, s))) return rc;
        a.st = (const DecState*)scratch;
    }
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.part = part; a.cnt = cnt; a.out = out; a.B = B; a.H = H;
    a.s_cap = s_cap; a.n_split = n_split; a.fixed_len = fixed_len; a.nt = nt; a.kv_half = kv_half; a.defer_merge = defer_merge;
    a.alive = alive; a.slot_row = slot_row; a.ln_h = ln_h; a.ln_r = ln_r; a.ln_t = ln_t;
    return rc_of(launch_dec_attn(a, s));
}
extern "C" size_t wt_dbg_self_attention_then_pair_state_scratch_bytes(void) { return dbg_align(sizeof(DecState)); }
extern "C" int wt_dbg_self_attention_then_pair_state(const float* q, const void* kcache, const void* vcache, float* part, const void* Wo,
                                                    const float* bo, const float* h, float* h1, const void* Wf, const float* c, float* u,
                                                    const int32_t* self_len, int fixed_len, int B, int H, int s_cap, int half, int nt,
                                                    void* scratch, void* stream) {
    if (!q || !kcache || !vcache || !part || !Wo || !bo || !h || !h1 || !Wf || !c || !u) return -22;
    if (B < 1 || B > MAX_ROWS || H < 1 || H * 64 > 1024 || s_cap < 1 || (nt != 0 && nt != 1) || (half != 0 && half != 1)) return -22;
    if ((self_len != nullptr) == (fixed_len > 0) || fixed_len < 0 || fixed_len > s_cap || (self_len && !scratch)) return -22;
    hipStream_t s = (hipStream_t)stream;
    const int d = H * 64;
    DecAttnParams a;
    memset(&a, 0, sizeof a);
    if (self_len) {
        DecState hs;
        if (!dbg_self_len_state(hs, self_len, B, s_cap)) return -22;
        const int rc = upload_state(scratch, hs, s);
        if (rc) return rc;
        a.st = (const DecState*)scratch;
    }
    a.q = q; a.kcache = (const float*)kcache; a.vcache = (const float*)vcache; a.part = part; a.B = B; a.H = H; a.s_cap = s_cap; a.n_split = 2;
    a.fixed_len = fixed_len; a.nt = nt; a.kv_half = half; a.defer_merge = 1;
    int rc = rc_of(launch_dec_attn(a, s));
    if (rc) return rc;
    SkinnyParams k, k2;
    memset(&k, 0, sizeof k);
    memset(&k2, 0, sizeof k2);
    k.parts = part; k.parts_nsplit = 2; k.parts_H = H; k.W = (const float*)Wo; k.bias = bo; k.resid = h; k.Y = h1; k.B = B; k.N = d; k.K = d;
    k.q_scale = 1.f; k.w_nt = nt; k.w_half = half; k.st = a.st;
    k2.parts = part; k2.parts_nsplit = 2; k2.parts_H = H; k2.X2 = h; k2.x_direct = 1; k2.W = (const float*)Wf; k2.bias = c; k2.Y = u; k2.B = B;
    k2.N = d; k2.K = 2 * d; k2.q_scale = 1.f; k2.w_nt = nt; k2.w_half = half; k2.st = a.st;
    return rc_of(launch_skinny_pair(k, k2, s));
}

static void dbg_state_to_dev(const int32_t* w, DecState& h) {
    memset(&h, 0, sizeof h);
    h.done = w[0]; h.n_unfinished = w[1]; h.step = w[2]; h.seq = w[3];
    for (int b = 0; b < MAX_ROWS; ++b) {
        h.cur_len[b] = w[4 + b]; h.pos[b] = w[4 + MAX_ROWS + b]; h.self_len[b] = w[4 + 2 * MAX_ROWS + b];
        h.slot_row[b] = -1; h.row_force[b] = -1;
    }
}
static void dbg_state_to_host(const DecState& h, int32_t* w) {
    w[0] = h.done; w[1] = h.n_unfinished; w[2] = h.step; w[3] = h.seq;
    for (int b = 0; b < MAX_ROWS; ++b) {
        w[4 + b] = h.cur_len[b]; w[4 + MAX_ROWS + b] = h.pos[b]; w[4 + 2 * MAX_ROWS + b] = h.self_len[b];
    }
}
struct SelScratch { size_t st, forced, rows, pv, pi, total; };
static SelScratch sel_scratch_layout(int max_length) {
    SelScratch l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = dbg_align(off + bytes); return o; };
    l.st = take(sizeof(DecState)); l.forced = take((size_t)(max_length + 1) * 4); l.rows = take(MAX_ROWS * 4);
    l.pv = take((size_t)MAX_ROWS * SELECT_CHUNKS * 4); l.pi = take((size_t)MAX_ROWS * SELECT_CHUNKS * 4);
    l.total = off;
    return l;
}
extern "C" size_t wt_dbg_greedy_select_scratch_bytes(int max_length) { return max_length < 2 ? 0 : sel_scratch_layout(max_length).total; }
extern "C" int wt_dbg_greedy_select(const float* logits, const float* part_val, const int32_t* part_idx, int n_parts, const unsigned char* mask,
                                    const int32_t* forced, int32_t* ids, int32_t* unfinished, int32_t* state, int force_eos_step,
                                    const int32_t* force_eos_rows, const void* tok_emb, const float* pos_emb, int pos_rows, int emb_half, float* next_x,
                                    int B, int V, int d, int max_length, int begin_index, int eos, int pad, void* scratch, void* stream) {
    const bool fused = logits == nullptr;
    if (!mask || !forced || !ids || !unfinished || !state || !scratch || B < 1 || B > MAX_ROWS || V < 1 || max_length < 2) return -22;
    if (fused ? (!part_val || !part_idx || n_parts < 1) : (part_val || part_idx)) return -22;
    if (eos < 0 || eos >= V || pad < 0 || pad >= V) return -22;
    if (next_x && (!tok_emb || !pos_emb || d < 4 || (d & 3))) return -22;
    for (int b = 0; b < B; ++b)   // greedy_select_kernel reads cur_len[b]; greedy_finish_kernel indexes ids / forced by row 0's cur_len
        if (state[4 + b] < 1 || state[4 + b] >= max_length) return -22;
    for (int b = 0; b < B; ++b)   // ... and advances pos / self_len per row: every row's next position must lie inside pos_emb
        if (next_x && (state[4 + MAX_ROWS + b] < -1 || state[4 + MAX_ROWS + b] + 1 >= pos_rows)) return -22;
    for (int i = 0; i < max_length; ++i)
        if (forced[i] >= V) return -22;
    hipStream_t s = (hipStream_t)stream;
    const SelScratch l = sel_scratch_layout(max_length);
    char* base = (char*)scratch;
    DecState h;
    dbg_state_to_dev(state, h);
    int rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.forced, forced, (size_t)max_length * 4, hipMemcpyHostToDevice, s)))) return rc;
    if (force_eos_rows && (rc = rc_of(hipMemcpyAsync(base + l.rows, force_eos_rows, (size_t)B * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = upload_state(base + l.st, h, s))) return rc;
    SelectParams p;
    greedy_select_params(p, logits, mask, (const int*)(base + l.forced), ids, unfinished, (DecState*)(base + l.st), nullptr,
                         fused ? const_cast<float*>(part_val) : (float*)(base + l.pv), fused ? const_cast<int32_t*>(part_idx) : (int*)(base + l.pi),
                         tok_emb, pos_emb, next_x, d, emb_half ? 1 : 0, B, V, max_length, begin_index, eos, pad, force_eos_step,
                         force_eos_rows ? (const int*)(base + l.rows) : nullptr, nullptr, 0);
    if (fused) greedy_select_fused(p, n_parts);
    if ((rc = rc_of(launch_greedy_select(p, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(&h, base + l.st, sizeof h, hipMemcpyDeviceToHost, s)))) return rc;
    if ((rc = rc_of(hipStreamSynchronize(s)))) return rc;
    dbg_state_to_host(h, state);
    return 0;
}

// ---- log-probability mode: the greedy tail's three forms on caller-supplied operands ----
struct LpScratch { size_t st, unf, forced, pv, pi, lpp, side, tsp, tok, lg, total; };
static LpScratch lp_scratch_layout(int B, int V, int max_length) {
    LpScratch l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = dbg_align(off + bytes); return o; };
    const size_t parts = (size_t)(V / 2 + SELECT_CHUNKS + 1);   // >= workgroups of any vocabulary GEMV plan (a group takes >= 2 rows)
    l.st = take(sizeof(DecState)); l.unf = take((size_t)B * 4); l.forced = take((size_t)(max_length + 1) * 4);
    l.pv = take((size_t)B * parts * 4); l.pi = take((size_t)B * parts * 4); l.lpp = take((size_t)B * parts * sizeof(float4));
    l.side = take((size_t)B * 2 * 4); l.tsp = take((size_t)B * SELECT_CHUNKS * sizeof(TsPart)); l.tok = take((size_t)B * max_length * 4);
    l.lg = take((size_t)B * V * 4);
    l.total = off;
    return l;
}
extern "C" size_t wt_dbg_logprob_select_scratch_bytes(int B, int V, int max_length) {
    if (B < 1 || B > MAX_ROWS || V < 1 || max_length < 2) return 0;
    return lp_scratch_layout(B, V, max_length).total;
}
extern "C" int wt_dbg_logprob_select(int form, const float* X, const float* W, int K, const float* logits, const unsigned char* mask,
                                     const int32_t* forced, int32_t* ids, int B, int V, int max_length, int cur_len, int step, int begin_index,
                                     int eos, int force_eos_step, const wt_timestamp_params* t, int no_speech_token_id, float* logprob_out,
                                     float* sum_out, float* no_speech_out, void* scratch, void* stream) {
    if (form < 0 || form > 2 || !mask || !forced || !ids || !logprob_out || !sum_out || !scratch) return -22;
    if (B < 1 || B > MAX_ROWS || V < 1 || max_length < 2 || cur_len < 1 || cur_len >= max_length || step < 0) return -22;
    if (eos < 0 || eos >= V || no_speech_token_id >= V || (no_speech_token_id >= 0 && !no_speech_out)) return -22;
    if (form == 0 ? (!X || !W || K < 8 || K > 1024 || (K & 7)) : !logits) return -22;
    if (form == 2 && !t) return -22;
    for (int i = 0; i < max_length; ++i)
        if (forced[i] >= V) return -22;
    hipStream_t s = (hipStream_t)stream;
    const LpScratch l = lp_scratch_layout(B, V, max_length);
    char* base = (char*)scratch;
    DecState h;
    memset(&h, 0, sizeof h);
    h.step = step;
    for (int b = 0; b < MAX_ROWS; ++b) {
        h.cur_len[b] = cur_len; h.pos[b] = cur_len - 1; h.self_len[b] = cur_len - 1; h.slot_row[b] = -1; h.row_force[b] = -1;
    }
    int unf[MAX_ROWS];
    for (int b = 0; b < MAX_ROWS; ++b) unf[b] = 1;
    int rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.forced, forced, (size_t)max_length * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.unf, unf, (size_t)B * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.tok, 0, (size_t)B * max_length * 4, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.side, 0, (size_t)B * 2 * 4, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(sum_out, 0, (size_t)B * 4, s)))) return rc;
    if ((rc = upload_state(base + l.st, h, s))) return rc;
    SelectParams p;
    greedy_select_params(p, form == 0 ? (const float*)(base + l.lg) : logits, mask, (const int*)(base + l.forced), ids, (int*)(base + l.unf),
                         (DecState*)(base + l.st), nullptr, (float*)(base + l.pv), (int*)(base + l.pi), nullptr, nullptr, nullptr, 0, 0, B, V,
                         max_length, begin_index, eos, eos, force_eos_step, nullptr, nullptr, 0);
    p.lp_on = 1; p.lp_ns = no_speech_token_id; p.lp_part = (float4*)(base + l.lpp); p.lp_side = (float*)(base + l.side);
    p.lp_tok = (float*)(base + l.tok); p.lp_sum = sum_out; p.lp_nsp = no_speech_out;
    if (form == 2) {
        p.ts_on = 1; p.no_ts = t->no_timestamps_token_id; p.tb = t->timestamp_begin; p.ts_begin_index = t->begin_index;
        p.max_init = t->max_initial_timestamp_index; p.ts_part = (TsPart*)(base + l.tsp);
    }
    if (form == 0) {
        SkinnyParams k = dbg_vocab_params(X, nullptr, nullptr, W, nullptr, nullptr, (const DecState*)(base + l.st), B, V, K, 0, 0, 0);
        const int grid = vocab_skinny_fuse_argmax(k, p);
        if (grid < 1 || grid > V / 2 + SELECT_CHUNKS + 1) return -22;
        if ((rc = rc_of(launch_skinny(k, s)))) return rc;
        greedy_select_fused(p, grid);
    }
    if ((rc = rc_of(launch_greedy_select(p, s)))) return rc;
    if ((rc = rc_of(hipMemcpy2DAsync(logprob_out, 4, p.lp_tok + cur_len, (size_t)max_length * 4, 4, B, hipMemcpyDeviceToDevice, s)))) return rc;
    return rc_of(hipStreamSynchronize(s));
}

// ---- temperature sampling: the same launches in their sampling form (form 0: the vocabulary GEMV's epilogue from X, W; form 1: the select
// kernel from logits, the timestamp-mode pair when `t` is given), then the finish kernel ----
struct SmScratch { size_t seeds, sc, ts, key, total; };
static SmScratch sm_scratch_layout(int B, int V, int max_length) {
    SmScratch l;
    size_t off = lp_scratch_layout(B, V, max_length).total;
    auto take = [&](size_t bytes) { const size_t o = off; off = dbg_align(off + bytes); return o; };
    const size_t parts = (size_t)(V / 2 + SELECT_CHUNKS + 1);
    l.seeds = take((size_t)B * 8); l.sc = take((size_t)B * parts * 4); l.ts = take((size_t)B * SELECT_CHUNKS * sizeof(float4)); l.key = take((size_t)B * 4);
    l.total = off;
    return l;
}
extern "C" size_t wt_dbg_sample_select_scratch_bytes(int B, int V, int max_length) {
    if (B < 1 || B > MAX_ROWS || V < 1 || max_length < 2) return 0;
    return sm_scratch_layout(B, V, max_length).total;
}
extern "C" int wt_dbg_sample_select(int form, const float* X, const float* W, int K, const float* logits, const unsigned char* mask,
                                    const int32_t* forced, int32_t* ids, int B, int V, int max_length, int cur_len, int step, int begin_index,
                                    int eos, int force_eos_step, const wt_timestamp_params* t, int no_speech_token_id, float temperature,
                                    const uint64_t* seeds, float* logprob_out, float* sum_out, float* no_speech_out, float* key_out,
                                    void* scratch, void* stream) {
    if (form < 0 || form > 1 || !mask || !forced || !ids || !logprob_out || !sum_out || !key_out || !seeds || !scratch) return -22;
    if (!(temperature > 0.f) || !(temperature <= 3.4028235e38f)) return -22;
    if (B < 1 || B > MAX_ROWS || V < 1 || max_length < 2 || cur_len < 1 || cur_len >= max_length || step < 0) return -22;
    if (eos < 0 || eos >= V || no_speech_token_id >= V || (no_speech_token_id >= 0 && !no_speech_out)) return -22;
    if (form == 0 ? (!X || !W || t) : !logits) return -22;
    if (!t && (K < 8 || K > 1024 || (K & 7))) return -22;   // form 1 walks the logits in the partition of form 0's GEMV for this K
    for (int i = 0; i < max_length; ++i)
        if (forced[i] >= V) return -22;
    hipStream_t s = (hipStream_t)stream;
    const LpScratch l = lp_scratch_layout(B, V, max_length);
    const SmScratch m = sm_scratch_layout(B, V, max_length);
    char* base = (char*)scratch;
    DecState h;
    memset(&h, 0, sizeof h);
    h.step = step;
    for (int b = 0; b < MAX_ROWS; ++b) {
        h.cur_len[b] = cur_len; h.pos[b] = cur_len - 1; h.self_len[b] = cur_len - 1; h.slot_row[b] = -1; h.row_force[b] = -1;
    }
    int unf[MAX_ROWS];
    for (int b = 0; b < MAX_ROWS; ++b) unf[b] = 1;
    int rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.forced, forced, (size_t)max_length * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + l.unf, unf, (size_t)B * 4, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(base + m.seeds, seeds, (size_t)B * 8, hipMemcpyHostToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.tok, 0, (size_t)B * max_length * 4, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(base + l.side, 0, (size_t)B * 2 * 4, s)))) return rc;
    if ((rc = rc_of(hipMemsetAsync(sum_out, 0, (size_t)B * 4, s)))) return rc;
    if ((rc = upload_state(base + l.st, h, s))) return rc;
    SelectParams p;
    greedy_select_params(p, form == 0 ? (const float*)(base + l.lg) : logits, mask, (const int*)(base + l.forced), ids, (int*)(base + l.unf),
                         (DecState*)(base + l.st), nullptr, (float*)(base + l.pv), (int*)(base + l.pi), nullptr, nullptr, nullptr, 0, 0, B, V,
                         max_length, begin_index, eos, eos, force_eos_step, nullptr, nullptr, 0);
    p.lp_on = 1; p.lp_ns = no_speech_token_id; p.lp_part = (float4*)(base + l.lpp); p.lp_side = (float*)(base + l.side);
    p.lp_tok = (float*)(base + l.tok); p.lp_sum = sum_out; p.lp_nsp = no_speech_out;
    p.samp_on = 1; p.samp_temp = temperature; p.samp_seeds = (const unsigned long long*)(base + m.seeds); p.samp_sc = (float*)(base + m.sc);
    p.samp_ts = (float4*)(base + m.ts); p.samp_key = (float*)(base + m.key);
    p.samp_K = K; p.samp_parts_cap = V / 2 + SELECT_CHUNKS + 1;
    if (t) {
        p.ts_on = 1; p.no_ts = t->no_timestamps_token_id; p.tb = t->timestamp_begin; p.ts_begin_index = t->begin_index;
        p.max_init = t->max_initial_timestamp_index; p.ts_part = (TsPart*)(base + l.tsp);
    }
    if (form == 0) {
        SkinnyParams k = dbg_vocab_params(X, nullptr, nullptr, W, nullptr, nullptr, (const DecState*)(base + l.st), B, V, K, 0, 0, 0);
        const int grid = vocab_skinny_fuse_argmax(k, p);
        if (grid < 1 || grid > V / 2 + SELECT_CHUNKS + 1) return -22;
        if ((rc = rc_of(launch_skinny(k, s)))) return rc;
        greedy_select_fused(p, grid);
    }
    if ((rc = rc_of(launch_greedy_select(p, s)))) return rc;
    if ((rc = rc_of(hipMemcpy2DAsync(logprob_out, 4, p.lp_tok + cur_len, (size_t)max_length * 4, 4, B, hipMemcpyDeviceToDevice, s)))) return rc;
    if ((rc = rc_of(hipMemcpyAsync(key_out, base + m.key, (size_t)B * 4, hipMemcpyDeviceToDevice, s)))) return rc;
    return rc_of(hipStreamSynchronize(s));
}

extern "C" size_t wt_dbg_dec_embed_scratch_bytes(int B, int ids_ld) {
    return B < 1 || ids_ld < 1 ? 0 : dbg_align(sizeof(DecState)) + dbg_align((size_t)B * ids_ld * 4);
}
extern "C" int wt_dbg_dec_embed(const int32_t* ids, int ids_ld, const int32_t* cur_len, const int32_t* pos, const void* tok_emb, int V,
                                const float* pos_emb, int pos_rows, int emb_half, float* x, int B, int d, void* scratch, void* stream) {
    if (!ids || !cur_len || !pos || !tok_emb || !pos_emb || !x || !scratch || B < 1 || B > MAX_ROWS || d < 4 || (d & 3) || ids_ld < 1) return -22;
    for (int b = 0; b < B; ++b) {
        if (cur_len[b] < 1 || cur_len[b] > ids_ld || pos[b] < 0 || pos[b] >= pos_rows) return -22;
        const int tok = ids[(size_t)b * ids_ld + cur_len[b] - 1];
        if (tok < 0 || tok >= V) return -22;
    }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    int* ids_dev = (int*)(base + dbg_align(sizeof(DecState)));
    DecState h;
    memset(&h, 0, sizeof h);
    for (int b = 0; b < B; ++b) {
        h.cur_len[b] = cur_len[b];
        h.pos[b] = pos[b];
    }
    int rc = rc_of(hipMemcpyAsync(ids_dev, ids, (size_t)B * ids_ld * 4, hipMemcpyHostToDevice, s));
    if (rc || (rc = upload_state(base, h, s))) return rc;
    return rc_of(launch_dec_embed(ids_dev, ids_ld, (const float*)tok_emb, pos_emb, x, B, d, (const DecState*)base, s, emb_half ? 1 : 0));
}

// ---- token-level timestamps: the post-pass launches on caller-supplied inputs, through the engine's TokTsParams ----
struct TtScratch { size_t W, mean, sdev, matrix, trace, total; };
static TtScratch tt_scratch_layout(int n_sel, int B, int N, int S) {
    TtScratch l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    l.W = take((size_t)n_sel * N * S * 4); l.mean = take((size_t)n_sel * S * 4); l.sdev = take((size_t)n_sel * S * 4);
    l.matrix = take((size_t)B * N * S * 4); l.trace = take((size_t)B * N * tt_trace_ld(S));
    l.total = off;
    return l;
}
static bool tt_dims_ok(int n_sel, int B, int N, int S) {
    return n_sel >= 1 && n_sel <= TT_MAX_HEADS && B >= 1 && B <= MAX_ROWS && N >= 1 && N <= TT_MAX_TOKENS && S >= 1 && S <= 4000;
}
extern "C" size_t wt_dbg_token_timestamps_scratch_bytes(int n_sel, int B, int N, int S) {
    return tt_dims_ok(n_sel, B, N, S) ? tt_scratch_layout(n_sel, B, N, S).total : 0;
}
static void tt_dbg_params(TokTsParams& p, int n_sel, int B, int N, int S, int width, void* scratch) {
    const TtScratch l = tt_scratch_layout(n_sel, B, N, S);
    char* base = (char*)scratch;
    memset(&p, 0, sizeof p);
    p.qh_rows = 1; p.qh_steps = N; p.cross_rows = 1; p.H = n_sel; p.S = S; p.n_sel = n_sel;
    for (int i = 0; i < n_sel; ++i) { p.layer[i] = 0; p.head[i] = i; }
    p.width = width; p.time_precision = 0.02; p.n_fixed = N; p.n_cap = N; p.B = B;
    p.W = (float*)(base + l.W); p.mean = (float*)(base + l.mean); p.sdev = (float*)(base + l.sdev); p.matrix = (float*)(base + l.matrix);
    p.trace = (uint8_t*)(base + l.trace); p.trace_ld = tt_trace_ld(S);
}
extern "C" int wt_dbg_token_timestamp_matrix_kernels(const float* q_hist, const void* K, int kv_half, int n_sel, int N, int S, int width, float* w_out,
                                                     float* matrix_out, void* scratch, void* stream) {
    if (!q_hist || !K || !matrix_out || !scratch || !tt_dims_ok(n_sel, 1, N, S) || width < 1 || width > TT_MAX_WIDTH || !(width & 1)) return -22;
    hipStream_t s = (hipStream_t)stream;
    TokTsParams p;
    tt_dbg_params(p, n_sel, 1, N, S, width, scratch);
    p.q_hist = q_hist; p.cross_k = K; p.kv_half = kv_half ? 1 : 0;
    int rc = rc_of(launch_tt_matrix(p, 0, s));
    if (rc) return rc;
    if (w_out && (rc = rc_of(hipMemcpyAsync(w_out, p.W, (size_t)n_sel * N * S * 4, hipMemcpyDeviceToDevice, s)))) return rc;
    return rc_of(hipMemcpyAsync(matrix_out, p.matrix, (size_t)N * S * 4, hipMemcpyDeviceToDevice, s));
}
extern "C" int wt_dbg_token_timestamp_median(const float* w_in, int n_sel, int N, int S, int width, float* matrix_out, void* scratch, void* stream) {
    if (!w_in || !matrix_out || !scratch || !tt_dims_ok(n_sel, 1, N, S) || width < 1 || width > TT_MAX_WIDTH || !(width & 1)) return -22;
    hipStream_t s = (hipStream_t)stream;
    TokTsParams p;
    tt_dbg_params(p, n_sel, 1, N, S, width, scratch);
    p.W = const_cast<float*>(w_in); p.mean = nullptr; p.sdev = nullptr;
    const int rc = rc_of(launch_tt_median(p, 0, s));
    if (rc) return rc;
    return rc_of(hipMemcpyAsync(matrix_out, p.matrix, (size_t)N * S * 4, hipMemcpyDeviceToDevice, s));
}
extern "C" int wt_dbg_token_timestamp_dtw(const float* matrix, int B, int N, int S, double time_precision, float* ts_out, int32_t* path_out,
                                          int32_t* path_len, void* scratch, void* stream) {
    if (!matrix || !ts_out || !path_out || !path_len || !scratch || !tt_dims_ok(1, B, N, S) || !(time_precision > 0.0)) return -22;
    TokTsParams p;
    tt_dbg_params(p, 1, B, N, S, 1, scratch);
    p.matrix = const_cast<float*>(matrix); p.time_precision = time_precision;
    p.path = path_out; p.path_len = path_len; p.out = ts_out; p.out_ld = N + 1;
    return rc_of(launch_tt_dtw(p, (hipStream_t)stream));
}

// ---- the prefill's own kernels (kernels_prefill.hip), as wt_decoder_begin launches them behind a prompt ----
extern "C" int wt_dbg_prefill_attention(const float* q, const float* kcache, const float* vcache, float* ctx, int B, int H, int nq, int nk, int cap,
                                        int ldq, int ldc, int causal, float q_scale, void* stream) {
    PrefillAttnParams a;
    memset(&a, 0, sizeof a);
    a.q = q; a.k = kcache; a.v = vcache; a.ctx = ctx; a.B = B; a.H = H; a.nq = nq; a.nk = nk; a.cap = cap; a.ldq = ldq; a.ldc = ldc;
    a.causal = causal ? 1 : 0; a.q_scale = q_scale;
    return rc_of(launch_prefill_attention(a, (hipStream_t)stream));
}
extern "C" int wt_dbg_prefill_query_finish(const float* u, const float* h1, const float* r, const float* t, float* q, int rows, int d, void* stream) {
    return rc_of(launch_prefill_query_finish(u, h1, r, t, q, rows, d, (hipStream_t)stream));
}

// ---- lang_select_kernel alone, built by the engine's own helper (wt_common.h: lang_select_params) ----
extern "C" size_t wt_dbg_lang_select_scratch_bytes(void) { return dbg_align((size_t)LANG_MAX * 4); }
extern "C" int wt_dbg_lang_select(const float* x, const float* ln_w, const float* ln_b, const void* emb, int emb_half, const int32_t* lang_ids,
                                  int n_lang, int V, int B, int d, int32_t* lang_tok, float* lang_prob, void* scratch, void* stream) {
    if (!x || !emb || !lang_ids || !lang_tok || !lang_prob || !scratch || (ln_w == nullptr) != (ln_b == nullptr)) return -22;
    if (B < 1 || B > MAX_ROWS || n_lang < 1 || n_lang > LANG_MAX || V < 1 || d < 4 || d > LANG_D_MAX || (d & 3)) return -22;
    for (int i = 0; i < n_lang; ++i)   // the kernel reads embedding row lang_ids[i]: inside the table
        if (lang_ids[i] < 0 || lang_ids[i] >= V) return -22;
    hipStream_t s = (hipStream_t)stream;
    int rc = rc_of(hipMemcpyAsync(scratch, lang_ids, (size_t)n_lang * 4, hipMemcpyHostToDevice, s));
    if (rc || (rc = rc_of(hipStreamSynchronize(s)))) return rc;   // (pageable source)
    const LangSelectParams p = lang_select_params(x, ln_w, ln_b, emb, emb_half, (const int*)scratch, n_lang, B, d, lang_tok, lang_prob);
    return rc_of(launch_lang_select(p, s));
}
