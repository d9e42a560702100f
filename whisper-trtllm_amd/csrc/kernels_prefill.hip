// Kernels of the decoder-prompt prefill (wt_decoder_set_prompt, DESIGN.md "Decoder prompts"): the positions of a prompt run through the
// decoder layers together, as GEMMs over M = B * len rows (launch_layernorm / launch_gemm_f32 of the encoder) and the attention below.
#include "wt_common.h"
#include <type_traits>

namespace wt {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ prefill attention
// softmax(q_scale . Q K^T) V per (utterance, head) with nq queries against the first nk keys of a head cache [rows][H][cap][64]:
// the causal form (self attention over the prompt: query t sees keys 0..t, nk == nq) and the full form (cross attention: every query
// sees keys 0..nk-1).  enc_attn_kernel's structure (kernels_encoder.hip): one workgroup = 128 queries (4 waves x 32), K/V tiles of 64
// keys double-buffered in LDS, both products on v_mfma_f32_32x32x2_f32 in the TRANSPOSED orientation
//   S^T[key][query] = K . Q^T,   O^T[dv][query] += V^T . P^T
// so that a query's scores sit in one lane (pair) and the online softmax is lane-local.  What differs: Q has its own pointer and leading
// dimension, K and V rows of a head are contiguous (256 B per key), nq != nk, the causal limit, and q_scale is an argument.
// Masking is confined to the tiles that need it (block-uniform): the ragged last tile, and in the causal form the tiles at or behind the
// block's first query.  Key 0 is visible to every query, so no row is ever fully masked and the running maximum is finite after tile 0.
// Loads are clamped to row nk - 1 / query nq - 1: nothing behind the valid keys or queries is ever read.
constexpr int PA_BQ = 128, PA_BKV = 64, PA_LD = 68;
constexpr int PA_SMEM = 2 * 2 * PA_BKV * PA_LD * (int)sizeof(float);  // 69,632 B

template <bool CAUSAL>
__global__ __launch_bounds__(256, 2) void prefill_attn_kernel(const PrefillAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int nq = p.nq, nk = p.nk, H = p.H;
    const int nqb = (nq + PA_BQ - 1) / PA_BQ;
    // consecutive workgroups = the query blocks of one (utterance, head), then the next head
    const int bh = blockIdx.x / nqb, b = bh / H, h = bh - b * H, q0 = (blockIdx.x - bh * nqb) * PA_BQ;
    const float* kbase = p.k + ((size_t)b * H + h) * p.cap * HEAD_DIM;
    const float* vbase_g = p.v + ((size_t)b * H + h) * p.cap * HEAD_DIM;

    // Q fragment (B operand of S^T): lane (query, half hh) holds Q[query][8q+4hh .. +3], pre-scaled
    const int qrow = q0 + wave * 32 + l31, qrow_c = min(qrow, nq - 1);
    f32x4 qf[8];
    {
        const float* qp = p.q + ((size_t)b * nq + qrow_c) * p.ldq + h * HEAD_DIM + 4 * hh;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            qf[q] = *reinterpret_cast<const f32x4*>(qp + 8 * q);
            qf[q] *= p.q_scale;
        }
    }
    // the last key this lane's query may see
    const int key_last = CAUSAL ? min(qrow_c, nk - 1) : nk - 1;
    // keys the block needs, and the tiles in front that no lane of the block has to mask
    const int nkeys = CAUSAL ? min(nk, q0 + PA_BQ) : nk;
    const int ntiles = (nkeys + PA_BKV - 1) / PA_BKV;
    const int nplain = min(CAUSAL ? q0 / PA_BKV : nk / PA_BKV, ntiles);

    // staging map: 64 keys x 16 float4 per matrix; thread -> column c4, rows r0 + 16*i (named vectors, not arrays: see enc_attn_kernel)
    const int c4 = tid & 15, r0 = tid >> 4;
    f32x4 rk0, rk1, rk2, rk3, rv0, rv1, rv2, rv3;
#define PA_GLOAD(kv0_)                                                                   \
    do {                                                                                 \
        const size_t o0_ = (size_t)min((kv0_) + r0, nk - 1) * HEAD_DIM + c4 * 4;         \
        const size_t o1_ = (size_t)min((kv0_) + r0 + 16, nk - 1) * HEAD_DIM + c4 * 4;    \
        const size_t o2_ = (size_t)min((kv0_) + r0 + 32, nk - 1) * HEAD_DIM + c4 * 4;    \
        const size_t o3_ = (size_t)min((kv0_) + r0 + 48, nk - 1) * HEAD_DIM + c4 * 4;    \
        rk0 = *reinterpret_cast<const f32x4*>(kbase + o0_); rv0 = *reinterpret_cast<const f32x4*>(vbase_g + o0_); \
        rk1 = *reinterpret_cast<const f32x4*>(kbase + o1_); rv1 = *reinterpret_cast<const f32x4*>(vbase_g + o1_); \
        rk2 = *reinterpret_cast<const f32x4*>(kbase + o2_); rv2 = *reinterpret_cast<const f32x4*>(vbase_g + o2_); \
        rk3 = *reinterpret_cast<const f32x4*>(kbase + o3_); rv3 = *reinterpret_cast<const f32x4*>(vbase_g + o3_); \
    } while (0)
#define PA_LSTORE(buf_)                                                                  \
    do {                                                                                 \
        float* Ks_ = smem + (buf_) * (2 * PA_BKV * PA_LD) + r0 * PA_LD + c4 * 4;         \
        float* Vs_ = Ks_ + PA_BKV * PA_LD;                                               \
        *reinterpret_cast<f32x4*>(Ks_) = rk0; *reinterpret_cast<f32x4*>(Vs_) = rv0;      \
        *reinterpret_cast<f32x4*>(Ks_ + 16 * PA_LD) = rk1; *reinterpret_cast<f32x4*>(Vs_ + 16 * PA_LD) = rv1; \
        *reinterpret_cast<f32x4*>(Ks_ + 32 * PA_LD) = rk2; *reinterpret_cast<f32x4*>(Vs_ + 32 * PA_LD) = rv2; \
        *reinterpret_cast<f32x4*>(Ks_ + 48 * PA_LD) = rk3; *reinterpret_cast<f32x4*>(Vs_ + 48 * PA_LD) = rv3; \
    } while (0)

    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    PA_GLOAD(0);
    PA_LSTORE(0);
    __syncthreads();
    // One 64-key tile.  MASK (compile-time: the compare + select per score is paid only where a lane can need it): keys behind key_last get
    // probability 0.  `more` (block-uniform): another tile follows, its global loads fly under this tile's products.
    auto tile = [&](auto MASK_T, const int t, const bool more) {
        constexpr bool MASK = decltype(MASK_T)::value;
        const int cur = t & 1, kv0 = t * PA_BKV;
        if (more) PA_GLOAD(kv0 + PA_BKV);
        const float* Ks = smem + cur * (2 * PA_BKV * PA_LD);
        const float* Vs = Ks + PA_BKV * PA_LD;

        f32x16 s0, s1;
        const float* kp = Ks + l31 * PA_LD + 4 * hh;
        f32x4 kf0[8], kf1[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            kf0[q] = *reinterpret_cast<const f32x4*>(kp + 8 * q);
            kf1[q] = *reinterpret_cast<const f32x4*>(kp + 32 * PA_LD + 8 * q);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q + 2 < 8) {
                kf0[q + 2] = *reinterpret_cast<const f32x4*>(kp + 8 * (q + 2));
                kf1[q + 2] = *reinterpret_cast<const f32x4*>(kp + 32 * PA_LD + 8 * (q + 2));
            }
            const f32x4 k0 = kf0[q], k1 = kf1[q], qq = qf[q];
            if (q == 0) {
                const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[0], qq[0], zero16, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[0], qq[0], zero16, 0, 0, 0);
            } else {
                s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[0], qq[0], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[0], qq[0], s1, 0, 0, 0);
            }
            s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[1], qq[1], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[1], qq[1], s1, 0, 0, 0);
            s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[2], qq[2], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[2], qq[2], s1, 0, 0, 0);
            s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[3], qq[3], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[3], qq[3], s1, 0, 0, 0);
        }
        if (MASK) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {   // S^T accumulator: register r of lane half hh is key (r & 3) + 8 (r >> 2) + 4 hh of the 32-key block
                const int key = kv0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (key > key_last) s0[r] = -INFINITY;
                if (key + 32 > key_last) s1[r] = -INFINITY;
            }
        }
        float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        // (a masked tile may hold no visible key for this query: mx = -inf, and m_run is finite by then -- tile 0 holds key 0)
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = __expf(s0[r] - m_new);
            s1[r] = __expf(s1[r] - m_new);
            ps += s0[r] + s1[r];
        }
        l_run = l_run * alpha + ps;  // per-lane partial (half of the query's keys per tile); the halves are merged at the end
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o0[r] *= alpha;
            o1[r] *= alpha;
        }
        const float* vb = Vs + 4 * hh * PA_LD + l31;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float va[4], vc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                va[i] = vb[(8 * g + i) * PA_LD];
                vc[i] = vb[(8 * g + i) * PA_LD + 32];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[i], s0[4 * g + i], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[i], s0[4 * g + i], o1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float va[4], vc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                va[i] = vb[(32 + 8 * g + i) * PA_LD];
                vc[i] = vb[(32 + 8 * g + i) * PA_LD + 32];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[i], s1[4 * g + i], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[i], s1[4 * g + i], o1, 0, 0, 0);
            }
        }
        if (more) PA_LSTORE(cur ^ 1);
        __syncthreads();
    };
    for (int t = 0; t < nplain; ++t) tile(std::false_type{}, t, t + 1 < ntiles);
    for (int t = nplain; t < ntiles; ++t) tile(std::true_type{}, t, t + 1 < ntiles);
#undef PA_GLOAD
#undef PA_LSTORE
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
    if (qrow < nq) {
        float* op = p.ctx + ((size_t)b * nq + qrow) * p.ldc + h * HEAD_DIM + 4 * hh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<float4*>(op + 8 * g) = make_float4(o0[4 * g + 0] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4*>(op + 32 + 8 * g) =
                make_float4(o1[4 * g + 0] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
}

hipError_t launch_prefill_attention(const PrefillAttnParams& p, hipStream_t s) {
    if (p.B < 1 || p.H < 1 || p.nq < 1 || p.nk < 1 || p.nk > p.cap || (p.causal && p.nk != p.nq)) return hipErrorInvalidValue;
    if (p.ldq < p.H * HEAD_DIM || p.ldc < p.H * HEAD_DIM || (p.ldq & 3) || (p.ldc & 3)) return hipErrorInvalidValue;
    if (((uintptr_t)p.q & 15) || ((uintptr_t)p.k & 15) || ((uintptr_t)p.v & 15) || ((uintptr_t)p.ctx & 15)) return hipErrorInvalidValue;
    const long long blocks = (long long)p.B * p.H * ((p.nq + PA_BQ - 1) / PA_BQ);
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    static PerDeviceFlag attr_set;
    if (!attr_set.get()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(prefill_attn_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, PA_SMEM);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(prefill_attn_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, PA_SMEM);
        if (e != hipSuccess) return e;
        attr_set.set();
    }
    if (p.causal) hipLaunchKernelGGL(prefill_attn_kernel<true>, dim3((unsigned)blocks), dim3(256), PA_SMEM, s, p);
    else hipLaunchKernelGGL(prefill_attn_kernel<false>, dim3((unsigned)blocks), dim3(256), PA_SMEM, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ folded cross query, finished per row
// q[m] = (u[m] - mean(h1[m]) . r) * rstd(h1[m]) + t  -- what dec_attn_kernel does to its one query row per block (two-pass statistics,
// eps 1e-5), here for M rows ahead of the prefill's cross attention.  One wave per row, d <= 1280.
__device__ __forceinline__ float pf_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__global__ __launch_bounds__(256) void prefill_query_finish_kernel(const float* __restrict__ u, const float* __restrict__ h1,
                                                                   const float* __restrict__ r, const float* __restrict__ t,
                                                                   float* __restrict__ q, int rows, int d) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4* hr = reinterpret_cast<const float4*>(h1 + (size_t)row * d);
    const int n4 = d >> 2;
    float4 v[5];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < n4 ? hr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = pf_wave_sum(s) / d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int c = lane + 64 * i;
        if (c < n4) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            sq += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    const float rstd = rsqrtf(pf_wave_sum(sq) / d + 1e-5f);
    const float4* u4 = reinterpret_cast<const float4*>(u + (size_t)row * d);
    const float4* r4 = reinterpret_cast<const float4*>(r);
    const float4* t4 = reinterpret_cast<const float4*>(t);
    float4* q4 = reinterpret_cast<float4*>(q + (size_t)row * d);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int c = lane + 64 * i;
        if (c < n4) {
            const float4 uu = u4[c], rr = r4[c], tt = t4[c];
            q4[c] = make_float4((uu.x - mean * rr.x) * rstd + tt.x, (uu.y - mean * rr.y) * rstd + tt.y, (uu.z - mean * rr.z) * rstd + tt.z,
                                (uu.w - mean * rr.w) * rstd + tt.w);
        }
    }
}
hipError_t launch_prefill_query_finish(const float* u, const float* h1, const float* r, const float* t, float* q, int rows, int d, hipStream_t s) {
    if (rows < 1 || d > 1280 || (d & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefill_query_finish_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, u, h1, r, t, q, rows, d);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ prompt embedding, state
// x[b * len + t] = embed_tokens[prompt(b)[t]] + embed_positions[t]; prompt(b) = row b of `prompt` [n_rows][len], or row 0 when n_rows == 1
__global__ __launch_bounds__(256) void prefill_embed_kernel(const int* __restrict__ prompt, int n_rows, int len, const float* __restrict__ tok_emb,
                                                            const float* __restrict__ pos_emb, float* __restrict__ x, int d) {
    const int m = blockIdx.x, b = m / len, t = m - b * len;
    const int tok = prompt[(size_t)(n_rows == 1 ? 0 : b) * len + t];
    const float4* te = reinterpret_cast<const float4*>(tok_emb + (size_t)tok * d);
    const float4* pe = reinterpret_cast<const float4*>(pos_emb + (size_t)t * d);
    float4* xo = reinterpret_cast<float4*>(x + (size_t)m * d);
    for (int i = threadIdx.x; i < (d >> 2); i += 256) {
        const float4 a = te[i], c = pe[i];
        xo[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}
hipError_t launch_prefill_embed(const int* prompt, int n_rows, int len, const float* tok_emb, const float* pos_emb, float* x, int B, int d,
                                hipStream_t s) {
    if (B < 1 || len < 1 || (d & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefill_embed_kernel, dim3((unsigned)(B * len)), dim3(256), 0, s, prompt, n_rows, len, tok_emb, pos_emb, x, d);
    return hipGetLastError();
}

// after launch_dec_init: row b of the id buffer = prompt(b), start token; the state behind a prompt of `len` tokens whose keys and values
// lie in the self caches (cur_len = len + 1, pos = len, self_len = len; step stays 0)
__global__ void prefill_state_kernel(DecState* st, int* ids, const int* __restrict__ prompt, int n_rows, int len, int B, int max_length,
                                     int start_token) {
    const int t = threadIdx.x;
    if (t < MAX_ROWS) {
        st->cur_len[t] = len + 1;
        st->pos[t] = len;
        st->self_len[t] = len;
    }
    if (t == 0) st->done = len + 1 >= max_length ? 1 : 0;
    for (int i = t; i < B * (len + 1); i += blockDim.x) {
        const int b = i / (len + 1), j = i - b * (len + 1);
        ids[(size_t)b * max_length + j] = j < len ? prompt[(size_t)(n_rows == 1 ? 0 : b) * len + j] : start_token;
    }
}
hipError_t launch_prefill_state(DecState* st, int* ids, const int* prompt, int n_rows, int len, int B, int max_length, int start_token,
                                hipStream_t s) {
    if (B < 1 || B > MAX_ROWS || len < 1 || len + 1 > max_length) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefill_state_kernel, dim3(1), dim3(256), 0, s, st, ids, prompt, n_rows, len, B, max_length, start_token);
    return hipGetLastError();
}

// The ragged form (wt_decoder_set_prompt_rows): row b holds lens[b] <= len prompt tokens, `prompt` [B][len] is right-padded (the layout the
// prefill pass computes over).  The id row is left-padded -- pad x (len - lens[b]), prompt(b), start token -- so that cur_len = len + 1 stays
// batch-wide and every rule that keys on it is untouched; pos and self_len are the row's own: its start token sits at decoder position
// lens[b], behind lens[b] valid keys (the filler's keys in cache rows lens[b]..len-1 are overwritten step by step before they are read).
__global__ void prefill_state_rows_kernel(DecState* st, int* ids, const int* __restrict__ prompt, const int* __restrict__ lens, int len, int B,
                                          int max_length, int start_token, int pad) {
    const int t = threadIdx.x;
    if (t < MAX_ROWS) {
        const int n = t < B ? min(max(lens[t], 0), len) : len;
        st->cur_len[t] = len + 1;
        st->pos[t] = n;
        st->self_len[t] = n;
    }
    if (t == 0) st->done = len + 1 >= max_length ? 1 : 0;
    for (int i = t; i < B * (len + 1); i += blockDim.x) {
        const int b = i / (len + 1), j = i - b * (len + 1), lead = len - min(max(lens[b], 0), len);
        ids[(size_t)b * max_length + j] = j < lead ? pad : j < len ? prompt[(size_t)b * len + (j - lead)] : start_token;
    }
}
hipError_t launch_prefill_state_rows(DecState* st, int* ids, const int* prompt, const int* lens, int len, int B, int max_length, int start_token,
                                     int pad, hipStream_t s) {
    if (B < 1 || B > MAX_ROWS || len < 1 || len + 1 > max_length || !lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefill_state_rows_kernel, dim3(1), dim3(256), 0, s, st, ids, prompt, lens, len, B, max_length, start_token, pad);
    return hipGetLastError();
}

}  // namespace wt
