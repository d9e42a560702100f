// Decoder-step HIP kernels for gfx950 (MI355X).  One greedy step over a batch of B utterances is
//   embed -> per layer { LN+QKV skinny GEMM (+ in-place self-KV append) -> self decode-attention ->
//   out-proj (+residual) -> LN+q skinny GEMM -> cross decode-attention -> out-proj (+residual) ->
//   LN+fc1+GELU -> fc2 (+residual) } -> final LN + vocabulary projection -> logits processors + argmax.
// Every kernel is HBM-bound (weights streamed once per step for the whole batch, K/V streamed once per
// utterance), so the design rules are: 16-byte coalesced loads straight to registers, many loads in flight,
// wave-level reductions with v_permlane32_swap / v_permlane16_swap / DPP, and no step-dependent kernel
// arguments (the step counters live in DecState) so a single hipGraph replays for every token.
//
// Reference semantics: tensorrt_llm/models/whisper/model.py:153-304 (WhisperDecoderAttention),
// :306-369 (WhisperDecoderLayer), :407-470 (WhisperDecoder.forward); greedy loop examples/whisper/run.py:171-227;
// processors HF generation/logits_process.py:1281-1328.  Numerics follow the HF oracle.
#include "wt_common.h"
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include <type_traits>

namespace wt {

__device__ __forceinline__ float gelu_erf_d(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// sum over the 16 lanes of a DPP row; every lane of the row ends with the total
__device__ __forceinline__ float row16_allreduce_sum(float v) {
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x121, 0xf, 0xf, false));  // row_ror:1
    return v;
}
__device__ __forceinline__ float wave_allreduce_sum_d(float v) {
    v = row16_allreduce_sum(v);  // every lane now holds the sum of its 16-lane row; add the four rows via SGPRs
    const float r0 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 0));
    const float r1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 16));
    const float r2 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 32));
    const float r3 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 48));
    return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}

// ------------------------------------------------------------------------------------------------ embed
// x[b] = embed_tokens[ids[b][cur_len-1]] + embed_positions[pos]      (model.py:423-425; HF :1149-1156)
// fp16 decoder engines keep embed_tokens (tied to the vocabulary projection) in fp16; embed_positions stays fp32.
__device__ __forceinline__ float4 load_emb4(const float* tab, size_t elem, const bool half) {
    if (!half) return *reinterpret_cast<const float4*>(tab + elem);
    const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(tab) + elem);
    const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&r.x)), b = __half22float2(*reinterpret_cast<const __half2*>(&r.y));
    return make_float4(a.x, a.y, b.x, b.y);
}
__global__ __launch_bounds__(256) void dec_embed_kernel(const int* __restrict__ ids, int ids_ld,
                                                        const float* __restrict__ tok_emb,
                                                        const float* __restrict__ pos_emb, float* __restrict__ x, int d,
                                                        const DecState* __restrict__ st, int emb_half) {
    const int b = blockIdx.x;
    const int tok = ids[(size_t)b * ids_ld + st->cur_len[b] - 1];
    const float4* pe = reinterpret_cast<const float4*>(pos_emb + (size_t)st->pos[b] * d);
    float4* xo = reinterpret_cast<float4*>(x + (size_t)b * d);
    for (int i = threadIdx.x; i < (d >> 2); i += 256) {
        const float4 a = load_emb4(tok_emb, (size_t)tok * d + 4 * i, emb_half != 0), c = pe[i];
        xo[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}
hipError_t launch_dec_embed(const int* ids, int ids_ld, const float* tok_emb, const float* pos_emb, float* x, int B,
                            int d, const DecState* st, hipStream_t s, int emb_half) {
    hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(256), 0, s, ids, ids_ld, tok_emb, pos_emb, x, d, st, emb_half);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ skinny GEMM
// y[b][n] = epi(sum_k X(b)[k] W[n][k] + bias[n]) for NB <= 16 batch rows: W is streamed from HBM exactly once.
// A wave owns a K-slice of <= 256*V columns: its slice of all NB activation rows stays in registers for the life of the
// kernel (NB x V float4; V = 4 for NB <= 8, V = 2 for NB = 16), W rows arrive as coalesced 1 KiB wave loads (float4
// per lane), two rows per iteration with the next pair prefetched.  The 2*NB per-lane partial sums are reduced
// across the wave by a halving butterfly (v_permlane32_swap, v_permlane16_swap, then DPP row rotations), leaving
// each (row, batch) total in one lane, which applies the epilogue.  When K exceeds a slice, the NW waves of a block
// split K (nsplit = 2, 4 or 8) and combine through LDS.  Whole activation rows (K <= 1024) are staged -- and
// LayerNorm-ed -- once per block through LDS.
// WH (fp16 decoder engines, build_decoder.py --engine_precision float16): W is IEEE half, everything else (activations, accumulation,
// LayerNorm, epilogue) stays fp32.  A lane's 16-byte load then carries EIGHT columns, so the slice chunk map becomes
// column(v) = ks0 + 8*lane + 512*(v>>1) + 4*(v&1): the same 256*V columns per wave, the same activation registers and the same K-split
// plan as the fp32 form, half the weight bytes per row (V/2 loads of 1 KiB per wave and row); the halves are widened with
// v_cvt_f32_f16 right before the packed FMAs.
// GELU_IN: PROBE ONLY (wt_dbg_skinny_gelu_in): the consumer side of "fold the cross out-projection through LN3 into
// fc1" -- fc2 would have to finish x = gelu((u - mean.r).rstd + t) on its own activation slice.  Timing only (statistics are stand-ins).
// LP (log-probability mode, ARGMAX only; wt_decoder_set_logprobs): 1 = every output lane also keeps the online log-sum-exp pair of its masked
// scores, 2 = and a second pair over the raw logits (no_speech_prob); merged per workgroup through the LDS stage of the candidates, in a
// fixed order, and written beside am_val / am_idx with one vector store.  A compile-time form: the LP = 0 instantiations are untouched.
// SAMP (temperature sampling, with LP != 0; wt_decoder_set_sampling): the running argmax compares the Gumbel-max key s / T + g (sample_key)
// instead of the score s and keeps the winner's s beside it; both go through the candidates' LDS stage.  The pairs are those of s, unchanged.
template <int NB, int V, int NW, bool W_NT, bool HALF = false, bool ARGMAX = false, bool WH = false, bool GELU_IN = false, int LP = 0,
          bool SAMP = false>
__device__ __forceinline__ void skinny_body(const SkinnyParams& p, const int nsplit, const int KS, const int rows_per_group,
                                            const int block) {
    extern __shared__ __attribute__((aligned(16))) float sk_smem[];
    float(*xs)[1024] = reinterpret_cast<float(*)[1024]>(sk_smem);                       // [NB][1024]
    float(*comb)[NW][2 * NB] = reinterpret_cast<float(*)[NW][2 * NB]>(sk_smem + NB * 1024);  // [2][NW][2*NB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = NW / nsplit;
    const int sp = wave % nsplit, grp = wave / nsplit;
    const int ks0 = sp * KS;                       // first column of this wave's slice
    const int kend = min(p.K, ks0 + KS);           // one past its last column
    const long long group_id = (long long)block * G + grp;
    const int row_begin = (int)min((long long)p.N, group_id * rows_per_group);
    const int row_end = min(p.N, row_begin + rows_per_group);

    static_assert(!WH || (V % 2) == 0, "half weights: two activation chunks per 16-byte load");
    constexpr int VW = WH ? V / 2 : V;             // 16-byte weight loads per row and lane
    constexpr int WSZ = WH ? 2 : 4;                // bytes per weight element
    auto colu = [&](const int v) { return WH ? ks0 + 8 * lane + 512 * (v >> 1) + 4 * (v & 1) : ks0 + 4 * lane + 256 * v; };
    float4 xr[NB][V];
    bool kok[V];
#pragma unroll
    for (int v = 0; v < V; ++v) kok[v] = colu(v) < kend;
    // ---- stream W ----------------------------------------------------------------------------------------------
    // Every load below is UNCONDITIONAL from a clamped address, with out-of-range lanes zeroed afterwards: a predicated
    // load (`ok ? *p : 0`) compiles to an exec-masked branch whose merge copy makes the compiler wait for vmcnt(0) in the
    // middle of the request burst -- one full HBM round trip before the remaining loads are even issued.
    int kcol[V];   // this lane's column of slice chunk v, clamped into the slice (half weights: the 8-column load is clamped as a whole)
#pragma unroll
    for (int v = 0; v < V; ++v) kcol[v] = WH ? min(ks0 + 8 * lane + 512 * (v >> 1), kend - 8) + 4 * (v & 1) : min(colu(v), kend - 4);
    typedef float f4v __attribute__((ext_vector_type(4)));   // 16 raw bytes: four floats, or eight halves
    f4v wbuf[2][2][VW];
    auto wload = [&](int buf, int row) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const char* wp = reinterpret_cast<const char*>(p.W) + (size_t)min(row + r, p.N - 1) * p.K * WSZ;
#pragma unroll
            for (int c = 0; c < VW; ++c) {
                const f4v* src = reinterpret_cast<const f4v*>(wp + (size_t)kcol[WH ? 2 * c : c] * WSZ);
                if (W_NT) wbuf[buf][r][c] = __builtin_nontemporal_load(src);  // weights are read exactly once per step: streaming loads
                else wbuf[buf][r][c] = *src;
            }
        }
    };
    auto wget = [&](const int buf, const int r, const int v) -> float4 {   // the four weights that meet activation chunk v
        if constexpr (WH) {
            typedef _Float16 h2v __attribute__((ext_vector_type(2)));
            const f4v raw = wbuf[buf][r][v >> 1];
            // (copies first: __builtin_bit_cast applied directly to a vector-element expression `raw[i]` reads element 0 with this clang)
            const float f0 = raw[2 * (v & 1)], f1 = raw[2 * (v & 1) + 1];
            const h2v lo = __builtin_bit_cast(h2v, f0), hi = __builtin_bit_cast(h2v, f1);
            return make_float4((float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]);
        } else {
            const f4v raw = wbuf[buf][r][v];
            return make_float4(raw[0], raw[1], raw[2], raw[3]);
        }
    };
    // W values of clamped (out-of-slice) lanes are multiplied by activations that ARE zeroed below, so they need no fix-up
    // which (row, batch) total this lane ends up holding after the butterfly
    const int rho = lane >> 4, li = lane & 15;
    const int my_r = rho >> 1;
    const int my_b = li + (rho & 1) * (NB / 2);
    const bool is_out_lane = li < NB / 2;
    // The epilogue operands of the FIRST row pair (bias, residual element, append position) are requested before anything
    // else: loaded where they are used they were two dependent L2 round trips at the very end of every launch
    // (in-kernel timestamps: ~0.8 us between "weights landed" and "stores issued" for 128 packed FMAs and a butterfly).
    float bias_pf = 0.f, resid_pf = 0.f;
    int self_len_pf = 0;
    {
        const int n_pf = min(row_begin + my_r, p.N - 1), b_pf = min(my_b, p.B - 1);
        if (p.bias) bias_pf = p.bias[n_pf];
        if (p.ymode == YMODE_PLAIN) {
            if (p.resid) resid_pf = p.resid[(size_t)b_pf * p.N + n_pf];
        } else if (!ARGMAX && p.ymode == YMODE_QKV_APPEND) {
            self_len_pf = p.st->self_len[b_pf];
        }
    }

    // ---- activation slice -> registers -------------------------------------------------------------------
    // vmcnt retires in issue order, so whatever is requested first is waited for first: with LDS staging the activation
    // rows go out before the first W rows.  (Measured neutral either way: the rows were written by the previous kernel on
    // other XCDs, so they arrive from the memory side together with the first weights, ~1.6-2.2 us after the start;
    // the LayerNorm + staging + barrier that follow are ~0.4-1 us of the launch -- DESIGN.md, timestamp study.)
    // `half_staged`: y = W . [a ; X2] where `a` is the merge of attention split partials (K/2 columns, staged + merged through LDS
    // like the plain `parts` case) and X2 is read directly: the folded cross-attention query behind a two-split self-attention.
    // (a compile-time switch: as a run-time branch it pushed every GEMV of the step into register spills -- 0.6-1 us each, 10 us on
    //  the vocabulary GEMV)
    constexpr bool half_staged = HALF;
    const int Ks = half_staged ? (p.K >> 1) : p.K;   // columns that go through the LDS staging
    const bool staged = half_staged || (p.K <= 1024 && !(p.xmode == XMODE_PLAIN && (p.x_direct || p.X2) && !p.parts));
    if (!staged && row_begin < row_end) wload(0, row_begin);
    if (staged) {
        // every wave of the block needs (a slice of) the same NB whole rows: stage them once per block through LDS.
        // Wave w loads (and LayerNorm-s) rows w and w + NW; after the barrier each wave pulls its slice of all rows.
        // (SJ rows per wave: two, or NB / NW where a block has fewer than NB / 2 waves -- the four-wave 16-row sampling form)
        constexpr int SJ = NB > 2 * NW ? NB / NW : 2;
        bool kfull[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) kfull[v] = (4 * lane + 256 * v) < Ks;
        // gamma/beta are requested together with the rows (not after the statistics) to keep them off the critical path
        float4 g[4], be[4];
        int fcol[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) fcol[v] = min(4 * lane + 256 * v, Ks - 4);
        if (p.xmode == XMODE_LAYERNORM) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                g[v] = *reinterpret_cast<const float4*>(p.ln_w + fcol[v]);
                be[v] = *reinterpret_cast<const float4*>(p.ln_b + fcol[v]);
            }
        }
        float4 xv[SJ][4];
        if (p.parts == nullptr) {
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const int b = min(wave + NW * j, p.B - 1);
#pragma unroll
                for (int v = 0; v < 4; ++v) xv[j][v] = *reinterpret_cast<const float4*>(p.X + (size_t)b * Ks + fcol[v]);
            }
            if (row_begin < row_end) wload(0, row_begin);
            __builtin_amdgcn_sched_barrier(0);  // all requests are in flight before the first fix-up below
        } else {
            // the activation row is the merge of the attention kernel's split partials (deferred from its tail: no ticket, no
            // write-through stores there).  Same operations in the same order as dec_attn_kernel's own merge -> same bits.
            // exactly two splits (launch_skinny checks): both partials of all 8 chunks are requested before the first use
            float4 o0[SJ][4], o1[SJ][4];
            float m0[SJ][4], m1[SJ][4], l0[SJ][4], l1[SJ][4];
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const int b = min(wave + NW * j, p.B - 1);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float* base = p.parts + ((size_t)b * p.parts_H + (fcol[v] >> 6)) * 2 * PART_STRIDE;
                    o0[j][v] = *reinterpret_cast<const float4*>(base + (fcol[v] & 63));
                    o1[j][v] = *reinterpret_cast<const float4*>(base + PART_STRIDE + (fcol[v] & 63));
                    m0[j][v] = base[64]; l0[j][v] = base[65];
                    m1[j][v] = base[PART_STRIDE + 64]; l1[j][v] = base[PART_STRIDE + 65];
                }
            }
            if (row_begin < row_end) wload(0, row_begin);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < SJ; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float Mg = fmaxf(fmaxf(-INFINITY, m0[j][v]), m1[j][v]);
                    const float w0 = __expf(m0[j][v] - Mg), w1 = __expf(m1[j][v] - Mg);
                    const float Lg = fmaf(w1, l1[j][v], fmaf(w0, l0[j][v], 0.f));
                    xv[j][v].x = fmaf(w1, o1[j][v].x, fmaf(w0, o0[j][v].x, 0.f)) / Lg;
                    xv[j][v].y = fmaf(w1, o1[j][v].y, fmaf(w0, o0[j][v].y, 0.f)) / Lg;
                    xv[j][v].z = fmaf(w1, o1[j][v].z, fmaf(w0, o0[j][v].z, 0.f)) / Lg;
                    xv[j][v].w = fmaf(w1, o1[j][v].w, fmaf(w0, o0[j][v].w, 0.f)) / Lg;
                }
        }
        if (p.xmode == XMODE_LAYERNORM) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (!kfull[v]) g[v] = be[v] = make_float4(0.f, 0.f, 0.f, 0.f);  // gamma = beta = 0 outside the row: padding lanes stay 0
        }
#pragma unroll
        for (int j = 0; j < SJ; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (!kfull[v] || wave + NW * j >= p.B) xv[j][v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < SJ; ++j) {
            const int b = wave + NW * j;
            if (b >= NB) break;
            if (p.xmode == XMODE_LAYERNORM) {
                float sum = 0.f;
#pragma unroll
                for (int v = 0; v < 4; ++v) sum += (xv[j][v].x + xv[j][v].y) + (xv[j][v].z + xv[j][v].w);
                const float mean = wave_allreduce_sum_d(sum) / Ks;
                float q = 0.f;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (kfull[v]) {
                        float a = xv[j][v].x - mean, c = xv[j][v].y - mean, e = xv[j][v].z - mean, f = xv[j][v].w - mean;
                        q += (a * a + c * c) + (e * e + f * f);
                    }
                const float rstd = rsqrtf(wave_allreduce_sum_d(q) / Ks + 1e-5f);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    xv[j][v].x = (xv[j][v].x - mean) * rstd * g[v].x + be[v].x;
                    xv[j][v].y = (xv[j][v].y - mean) * rstd * g[v].y + be[v].y;
                    xv[j][v].z = (xv[j][v].z - mean) * rstd * g[v].z + be[v].z;
                    xv[j][v].w = (xv[j][v].w - mean) * rstd * g[v].w + be[v].w;
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) *reinterpret_cast<float4*>(&xs[b][4 * lane + 256 * v]) = xv[j][v];
        }
        __syncthreads();
        if (half_staged && ks0 >= Ks) {  // this wave's K-slice lies in the X2 half (slices never straddle: KS divides K/2): straight from L2
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < V; ++v) xr[b][v] = *reinterpret_cast<const float4*>(p.X2 + (size_t)min(b, p.B - 1) * Ks + (kcol[v] - Ks));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < V; ++v)
                    if (!kok[v] || b >= p.B) xr[b][v] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < V; ++v)
                    xr[b][v] = kok[v] ? *reinterpret_cast<const float4*>(&xs[b][colu(v)]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        if (p.X2 == nullptr) {  // rows longer than the staging buffer (or x_direct): each wave loads its own K-slice straight from L2
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < V; ++v)
                    xr[b][v] = *reinterpret_cast<const float4*>(p.X + (size_t)min(b, p.B - 1) * p.K + kcol[v]);
        } else {  // concatenated activations [X ; X2], K/2 columns each (K/2 is a multiple of 4: a float4 never straddles)
            const int kh = p.K >> 1;
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const int col = kcol[v];
                    const float* src = col < kh ? p.X + (size_t)min(b, p.B - 1) * kh + col : p.X2 + (size_t)min(b, p.B - 1) * kh + (col - kh);
                    xr[b][v] = *reinterpret_cast<const float4*>(src);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (!kok[v] || b >= p.B) xr[b][v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (GELU_IN) {   // probe: what the folded-fc1 consumer would add in front of its products (128 GELUs per lane at K = 4096)
            float4 rr[V], tt[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                rr[v] = *reinterpret_cast<const float4*>(p.ln_w + kcol[v]);
                tt[v] = *reinterpret_cast<const float4*>(p.ln_b + kcol[v]);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float mean = p.bias[min(b, p.N - 1)] * 1e-3f, rstd = 1.0f + mean;   // stand-ins for the LayerNorm statistics of row b
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    xr[b][v].x = gelu_erf((xr[b][v].x - mean * rr[v].x) * rstd + tt[v].x);
                    xr[b][v].y = gelu_erf((xr[b][v].y - mean * rr[v].y) * rstd + tt[v].y);
                    xr[b][v].z = gelu_erf((xr[b][v].z - mean * rr[v].z) * rstd + tt[v].z);
                    xr[b][v].w = gelu_erf((xr[b][v].w - mean * rr[v].w) * rstd + tt[v].w);
                }
            }
        }
    }

    // ARGMAX (a compile-time mode: its state would push the plain GEMVs of the step into register spills): running masked maximum
    // of the rows this lane finishes (rows ascend, so the lowest index wins ties)
    float am_best = -INFINITY;
    int am_bidx = 0x7fffffff;
    uint8_t am_mk[2] = {0, 0};  // mask bytes of this lane's rows, requested one iteration ahead with the weights (a load in the
                                // epilogue would be an exposed L2 round trip per row pair: measured +10 us on the 51864-row GEMV)
    bool am_at_begin = false;
    float* am_tr = nullptr;
    float lp_m = -INFINITY, lp_s = 0.f, lp_rm = -INFINITY, lp_rs = 0.f;   // LP: (max, sum of exp) of the masked / of the raw scores
    static_assert(LP == 0 || ARGMAX, "the log-sum-exp pairs belong to the ARGMAX epilogue");
    static_assert(!SAMP || LP != 0, "sampling runs with the log-sum-exp pairs on");
    float am_sc = -INFINITY;                 // SAMP: score of the running winner (am_best is its key)
    unsigned long long sm_seed = 0;
    int sm_t = 0;
    if constexpr (SAMP) {
        sm_seed = p.am_seeds[min(my_b, p.B - 1)];
        sm_t = p.st->pos[min(my_b, p.B - 1)] + 1;   // the row's own sequence position (== cur_len unless the id rows are left-padded)
    }
    if constexpr (ARGMAX) {
        am_mk[0] = p.am_mask[min(row_begin + my_r, p.N - 1)];
        am_at_begin = p.st->cur_len[min(my_b, p.B - 1)] == p.am_begin_index;
        // raw-logits trace row of this step; steps enqueued past the stop test (st->done) or past the trace's last row must not write
        if (p.am_trace && !p.st->done && p.st->step < p.am_trace_steps)
            am_tr = p.am_trace + ((size_t)min(my_b, p.B - 1) * p.am_trace_steps + p.st->step) * p.N;
    }
    const int niter = (rows_per_group + 1) / 2;  // identical for every wave of the block (barriers below)
    // one iteration = two W rows; `cur` (static) is the register buffer holding them, the other one is prefetched
    auto body = [&](auto cur_c, const int it) {
        constexpr int cur = decltype(cur_c)::value;
        const int row = row_begin + 2 * it;
        const bool active = row < row_end;
        if (active && row + 2 < row_end) {
            wload(cur ^ 1, row + 2);
            if constexpr (ARGMAX) am_mk[cur ^ 1] = p.am_mask[min(row + 2 + my_r, p.N - 1)];
        }
        float out = 0.f;
        if (active) {
            float acc[2][NB];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    // packed fp32 FMA (v_pk_fma_f32): even and odd columns accumulate in the two halves of a register pair
                    typedef float f2v __attribute__((ext_vector_type(2)));
                    f2v a2 = f2v{0.f, 0.f};
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const float4 w = wget(cur, r, v);
                        a2 = __builtin_elementwise_fma(f2v{w.x, w.y}, f2v{xr[b][v].x, xr[b][v].y}, a2);
                        a2 = __builtin_elementwise_fma(f2v{w.z, w.w}, f2v{xr[b][v].z, xr[b][v].w}, a2);
                    }
                    acc[r][b] = a2[0] + a2[1];
                }
            // butterfly stage 1 (lanes l <-> l^32): lower half-wave keeps row 0, upper half-wave row 1
            float s1[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[0][b]), __float_as_uint(acc[1][b]), false, false);
                s1[b] = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
            }
            // stage 2 (l <-> l^16): even 16-lane rows keep batch b, odd rows batch b + NB/2
            float s2[NB / 2];
#pragma unroll
            for (int b = 0; b < NB / 2; ++b) {
                auto r2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1[b]), __float_as_uint(s1[b + NB / 2]), false, false);
                s2[b] = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
            }
            // stage 3: total over the 16 lanes of the row; lane li < NB/2 keeps value li
#pragma unroll
            for (int b = 0; b < NB / 2; ++b) {
                const float t = row16_allreduce_sum(s2[b]);
                if (li == b) out = t;
            }
        }
        float total = out;
        bool do_epi = active && is_out_lane;
        if (nsplit > 1) {
            if (do_epi) comb[cur][wave][my_r * NB + my_b] = out;
            __syncthreads();
            do_epi = do_epi && sp == 0;  // the first wave of each K-split group finishes its rows
            if (do_epi) {
                total = 0.f;
                for (int s = 0; s < nsplit; ++s) total += comb[cur][grp * nsplit + s][my_r * NB + my_b];
            }
        }
        const int n = row + my_r;
        if (do_epi && n < row_end && my_b < p.B) {
            float v = total + (it == 0 ? bias_pf : (p.bias ? p.bias[n] : 0.f));
            if constexpr (ARGMAX) {  // logits processors (Suppress -> SuppressAtBegin) + running argmax, logits_process.py:1281-1311
                v *= p.q_scale;
                if (am_tr) am_tr[n] = v;
                if constexpr (LP == 2) {
                    lse_add(lp_rm, lp_rs, v);
                    if (n == p.am_ns) p.am_side[2 * my_b + 1] = v;
                }
                const uint8_t mk = am_mk[cur];
                if ((mk & 1) || ((mk & 2) && am_at_begin)) v = -INFINITY;
                if constexpr (LP != 0) {
                    lse_add(lp_m, lp_s, v);
                    if (n == p.am_eos) p.am_side[2 * my_b] = v;
                }
                if constexpr (SAMP) {
                    unsigned dr[4];
                    sample_draws(sm_seed, sm_t, n >> 2, dr);
                    const int q = n & 3;
                    const float key = sample_key(v, p.am_temp, q == 0 ? dr[0] : q == 1 ? dr[1] : q == 2 ? dr[2] : dr[3]);
                    if (argmax_better(key, n, am_best, am_bidx)) {
                        am_best = key;
                        am_bidx = n;
                        am_sc = v;
                    }
                } else if (argmax_better(v, n, am_best, am_bidx)) {
                    am_best = v;
                    am_bidx = n;
                }
            } else if (p.ymode == YMODE_PLAIN) {
                v *= p.q_scale;
                if (p.act) v = gelu_erf_d(v);
                const size_t off = (size_t)my_b * p.N + n;
                if (p.resid) v += it == 0 ? resid_pf : p.resid[off];
                p.Y[off] = v;
            } else {  // fused q|k|v projection: q (scaled) -> Y, k/v rows appended in place at index self_len
                const int third = n / p.d_model, nn = n - third * p.d_model;
                if (third == 0) {
                    p.Y[(size_t)my_b * p.d_model + nn] = v * p.q_scale;
                } else {
                    const int h = nn >> 6, j = nn & 63, H = p.d_model >> 6;
                    float* cache = third == 1 ? p.kcache : p.vcache;
                    const size_t at = (((size_t)my_b * H + h) * p.s_cap + self_len_pf) * HEAD_DIM + j;
                    if (p.kv_half) reinterpret_cast<__half*>(cache)[at] = __float2half(v);   // fp16 engines: resident caches in fp16
                    else cache[at] = v;
                }
            }
        }
    };
    for (int it = 0; it < niter; it += 2) {
        body(std::integral_constant<int, 0>{}, it);
        if (it + 1 < niter) body(std::integral_constant<int, 1>{}, it + 1);
    }
    if constexpr (ARGMAX) {
        // one (max, argmax) per batch row and workgroup: output lanes -> LDS (the activation staging area is free by now) ->
        // thread b scans the NW x 2 candidates of batch row b in a fixed order
        __syncthreads();
        float* cv = sk_smem;                                 // [NW][2][NB]
        int* ci = reinterpret_cast<int*>(sk_smem + NW * 2 * NB);
        if (is_out_lane) {
            cv[(wave * 2 + my_r) * NB + my_b] = am_best;
            ci[(wave * 2 + my_r) * NB + my_b] = am_bidx;
        }
        float* cl = sk_smem + 2 * NW * 2 * NB;               // LP: [4][NW][2][NB] = m, s, raw m, raw s
        if constexpr (LP != 0) {
            if (is_out_lane) {
                const int at = (wave * 2 + my_r) * NB + my_b;
                cl[at] = lp_m;
                cl[NW * 2 * NB + at] = lp_s;
                if constexpr (LP == 2) {
                    cl[2 * NW * 2 * NB + at] = lp_rm;
                    cl[3 * NW * 2 * NB + at] = lp_rs;
                }
            }
        }
        float* cs = sk_smem + 6 * NW * 2 * NB;               // SAMP: [NW][2][NB] scores of the candidates
        if constexpr (SAMP) {
            if (is_out_lane) cs[(wave * 2 + my_r) * NB + my_b] = am_sc;
        }
        __syncthreads();
        if (tid < p.B) {
            float best = -INFINITY, bsc = -INFINITY;
            int bidx = 0x7fffffff;
            for (int i = 0; i < NW * 2; ++i) {
                const float v = cv[i * NB + tid];
                const int ix = ci[i * NB + tid];
                if (argmax_better(v, ix, best, bidx)) {
                    best = v;
                    bidx = ix;
                    if constexpr (SAMP) bsc = cs[i * NB + tid];
                }
            }
            p.am_val[(size_t)tid * p.am_ld + block] = best;
            p.am_idx[(size_t)tid * p.am_ld + block] = bidx;
            if constexpr (SAMP) p.am_sc[(size_t)tid * p.am_ld + block] = bsc;
            if constexpr (LP != 0) {   // the pairs of the NW x 2 output lanes of batch row `tid`, merged in slot order
                float m = -INFINITY, s = 0.f, rm = -INFINITY, rs = 0.f;
                for (int i = 0; i < NW * 2; ++i) {
                    lse_merge(m, s, cl[i * NB + tid], cl[NW * 2 * NB + i * NB + tid]);
                    if constexpr (LP == 2) lse_merge(rm, rs, cl[2 * NW * 2 * NB + i * NB + tid], cl[3 * NW * 2 * NB + i * NB + tid]);
                }
                p.am_lse[(size_t)tid * p.am_ld + block] = make_float4(m, s, rm, rs);
            }
        }
    }
}

struct SkinnyPlan {
    int nsplit, KS, rows_per_group, grid;
};

template <int NB, int V, int NW, bool W_NT, bool ARGMAX = false, bool WH = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void skinny_gemm_kernel(const SkinnyParams p, const int nsplit, const int KS,
                                                                             const int rows_per_group) {
    skinny_body<NB, V, NW, W_NT, false, ARGMAX, WH>(p, nsplit, KS, rows_per_group, blockIdx.x);
}
// the vocabulary GEMV of the log-probability mode: the ARGMAX epilogue with the log-sum-exp pairs (LP = 1) and the raw pair (LP = 2)
// (one block per SIMD set: the pairs push the 8-row form past 256 registers, and the vocabulary GEMV's plan is one block per CU anyway --
//  with two the compiler spilled 8-16 bytes per lane to scratch, a vector-memory access queued behind the weight loads)
template <int NB, int V, int NW, bool W_NT, bool WH, int LP>
__global__ __launch_bounds__(64 * NW, 1) void skinny_logprob_kernel(const SkinnyParams p, const int nsplit, const int KS,
                                                                                const int rows_per_group) {
    skinny_body<NB, V, NW, W_NT, false, true, WH, false, LP>(p, nsplit, KS, rows_per_group, blockIdx.x);
}
// the vocabulary GEMV of temperature sampling: the LP epilogue comparing Gumbel-max keys (SAMP), one block per SIMD set as above
template <int NB, int V, int NW, bool W_NT, bool WH, int LP>
__global__ __launch_bounds__(64 * NW, 1) void skinny_sample_kernel(const SkinnyParams p, const int nsplit, const int KS,
                                                                               const int rows_per_group) {
    skinny_body<NB, V, NW, W_NT, false, true, WH, false, LP, true>(p, nsplit, KS, rows_per_group, blockIdx.x);
}

// probe (see GELU_IN above): the K > 1024 direct-activation GEMV with the GELU / LayerNorm finish in its prologue
__global__ __launch_bounds__(256, 2) void skinny_gelu_in_probe_kernel(const SkinnyParams p, const int nsplit, const int KS, const int rows_per_group) {
    skinny_body<8, 4, 4, true, false, false, false, true>(p, nsplit, KS, rows_per_group, blockIdx.x);
}

// Two GEMMs that depend on the same predecessor share ONE launch (the self-attention out-projection and the folded
// cross-attention query): blocks [0, pa.grid) run `a`, the rest run `b`.  The branch is block-uniform.
template <int NB, int V, int NW, bool HALF_B, bool WH = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void skinny_pair_kernel(const SkinnyParams a, const SkinnyPlan pa,
                                                                             const SkinnyParams b, const SkinnyPlan pb) {
    if ((int)blockIdx.x < pa.grid) skinny_body<NB, V, NW, true, false, false, WH>(a, pa.nsplit, pa.KS, pa.rows_per_group, blockIdx.x);
    else skinny_body<NB, V, NW, true, HALF_B, false, WH>(b, pb.nsplit, pb.KS, pb.rows_per_group, blockIdx.x - pa.grid);
}

// The q|k|v launch with a passenger ("Hoisted residual half"): blocks [0, pa.grid) run `a` -- LayerNorm -> q|k|v -> append,
// the very instantiation and plan skinny_gemm_kernel runs it with, so q and the cache rows keep their bits -- and the rest run the plain
// GEMV `b` over the raw residual row (uh = fold_wh . h + fold_c) on compute units the q|k|v range leaves idle.  Block-uniform branch.
template <int NB, int V, int NW, bool W_NT, bool WH = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void skinny_hoist_kernel(const SkinnyParams a, const SkinnyPlan pa,
                                                                              const SkinnyParams b, const SkinnyPlan pb) {
    if ((int)blockIdx.x < pa.grid) skinny_body<NB, V, NW, W_NT, false, false, WH>(a, pa.nsplit, pa.KS, pa.rows_per_group, blockIdx.x);
    else skinny_body<NB, V, NW, W_NT, false, false, WH>(b, pb.nsplit, pb.KS, pb.rows_per_group, blockIdx.x - pa.grid);
}

// ---- launchers.  Every compile-time form of the kernels above is derived here once: the shape from the batch (skinny_for_batch), the
// boolean forms from the run-time flags (with_flags), the dynamic-LDS size from the shape, and the launch itself in skinny_launch.
// A shape: NB batch rows, V float4 activation chunks per lane and K-slice, NW waves per workgroup.
template <int NB_, int V_, int NW_>
struct SkinnyShape {
    static constexpr int NB = NB_, V = V_, NW = NW_;
    static constexpr int smem = (NB * 1024 + 2 * NW * 2 * NB) * (int)sizeof(float);   // dynamic LDS: xs[NB][1024] + comb[2][NW][2 * NB]
};

// The shape ladder: f(shape of batch B).  16 rows: half-width K-slices, 8 waves per block.
// SAMP (the shapes of the sampling forms): the 16-row sampling form runs FOUR waves per workgroup, not eight: one wave per SIMD has 512
// registers per lane, and with two (256 each, of which the log-probability variant already takes 254-256) the Philox rounds spilled
// 48-124 bytes per lane to scratch.  So every sampling shape is four waves wide, and <16, 2, 8> has no sampling form.
template <bool SAMP, class F>
static hipError_t skinny_for_batch(const int B, F&& f) {
    if (B <= 2) return f(SkinnyShape<2, 4, 4>{});
    if (B <= 4) return f(SkinnyShape<4, 4, 4>{});
    if (B <= 8) return f(SkinnyShape<8, 4, 4>{});
    if constexpr (SAMP) return f(SkinnyShape<16, 2, 4>{});
    else return f(SkinnyShape<16, 2, 8>{});
}
static bool skinny_sampling(const SkinnyParams& p) { return p.ymode == YMODE_ARGMAX && p.am_samp; }

// Run-time flags -> template arguments: with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...), and f
// names the one instantiation its arguments select.  Only f's body decides which forms exist.
template <class F>
static hipError_t with_flags(F&& f) { return f(); }
template <class F, class... Bs>
static hipError_t with_flags(F&& f, const bool b, const Bs... bs) {
    return b ? with_flags([&](auto... c) { return f(std::true_type{}, c...); }, bs...)
             : with_flags([&](auto... c) { return f(std::false_type{}, c...); }, bs...);
}

template <class S>
static hipError_t skinny_plan(const SkinnyParams& p, SkinnyPlan* out, int tg_override = 0) {
    constexpr int NB = S::NB, V = S::V, NW = S::NW;
    if (p.B < 1 || p.B > NB || (p.K & 3)) return hipErrorInvalidValue;
    int nsplit = (p.parts && p.X2) ? 2 : 1;   // half-staged: a wave's K-slice must not straddle the [a ; X2] seam
    while (p.K / nsplit > 256 * V || (p.K % nsplit)) {
        nsplit *= 2;
        if (nsplit > NW) return hipErrorInvalidValue;
    }
    const int KS = p.K / nsplit;
    if (KS & 3) return hipErrorInvalidValue;
    if (p.w_half && ((KS & 7) || (reinterpret_cast<uintptr_t>(p.W) & 15))) return hipErrorInvalidValue;   // eight halves per 16-byte load
    if (p.K > 1024 && p.xmode != XMODE_PLAIN) return hipErrorInvalidValue;  // LayerNorm needs whole rows staged in LDS
    if (p.X2 && (p.xmode != XMODE_PLAIN || (p.K & 7))) return hipErrorInvalidValue;
    if (p.parts && !p.X2 && (p.K > 1024 || p.K != p.parts_H * 64 || p.parts_nsplit != 2)) return hipErrorInvalidValue;
    if (p.parts && p.X2 && (p.K > 2048 || (p.K >> 1) != p.parts_H * 64 || p.parts_nsplit != 2 || (KS > (p.K >> 1)) || ((p.K >> 1) % KS))) return hipErrorInvalidValue;
    const int G = NW / nsplit;
    // row groups (waves x K-splits) per launch: measured per decode step at medium.en B = 8 -- 512: 1.64 ms, 768: 1.53, 1024: 1.475,
    // 1280: 1.478, 1536: 1.49, 2048: 1.51, 3072: 1.51.  1024 = one 4-wave block per CU, each wave streaming two row pairs with
    // the second pair prefetched behind the first (A/B knob: WT_SKINNY_TARGET)
    // (only the 8-row template: batch 16 measured 424 audio-s/s with 2048 and 398 with 1024; batch 1 / 2 / 4: 1.07 / 1.11 / 1.24 ms
    //  per step with 2048 and 1.09 / 1.12 / 1.27 with 1024; batch 6: 1.44 vs 1.41)
    static const int tg_total = tuning_env("WT_SKINNY_TARGET") ? atoi(tuning_env("WT_SKINNY_TARGET")) : (NB == 8 ? 1024 : 2048);
    const int target_groups = (tg_override > 0 ? tg_override : tg_total) / nsplit;
    int rows_per_group = 2 * ((p.N + 2 * target_groups - 1) / (2 * target_groups));
    if (rows_per_group < 2) rows_per_group = 2;
    const int groups = (p.N + rows_per_group - 1) / rows_per_group;
    out->nsplit = nsplit; out->KS = KS; out->rows_per_group = rows_per_group; out->grid = (groups + G - 1) / G;
    return hipSuccess;
}
// both halves of a two-GEMV launch, planned alike
template <class S>
static hipError_t skinny_plan2(const SkinnyParams& a, const SkinnyParams& b, SkinnyPlan* pa, SkinnyPlan* pb, int tg_override = 0) {
    const hipError_t e = skinny_plan<S>(a, pa, tg_override);
    return e == hipSuccess ? skinny_plan<S>(b, pb, tg_override) : e;
}

// The one place a skinny kernel is launched.  A shape that needs more than the default 48 KiB of dynamic LDS (16 rows) first has the
// limit of the very kernel about to run raised: once per device and kernel -- and harmlessly again by a thread that races the first, or
// under the thread-local stream capture of a step graph (the attribute is a property of the function, not a stream operation).
template <auto KERNEL, class S, class... Args>
static hipError_t skinny_launch(const int grid, hipStream_t s, const Args&... args) {
    if constexpr (S::smem > 48 * 1024) {
        static PerDeviceFlag attr_set;
        if (!attr_set.get()) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, S::smem);
            if (e != hipSuccess) return e;
            attr_set.set();
        }
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(64 * S::NW), S::smem, s, args...);
    return hipGetLastError();
}

template <class S, bool SAMP>
static hipError_t skinny_single(const SkinnyParams& p, hipStream_t s) {
    constexpr int NB = S::NB, V = S::V, NW = S::NW;
    SkinnyPlan pl;
    const hipError_t e = skinny_plan<S>(p, &pl);
    if (e != hipSuccess) return e;
    if constexpr (SAMP) {
        static_assert(7 * NW * 2 * NB <= NB * 1024, "candidates + four pair arrays + scores fit the activation staging area");
        if (!p.am_lp || !p.am_seeds || !p.am_sc || !(p.am_temp > 0.f)) return hipErrorInvalidValue;
        return with_flags([&](auto NT, auto WH, auto LP2) {
            return skinny_launch<skinny_sample_kernel<NB, V, NW, NT, WH, LP2 ? 2 : 1>, S>(pl.grid, s, p, pl.nsplit, pl.KS, pl.rows_per_group);
        }, p.w_nt, p.w_half, p.am_lp == 2);
    } else if (p.ymode == YMODE_ARGMAX && p.am_lp) {
        static_assert(6 * NW * 2 * NB <= NB * 1024, "candidates + four pair arrays fit the activation staging area");
        return with_flags([&](auto NT, auto WH, auto LP2) {
            return skinny_launch<skinny_logprob_kernel<NB, V, NW, NT, WH, LP2 ? 2 : 1>, S>(pl.grid, s, p, pl.nsplit, pl.KS, pl.rows_per_group);
        }, p.w_nt, p.w_half, p.am_lp == 2);
    } else {
        return with_flags([&](auto NT, auto AM, auto WH) {
            return skinny_launch<skinny_gemm_kernel<NB, V, NW, NT, AM, WH>, S>(pl.grid, s, p, pl.nsplit, pl.KS, pl.rows_per_group);
        }, p.w_nt, p.ymode == YMODE_ARGMAX, p.w_half);
    }
}

template <class S>
static hipError_t skinny_pair_cfg(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s) {
    SkinnyPlan pa, pb;
    hipError_t e = skinny_plan2<S>(a, b, &pa, &pb);
    // 8-wave workgroups (batch 9..16) are resident one per CU: a pair of more than 256 of them runs in two rounds, the second
    // half empty (measured 12.5 us per launch at medium.en batch 16 with 128 + 256 workgroups).  Re-plan both halves with fewer,
    // fatter row groups until the pair fits one round.
    if (S::NW == 8)
        for (int tg = 1024; e == hipSuccess && pa.grid + pb.grid > 256 && tg >= 256; tg >>= 1) e = skinny_plan2<S>(a, b, &pa, &pb, tg);
    if (e != hipSuccess) return e;
    if (a.parts && a.X2) return hipErrorInvalidValue;   // the half-staged form exists for the second GEMV of a pair only
    if (a.w_half != b.w_half) return hipErrorInvalidValue;
    return with_flags([&](auto HALF_B, auto WH) {
        return skinny_launch<skinny_pair_kernel<S::NB, S::V, S::NW, HALF_B, WH>, S>(pa.grid + pb.grid, s, a, pa, b, pb);
    }, b.parts && b.X2, a.w_half);
}

template <class S>
static hipError_t skinny_hoist_cfg(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s) {
    SkinnyPlan pa, pb;
    hipError_t e = skinny_plan2<S>(a, b, &pa, &pb);   // the q|k|v range: the plan launch_skinny gives it alone
    // The passenger takes the workgroups the q|k|v range leaves free in its last round over the 256 compute units: fewer, fatter row
    // groups until it fits (medium.en batch 8: 192 + 64 workgroups, every wave of either range streams four rows).  Row groups at most
    // four times the usual size; where even those do not fit (or the q|k|v range fills its rounds exactly: no such shape today) the
    // passenger keeps its usual plan and spills into another round.
    const int room = (pa.grid + 255) / 256 * 256;
    if (e == hipSuccess && pa.grid + pb.grid > room && room > pa.grid) {
        SkinnyPlan fat = pb;
        for (int tg = S::NB == 8 ? 512 : 1024; e == hipSuccess && pa.grid + fat.grid > room && tg >= 256; tg >>= 1) e = skinny_plan<S>(b, &fat, tg);
        if (e == hipSuccess && pa.grid + fat.grid <= room) pb = fat;
    }
    if (e != hipSuccess) return e;
    return with_flags([&](auto NT, auto WH) {
        return skinny_launch<skinny_hoist_kernel<S::NB, S::V, S::NW, NT, WH>, S>(pa.grid + pb.grid, s, a, pa, b, pb);
    }, a.w_nt, a.w_half);
}

hipError_t launch_skinny_gelu_in_probe(const SkinnyParams& p, hipStream_t s) {
    if (p.B < 1 || p.B > 8 || p.K <= 1024 || p.xmode != XMODE_PLAIN || !p.ln_w || !p.ln_b || !p.bias) return hipErrorInvalidValue;
    using S = SkinnyShape<8, 4, 4>;   // the probe's one form, whatever the batch
    SkinnyPlan pl;
    const hipError_t e = skinny_plan<S>(p, &pl);
    if (e != hipSuccess) return e;
    return skinny_launch<skinny_gelu_in_probe_kernel, S>(pl.grid, s, p, pl.nsplit, pl.KS, pl.rows_per_group);
}

int skinny_grid(const SkinnyParams& p) {  // workgroups launch_skinny will use for p (the column count of am_val / am_idx)
    SkinnyPlan pl;
    const auto plan = [&](auto sh) { return skinny_plan<decltype(sh)>(p, &pl); };
    const hipError_t e = skinny_sampling(p) ? skinny_for_batch<true>(p.B, plan) : skinny_for_batch<false>(p.B, plan);
    return e == hipSuccess ? pl.grid : -1;
}

hipError_t launch_skinny(const SkinnyParams& p, hipStream_t s) {
    if (p.B < 1 || p.B > 16 || (p.K & 3)) return hipErrorInvalidValue;
    if (p.parts && p.X2) return hipErrorInvalidValue;   // half-staged: pair launches only
    if (p.ymode == YMODE_ARGMAX && (!p.am_mask || !p.am_val || !p.am_idx || p.am_ld < skinny_grid(p) || p.resid || p.act)) return hipErrorInvalidValue;
    if (p.am_lp && (p.ymode != YMODE_ARGMAX || (p.am_lp != 1 && p.am_lp != 2) || !p.am_lse || !p.am_side || p.am_eos < 0 || p.am_eos >= p.N ||
                    (p.am_lp == 2 && (p.am_ns < 0 || p.am_ns >= p.N))))
        return hipErrorInvalidValue;
    if (skinny_sampling(p)) return skinny_for_batch<true>(p.B, [&](auto sh) { return skinny_single<decltype(sh), true>(p, s); });
    return skinny_for_batch<false>(p.B, [&](auto sh) { return skinny_single<decltype(sh), false>(p, s); });
}

hipError_t launch_skinny_pair(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s) {
    if (a.B != b.B || a.B < 1 || a.B > 16) return hipErrorInvalidValue;
    return skinny_for_batch<false>(a.B, [&](auto sh) { return skinny_pair_cfg<decltype(sh)>(a, b, s); });
}

hipError_t launch_skinny_qkv_hoist(const SkinnyParams& a, const SkinnyParams& b, hipStream_t s) {
    if (a.B != b.B || a.B < 1 || a.B > 16 || (a.K & 3) || (b.K & 3)) return hipErrorInvalidValue;
    if (a.ymode != YMODE_QKV_APPEND || a.xmode != XMODE_LAYERNORM || a.parts || a.X2 || a.x_direct) return hipErrorInvalidValue;
    // the passenger: a plain GEMV over whole LDS-staged rows
    if (b.ymode != YMODE_PLAIN || b.xmode != XMODE_PLAIN || b.parts || b.X2 || b.x_direct || b.K > 1024 || !b.X || !b.W || !b.Y) return hipErrorInvalidValue;
    if (a.w_half != b.w_half || (a.w_nt != 0) != (b.w_nt != 0)) return hipErrorInvalidValue;
    return skinny_for_batch<false>(a.B, [&](auto sh) { return skinny_hoist_cfg<decltype(sh)>(a, b, s); });
}

// ------------------------------------------------------------------------------------------------ decode attention
// One query row per (utterance, head); keys/values [S][64] streamed once.  Grid (n_split, H, B).  A key is read by a group of LPK
// lanes with one 16-byte load each: fp32 caches 16 lanes x 4 dims (a block's 4 waves form 16 independent online-softmax streams),
// fp16 caches (fp16 decoder engines) 8 lanes x 8 dims (32 streams) -- either way one wave instruction reads 1 KiB of consecutive
// keys.  Streams take interleaved keys; their states are merged through LDS into one partial (o[64] unnormalised, m, l) per split.
// With n_split > 1 the splits of a (utterance, head) are merged by whichever block arrives last (arrival ticket; partials stored
// write-through and re-read with sc1 loads, cdna guide §6 G16 R1); the merge walks the partials in split order, so the result is
// bitwise reproducible whatever the arrival order.  Scores, softmax and accumulators are fp32 in both forms (the reference forces
// fp32 scores in fp16 builds too, model.py:292-295).  Output: normalised context rows out[b][h*64 .. +63].
__device__ __forceinline__ float row8_allreduce_sum(float v) {   // sum over each aligned group of 8 lanes, total in every lane
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x141, 0xf, 0xf, false));  // row_half_mirror: i <-> 7-i
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    return v;
}
// PIPE: the U keys a stream takes per iteration are handled as two half-tiles with their own registers; the loads of one half are in
// flight while the other is consumed (the same number of loads in flight as the plain form, but the exp / FMA work of a half-tile --
// a fifth of an iteration with fp16 caches, a tenth with fp32 -- no longer sits between one tile's arrival and the next request).
// NTHR = 512: eight waves per block = twice the streams, half the dependent load -> consume round trips per stream and twice the bytes
// in flight per CU (the kernel is bound by round trips x bytes in flight, not by the HBM rate: it takes 17.1 us with a layer's K/V
// resident in the Infinity Cache and 17.8 from HBM).
// SLOT (continuous mode, cross attention): slot b's keys / values live in cache row slot_row[b] of a pool, not in row b.
// ANC (beam search, self attention): key s of row b lives in cache row anc[b][s] -- after a beam step row b continues the history of
// another row, and instead of regathering the caches (L x 2 x rows x H x t x 64 elements read and written per step) only the row part
// of every key address comes from the ancestry table (one 4-byte load per key, shared by the lanes of that key); the 16-byte key
// loads, the streams and their order are those of the plain kernel, so the result is bitwise that of a regathered cache.
// G > 1 (beam search, cross attention, grouped form): the G beams of an utterance share its K/V, so ONE block streams cache row
// blockIdx.z and carries the G query rows blockIdx.z * G + g against every key tile -- the keys are in registers already; it is G dot
// products and online-softmax states per key instead of one, and the K/V stream is paid once per utterance instead of once per beam.
// QCAP (token-level timestamps, cross attention): the block of split 0 of a selected head stores its finished query into the history
// buffer p.qh at row st->step -- one stream's lanes, plain 16-byte vector stores -- before a finished row would leave; a compile-time form,
// the other instantiations are untouched.
template <int U, bool NT, bool KVH, bool PIPE = false, bool ALIVE = false, int NTHR = 256, bool SLOT = false, bool ANC = false, int G = 1,
          bool QCAP = false>
__global__ __launch_bounds__(NTHR) void dec_attn_kernel(const DecAttnParams p) {
    constexpr int LPK = KVH ? 8 : 16;          // lanes per key
    constexpr int DPL = HEAD_DIM / LPK;        // head dims per lane: 8 or 4 (16 bytes of K or V either way)
    constexpr int NSTR = NTHR / LPK;           // online-softmax streams per block
    constexpr int KSZ = KVH ? 2 : 4;
    static_assert(G == 1 || (!ALIVE && !SLOT && !ANC), "the grouped form is its own addressing");
    __shared__ float sm_o[G][NSTR][HEAD_DIM];
    __shared__ float sm_m[G][NSTR], sm_l[G][NSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & (LPK - 1), sid = tid / LPK;
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z * G;   // (G > 1: the first of the block's query rows)
    const int len = p.fixed_len > 0 ? p.fixed_len : p.st->self_len[b] + 1;
    const int chunk = (len + p.n_split - 1) / p.n_split;
    const int s_begin = split * chunk, s_end = min(len, s_begin + chunk);
    const int d = p.H * HEAD_DIM;
    // streams in use: all of them, except that an eight-wave block over a short key range (self-attention early in a transcript) works
    // as a four-wave one -- waves 4-7 leave at once (a finished wave does not hold a barrier), and the merge below walks half as many
    // partials: at 32 keys the full eight-wave form measured 3.8 us against 3.3
    static_assert(NTHR == 256 || NTHR == 512, "four- or eight-wave blocks");
    const int nkeys = s_end - s_begin;
    const int nstr = (NTHR == 256 || nkeys >= 128) ? NSTR : NSTR / 2;
    if (NTHR != 256 && sid >= nstr) return;   // wave-uniform (LPK divides 64)

    const int crow = G > 1 ? (int)blockIdx.z : SLOT ? max(p.slot_row[b], 0) : b;   // (an idle slot reads row 0: finite values nobody uses)
    const char* kb = reinterpret_cast<const char*>(p.kcache) + (((size_t)crow * p.H + h) * p.s_cap * HEAD_DIM + DPL * c) * KSZ;
    const char* vb = reinterpret_cast<const char*>(p.vcache) + (((size_t)crow * p.H + h) * p.s_cap * HEAD_DIM + DPL * c) * KSZ;
    typedef float f4v __attribute__((ext_vector_type(4)));   // 16 raw bytes
    const int* anc_row = nullptr;
    if constexpr (ANC) anc_row = p.anc + ((size_t)(p.st ? (p.st->step & 1) : 0) * MAX_ROWS + b) * p.anc_ld;
    const size_t row_bytes = (size_t)p.H * p.s_cap * HEAD_DIM * KSZ;
    // byte offset of key ks from kb / vb (ANC: kb / vb are row b's, the table gives the row that really holds the key)
    auto key_off = [&](const int ks) -> long long {
        long long off = (long long)ks * (HEAD_DIM * KSZ);
        if constexpr (ANC) off += ((long long)anc_row[ks] - crow) * (long long)row_bytes;
        return off;
    };
    auto load_tile = [&](f4v (&kk)[U], f4v (&vv)[U], const int s0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long key = key_off(min(s0 + nstr * u, s_end - 1));
            if (NT) {  // K/V are read exactly once per step: non-temporal loads keep them from displacing weights in L2
                kk[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(kb + key));
                vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(vb + key));
            } else {
                kk[u] = *reinterpret_cast<const f4v*>(kb + key);
                vv[u] = *reinterpret_cast<const f4v*>(vb + key);
            }
        }
    };
    auto widen = [&](const f4v raw, float (&x)[DPL]) {
        if constexpr (KVH) {
            typedef _Float16 h2v __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float f = raw[i];   // (a copy first: __builtin_bit_cast of the element expression itself reads element 0)
                const h2v t = __builtin_bit_cast(h2v, f);
                x[2 * i] = (float)t[0];
                x[2 * i + 1] = (float)t[1];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = raw[i];
        }
    };
    // the first K/V tile is requested before the query prologue, whose loads and reductions then hide under its latency
    const int s_first = s_begin + sid;
    f4v kk[U], vv[U];
    constexpr int UH = PIPE ? U / 2 : U;       // keys per stream and half-tile
    auto load_half = [&](const int h, const int s0) {   // half-tile h = registers [h * UH, (h + 1) * UH); unconditional clamped loads
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            const long long key = key_off(min(s0 + nstr * u, s_end - 1));
            if (NT) {
                kk[h * UH + u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(kb + key));
                vv[h * UH + u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(vb + key));
            } else {
                kk[h * UH + u] = *reinterpret_cast<const f4v*>(kb + key);
                vv[h * UH + u] = *reinterpret_cast<const f4v*>(vb + key);
            }
        }
    };
    if constexpr (PIPE) {
        if (s_begin < s_end) {   // block-uniform; clamping keeps every address inside this block's keys
            load_half(0, s_first);
            load_half(1, s_first + nstr * UH);
        }
    } else {
        if (s_first < s_end) load_tile(kk, vv, s_first);
    }

    float q[G][DPL];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < DPL; i += 4) {
        const float4 t = *reinterpret_cast<const float4*>(p.q + (size_t)(b + g) * d + h * HEAD_DIM + DPL * c + i);
        q[g][i] = t.x; q[g][i + 1] = t.y; q[g][i + 2] = t.z; q[g][i + 3] = t.w;
    }
    }
    if (p.ln_h) {
        // folded query: finish the LayerNorm of the residual row here (every wave for itself: d <= 1024 floats, no barrier),
        // two-pass statistics like the LayerNorm kernels: q = (u - mean . r) * rstd + t
        float r[DPL], t[DPL];
#pragma unroll
        for (int i = 0; i < DPL; i += 4) {
            const float4 r4 = *reinterpret_cast<const float4*>(p.ln_r + h * HEAD_DIM + DPL * c + i);
            const float4 t4 = *reinterpret_cast<const float4*>(p.ln_t + h * HEAD_DIM + DPL * c + i);
            r[i] = r4.x; r[i + 1] = r4.y; r[i + 2] = r4.z; r[i + 3] = r4.w;
            t[i] = t4.x; t[i + 1] = t4.y; t[i + 2] = t4.z; t[i + 3] = t4.w;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
        const float* hr = p.ln_h + (size_t)(b + g) * d;
        float4 hv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v)  // unconditional loads from clamped addresses, all four in flight before the first use
            hv[v] = *reinterpret_cast<const float4*>(hr + min(4 * lane + 256 * v, d - 4));
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise serialises them: load, wait, select, next load)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (4 * lane + 256 * v >= d) hv[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        float sum = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) sum += (hv[v].x + hv[v].y) + (hv[v].z + hv[v].w);
        const float mean = wave_allreduce_sum_d(sum) / d;
        float sq = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if ((4 * lane + 256 * v) < d) {
                const float a0 = hv[v].x - mean, a1 = hv[v].y - mean, a2 = hv[v].z - mean, a3 = hv[v].w - mean;
                sq += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        const float rstd = rsqrtf(wave_allreduce_sum_d(sq) / d + 1e-5f);
#pragma unroll
        for (int i = 0; i < DPL; ++i) q[g][i] = (q[g][i] - mean * r[i]) * rstd + t[i];
        }
    }
    if constexpr (QCAP) {
        static_assert(G == 1, "the query capture is a form of the plain cross attention");
        if (split == 0 && sid == 0) {
            const int sel = p.qh_sel[h], step = p.st->step;
            if (sel >= 0 && !p.st->done && step < p.qh_steps) {   // (steps enqueued past the stop test must not write)
                float* dst = p.qh + (((size_t)sel * p.qh_rows + b) * p.qh_steps + step) * HEAD_DIM + DPL * c;
#pragma unroll
                for (int i = 0; i < DPL; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(q[0][i], q[0][i + 1], q[0][i + 2], q[0][i + 3]);
            }
        }
    }
    // A finished row pads whatever it computes (run.py:219-226 stops a batch-1 decode at its own EOS): in the step graph that
    // wt_decoder_run switches to once a row has finished, such a row leaves here and streams no K/V.  (The test costs the dominant
    // kernel 0.3-1.8 % when it sits in the all-rows-alive graph -- measured -- which is why that graph is built without it.)
    if constexpr (ALIVE) {   // a compile-time form: the all-rows-alive graph runs the kernel exactly as it was
        if (p.alive[b] == 0) return;   // block-uniform
    }
    float m[G], l[G];
    float acc[G][DPL];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) acc[g][i] = 0.f;
    }
    auto consume = [&](const int h, const int s0) {   // online-softmax update with the UH keys of half-tile h (first key s0 < s_end)
        float sc[G][UH];
        float mx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) mx[g] = m[g];
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            float kf[DPL];
            widen(kk[h * UH + u], kf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float dot = q[g][DPL - 1] * kf[DPL - 1];
#pragma unroll
                for (int i = DPL - 2; i >= 0; --i) dot = fmaf(q[g][i], kf[i], dot);
                sc[g][u] = KVH ? row8_allreduce_sum(dot) : row16_allreduce_sum(dot);
                if (s0 + nstr * u >= s_end) sc[g][u] = -INFINITY;
                mx[g] = fmaxf(mx[g], sc[g][u]);
            }
        }
        // plain form: s0 < s_end, so u = 0 is a real key and mx is finite.  PIPE consumes branch-free (a skipped consumer would make
        // the waitcnt pass merge "loads pending" with "loads waited for" and drain vmcnt(0) in front of every request): a stream
        // past its last key has every score at -inf, keeps m, and rescales by exp(0) -- or by 0 while it has seen no key at all.
        float mxs[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            mxs[g] = PIPE && mx[g] == -INFINITY ? 0.f : mx[g];
            const float alpha = __expf(m[g] - mxs[g]);
            l[g] *= alpha;
#pragma unroll
            for (int i = 0; i < DPL; ++i) acc[g][i] *= alpha;
        }
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            float vf[DPL];
            widen(vv[h * UH + u], vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float pr = __expf(sc[g][u] - mxs[g]);
                l[g] += pr;
#pragma unroll
                for (int i = 0; i < DPL; ++i) acc[g][i] = fmaf(pr, vf[i], acc[g][i]);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) m[g] = mx[g];
    };
    if constexpr (PIPE) {
        const int stride = nstr * U;
        const int n_it = (s_end - s_begin + stride - 1) / stride;   // block-uniform; a stream's own keys end up to one iteration earlier
        int sA = s_first, sB = s_first + nstr * UH;
        // every load of the prologue (query, LayerNorm operands) has landed before the loop: the waitcnt pass merges the loop-entry
        // state into every iteration, so a register still pending at entry costs a near-full drain per iteration (seen in the ISA
        // as vmcnt(1) / vmcnt(0) in front of the first FMA that reads q).  vmcnt(0), lgkmcnt / expcnt untouched:
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (int it = 0; it < n_it; ++it) {
            // (scheduling fences: without them the consumer of half B is hoisted above the requests of half A.  No branch in the loop
            //  body: requests are unconditional and clamped -- the last iteration re-reads this block's last key -- so that the
            //  waits stay counted, vmcnt(2 * UH), instead of vmcnt(0))
            consume(0, sA);
            sA += stride;
            __builtin_amdgcn_sched_barrier(0);
            load_half(0, sA);
            __builtin_amdgcn_sched_barrier(0);
            consume(1, sB);
            sB += stride;
            __builtin_amdgcn_sched_barrier(0);
            load_half(1, sB);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int s0 = s_first; s0 < s_end; s0 += nstr * U) {  // (a register double buffer of WHOLE tiles measured 0.5-1 us SLOWER per launch)
            if (s0 != s_first) load_tile(kk, vv, s0);
            consume(0, s0);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int i = 0; i < DPL; i += 4)
            *reinterpret_cast<float4*>(&sm_o[g][sid][DPL * c + i]) = make_float4(acc[g][i], acc[g][i + 1], acc[g][i + 2], acc[g][i + 3]);
        if (c == 0) {
            sm_m[g][sid] = m[g];
            sm_l[g][sid] = l[g];
        }
    }
    __syncthreads();
    if (wave != 0) return;  // wave-uniform: only wave 0 publishes / merges
    // one query row at a time (G > 1: the block's rows b .. b + G - 1)
    auto finish_row = [&](const int g) {
    const int bg = b + g;
    // merge of the streams' partials by wave 0, with a COMPILE-TIME trip count in either case (a run-time bound keeps hipcc from issuing
    // the LDS reads of all partials ahead of the first exp: the loop then pays one LDS round trip per stream)
    float M, o = 0.f, L = 0.f;
    auto merge = [&](auto COUNT) {
        constexpr int n = decltype(COUNT)::value;
        M = sm_m[g][0];
#pragma unroll
        for (int i = 1; i < n; ++i) M = fmaxf(M, sm_m[g][i]);
        if (M > -INFINITY) {
#pragma unroll
            for (int i = 0; i < n; ++i) {
                const float w = __expf(sm_m[g][i] - M);  // streams with no key have m = -inf -> weight 0
                o = fmaf(w, sm_o[g][i][lane], o);
                L = fmaf(w, sm_l[g][i], L);
            }
        }
    };
    if (NTHR == 256 || nstr == NSTR) merge(std::integral_constant<int, NSTR>{});
    else merge(std::integral_constant<int, NSTR / 2>{});
    float* outp = p.out + (size_t)bg * d + h * HEAD_DIM;
    if (p.n_split == 1) {
        outp[lane] = o / L;
        return;
    }
    float* pbase = p.part + ((size_t)bg * p.H + h) * p.n_split * PART_STRIDE;
    float* pp = pbase + split * PART_STRIDE;
    if (p.defer_merge) {  // the consumer GEMV merges the splits while it stages its activations (kernel boundary = visibility)
        pp[lane] = o;
        if (lane == 0) {
            pp[64] = M;
            pp[65] = L;
        }
        return;
    }
    // publish (cdna guide §6 G16, write-through form): every payload word is stored sc1 by THIS wave, the wave
    // drains its stores, then one lane takes an arrival ticket; the last arriver reads every word with sc1 loads.
    __hip_atomic_store(pp + lane, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
        __hip_atomic_store(pp + 64, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 65, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int last = 0;
    if (lane == 0) {
        const int ticket = __hip_atomic_fetch_add(p.cnt + bg * p.H + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = ticket == p.n_split - 1;
    }
    last = __shfl(last, 0);
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler-only: keep the loads below the ticket
    // merge in split order; EVERY load of a published word is an agent-scope relaxed load (sc1, vector path, L1 bypass)
    float Mg = -INFINITY;
    for (int s = 0; s < p.n_split; ++s)
        Mg = fmaxf(Mg, __hip_atomic_load(pbase + s * PART_STRIDE + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    float og = 0.f, Lg = 0.f;
    for (int s = 0; s < p.n_split; ++s) {
        const float ms = __hip_atomic_load(pbase + s * PART_STRIDE + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float ls = __hip_atomic_load(pbase + s * PART_STRIDE + 65, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float os = __hip_atomic_load(pbase + s * PART_STRIDE + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float w = __expf(ms - Mg);  // a split with no keys has m = -inf, l = 0, o = 0 -> weight 0
        og = fmaf(w, os, og);
        Lg = fmaf(w, ls, Lg);
    }
    outp[lane] = og / Lg;
    if (lane == 0) p.cnt[bg * p.H + h] = 0;  // re-arm the ticket for the next launch (kernel boundary orders it)
    };
#pragma unroll
    for (int g = 0; g < G; ++g) finish_row(g);
}
// The instantiation a launch runs.  dec_attn_form chooses it -- the only place that does -- and launch_dec_attn maps it to the kernel.
struct DecAttnForm {
    bool nt, kv_half, pipe, alive, slot, anc, qcap;
    int threads, group;
};
// The two block-shape choices, as functions of the load policy and the cache precision (constexpr: the dispatch instantiates the chosen
// forms only, so an A/B of either is a one-line change here).
// Half-tile software pipeline (PIPE): measured per cross-attention launch, fp16 caches: batch 16 19.04 -> 18.69 us, batch 8
// 13.35 -> 12.84 (two splits) / 15.28 -> 13.49 (one); fp32 caches 19.87 vs 19.98 (no gain: a tenth of an iteration is arithmetic
// there, a fifth with fp16 caches) -- so fp16 caches only, and only the non-temporal forms have it.
constexpr bool dec_attn_pipe(const bool nt, const bool kv_half) { return kv_half && nt; }
// fp32 caches: eight-wave blocks (measured per launch, 256 -> 512 threads: cross-attention, two splits 19.5 -> 18.8 us, one split
// (batch 16) 23.9 -> 19.9; self-attention at 224 / 447 keys 6.6 -> 5.7 / 9.4 -> 8.3; below 128 keys the block works as four waves).
// (sixteen-wave blocks measured SLOWER than eight: cross-attention 19.2 -> 20.6 us, self-attention at 224 keys 5.9 -> 6.4)
// (and four keys per stream and iteration stay best in the eight-wave form: U = 2 / 4 / 8 -> 19.9 / 19.8 / 20.1 us cross-attention,
//  6.3 / 5.8 / 6.0 us self-attention at 224 keys)
// fp16 caches stay on four-wave blocks -- they already are 32 streams, 8 lanes per key: eight waves = 64 streams measured 18.65 vs 18.6 us
// at batch 16 and 13.1 vs 13.1 at batch 8 with two splits.
constexpr int dec_attn_threads(const bool kv_half) { return kv_half ? 256 : 512; }

// variant: WT_ATTN_VARIANT (0 forces default-policy loads, 1 forces non-temporal loads, 2: as the engine asks)
static hipError_t dec_attn_form(const DecAttnParams& p, const int variant, DecAttnForm* f) {
    if (p.qh) {   // token-level timestamps: the cross-attention launches of the step graph
        if (p.group > 1 || p.anc || p.slot_row || p.alive || !p.qh_sel || !p.st || !p.ln_h || p.fixed_len <= 0) return hipErrorInvalidValue;
    } else if (p.group > 1) {   // beam search, cross attention, grouped form: grid z = utterances, `group` query rows per block
        if (p.anc || p.alive || p.slot_row || p.B % p.group != 0 || (p.group != 2 && p.group != 4)) return hipErrorInvalidValue;
    } else if (p.anc) {   // beam search: the self-attention launches of the step graph
        if (p.n_split != 1 || p.slot_row || p.alive || p.anc_ld < p.s_cap) return hipErrorInvalidValue;
    }
    // non-temporal K/V loads: 18.6 vs 20.4 us per medium.en cross-attention launch; default policy only when a whole decode
    // step fits the Infinity Cache (engine.hip: wt_decoder_begin)
    f->nt = variant == 2 ? p.nt != 0 : variant != 0;
    f->kv_half = p.kv_half != 0;
    f->pipe = dec_attn_pipe(f->nt, f->kv_half);
    f->threads = dec_attn_threads(f->kv_half);
    // the skip-finished-rows step graph: non-temporal streaming forms only, others run the plain kernels (the forms above reject it)
    f->alive = p.alive && f->nt;
    f->slot = p.slot_row != nullptr;   // continuous mode: the cross-attention launches of the step graph (the engine's own plans only)
    f->anc = p.anc != nullptr;
    f->qcap = p.qh != nullptr;
    f->group = p.group > 1 ? p.group : 1;
    return hipSuccess;
}

// The forms of one addressing mode (SLOT, ANC, G, QCAP).  Only what dec_attn_form can choose is compiled: the block shape it gives a
// (load policy, cache precision), and ALIVE where the mode has it; any other record is an error, not another kernel.
template <bool SLOT, bool ANC, int G, bool QCAP>
static hipError_t dec_attn_launch(const DecAttnForm& f, const DecAttnParams& p, hipStream_t s) {
    return with_flags([&](auto NT, auto KVH, auto PIPE, auto ALIVE, auto WAVES8) {
        constexpr int NTHR = WAVES8 ? 512 : 256;
        constexpr bool chosen = PIPE == dec_attn_pipe(NT, KVH) && NTHR == dec_attn_threads(KVH);
        constexpr bool exists = !ALIVE || (NT && !ANC && G == 1 && !QCAP);
        if constexpr (!chosen || !exists) return hipErrorInvalidValue;
        else {
            hipLaunchKernelGGL((dec_attn_kernel<4, NT, KVH, PIPE, ALIVE, NTHR, SLOT, ANC, G, QCAP>), dim3(p.n_split, p.H, p.B / G), dim3(NTHR), 0, s, p);
            return hipGetLastError();
        }
    }, f.nt, f.kv_half, f.pipe, f.alive, f.threads == 512);
}

hipError_t launch_dec_attn(const DecAttnParams& p, hipStream_t s) {
    // A/B override, see dec_attn_form.  A function-local static with an initialiser: latched once, thread-safe (handles of different
    // host threads launch concurrently).
    static const int variant = [] {
        const char* e = tuning_env("WT_ATTN_VARIANT");
        return e ? atoi(e) : 2;
    }();
    DecAttnForm f;
    const hipError_t e = dec_attn_form(p, variant, &f);
    if (e != hipSuccess) return e;
    if (f.qcap) return dec_attn_launch<false, false, 1, true>(f, p, s);
    if (f.group == 4) return dec_attn_launch<false, false, 4, false>(f, p, s);
    if (f.group == 2) return dec_attn_launch<false, false, 2, false>(f, p, s);
    if (f.anc) return dec_attn_launch<false, true, 1, false>(f, p, s);
    if (f.slot) return dec_attn_launch<true, false, 1, false>(f, p, s);
    return dec_attn_launch<false, false, 1, false>(f, p, s);
}

// ------------------------------------------------------------------------------------------------ greedy select
// logits processors + argmax + pad/EOS bookkeeping + append, on device (run.py:199-226; HF utils.py:1502-1526;
// processors logits_process.py:1281-1328 in the order Suppress -> SuppressAtBegin -> Force).  Two launches:
//   greedy_select_kernel  grid (SELECT_CHUNKS, B): masked partial argmax of one vocabulary chunk (lowest index on ties);
//   greedy_finish_kernel  one block: final argmax per row, forced / pad / EOS rules, append, advance the step counters,
//                         stop test, and the NEXT step's input embedding (embed_tokens[tok] + embed_positions[pos]).
// LP (log-probability mode): the chunk's log-sum-exp pairs beside its candidate -- the same quantities as the LP epilogue of the
// vocabulary GEMV, so the fused and the non-fused step feed one finish kernel.
template <bool LP = false>
__global__ __launch_bounds__(256) void greedy_select_kernel(const SelectParams p) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ float4 s_lse[4];
    const DecState* st = p.st;
    if (st->done) return;  // steps enqueued past the stop test are no-ops
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, cur_len = st->cur_len[b], step = st->step;
    const bool at_begin = cur_len == p.begin_index;
    const float* lg = p.logits + (size_t)b * p.V;
    float* tr = p.trace ? p.trace + ((size_t)b * (p.max_length - 1) + step) * p.V : nullptr;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    float lm = -INFINITY, ls = 0.f, rm = -INFINITY, rs = 0.f;
    auto consider = [&](float x, uint8_t mk, int v) {
        if constexpr (LP) {
            if (p.lp_ns >= 0) {
                lse_add(rm, rs, x);
                if (v == p.lp_ns) p.lp_side[2 * b + 1] = x;
            }
        }
        if ((mk & 1) || ((mk & 2) && at_begin)) x = -INFINITY;
        if constexpr (LP) {
            lse_add(lm, ls, x);
            if (v == p.eos) p.lp_side[2 * b] = x;
        }
        if (argmax_better(x, v, best, bidx)) {
            best = x;
            bidx = v;
        }
    };
    if ((p.V & 3) == 0) {  // 16-byte path, several independent loads in flight per thread
        const int n4 = p.V >> 2, per = (n4 + SELECT_CHUNKS - 1) / SELECT_CHUNKS;
        const int i0 = chunk * per, i1 = min(n4, i0 + per);
        const float4* lg4 = reinterpret_cast<const float4*>(lg);
        const uchar4* mk4 = reinterpret_cast<const uchar4*>(p.mask);
        float4* tr4 = reinterpret_cast<float4*>(tr);
#pragma unroll 4
        for (int i = i0 + tid; i < i1; i += 256) {
            const float4 x = lg4[i];
            const uchar4 m = mk4[i];
            if (tr) tr4[i] = x;
            consider(x.x, m.x, 4 * i);
            consider(x.y, m.y, 4 * i + 1);
            consider(x.z, m.z, 4 * i + 2);
            consider(x.w, m.w, 4 * i + 3);
        }
    } else {
        const int per = (p.V + SELECT_CHUNKS - 1) / SELECT_CHUNKS;
        const int v0 = chunk * per, v1 = min(p.V, v0 + per);
        for (int v = v0 + tid; v < v1; v += 256) {
            const float x = lg[v];
            if (tr) tr[v] = x;
            consider(x, p.mask[v], v);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (argmax_better(ov, oi, best, bidx)) {
            best = ov;
            bidx = oi;
        }
        if constexpr (LP) {
            lse_merge(lm, ls, __shfl_xor(lm, o), __shfl_xor(ls, o));
            lse_merge(rm, rs, __shfl_xor(rm, o), __shfl_xor(rs, o));
        }
    }
    if ((tid & 63) == 0) {
        s_val[tid >> 6] = best;
        s_idx[tid >> 6] = bidx;
        if constexpr (LP) s_lse[tid >> 6] = make_float4(lm, ls, rm, rs);
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i)
            if (argmax_better(s_val[i], s_idx[i], best, bidx)) {
                best = s_val[i];
                bidx = s_idx[i];
            }
        p.part_val[b * SELECT_CHUNKS + chunk] = best;
        p.part_idx[b * SELECT_CHUNKS + chunk] = bidx;
        if constexpr (LP) {
            for (int i = 1; i < 4; ++i) {
                lse_merge(lm, ls, s_lse[i].x, s_lse[i].y);
                lse_merge(rm, rs, s_lse[i].z, s_lse[i].w);
            }
            p.lp_part[b * SELECT_CHUNKS + chunk] = make_float4(lm, ls, rm, rs);
        }
    }
}

// Temperature sampling without the fused epilogue (the WT_NO_FUSED_ARGMAX A/B path): the logits are in memory, and this kernel walks them
// in the PARTITION AND ORDER of the sampling GEMV's epilogue -- workgroup `block` of that GEMV's plan owns G row groups of rows_per_group
// rows, and within a group the rows of each parity are finished in ascending order by one output lane -- so every partial (best key, its
// id and score, the log-sum-exp pairs) is the float the fused epilogue would have written, and the finish kernel gives bitwise the same
// token and log-probability on either path.  Grid (GEMV workgroups, B), one thread per (group, row parity) slot.
__global__ __launch_bounds__(64) void sample_select_kernel(const SelectParams p, const int rows_per_group, const int G) {
    __shared__ float s_val[16], s_sc[16];
    __shared__ int s_idx[16];
    __shared__ float4 s_lse[16];
    const DecState* st = p.st;
    if (st->done) return;  // steps enqueued past the stop test are no-ops
    const int tid = threadIdx.x, block = blockIdx.x, b = blockIdx.y, cur_len = st->cur_len[b], step = st->step;
    const int samp_t = st->pos[b] + 1;   // the draws' position is the row's own (== cur_len unless the id rows are left-padded)
    const bool at_begin = cur_len == p.begin_index;
    const float* lg = p.logits + (size_t)b * p.V;
    float* tr = p.trace ? p.trace + ((size_t)b * (p.max_length - 1) + step) * p.V : nullptr;
    float best = -INFINITY, bsc = -INFINITY;
    int bidx = 0x7fffffff;
    float lm = -INFINITY, ls = 0.f, rm = -INFINITY, rs = 0.f;
    if (tid < 2 * G) {
        const unsigned long long seed = p.samp_seeds[b];
        const int row_begin = (int)min((long long)p.V, ((long long)block * G + (tid >> 1)) * rows_per_group);
        const int row_end = min(p.V, row_begin + rows_per_group);
        for (int n = row_begin + (tid & 1); n < row_end; n += 2) {
            float x = lg[n];
            if (tr) tr[n] = x;
            if (p.lp_ns >= 0) {
                lse_add(rm, rs, x);
                if (n == p.lp_ns) p.lp_side[2 * b + 1] = x;
            }
            const uint8_t mk = p.mask[n];
            if ((mk & 1) || ((mk & 2) && at_begin)) x = -INFINITY;
            lse_add(lm, ls, x);
            if (n == p.eos) p.lp_side[2 * b] = x;
            unsigned dr[4];
            sample_draws(seed, samp_t, n >> 2, dr);
            const int q = n & 3;
            const float key = sample_key(x, p.samp_temp, q == 0 ? dr[0] : q == 1 ? dr[1] : q == 2 ? dr[2] : dr[3]);
            if (argmax_better(key, n, best, bidx)) {
                best = key;
                bidx = n;
                bsc = x;
            }
        }
        s_val[tid] = best; s_idx[tid] = bidx; s_sc[tid] = bsc; s_lse[tid] = make_float4(lm, ls, rm, rs);
    }
    __syncthreads();
    if (tid == 0) {   // the slots in the order the epilogue's LDS stage scans them (its other slots are empty: exact no-ops)
        best = -INFINITY; bsc = -INFINITY; bidx = 0x7fffffff;
        lm = -INFINITY; ls = 0.f; rm = -INFINITY; rs = 0.f;
        for (int i = 0; i < 2 * G; ++i) {
            if (argmax_better(s_val[i], s_idx[i], best, bidx)) {
                best = s_val[i];
                bidx = s_idx[i];
                bsc = s_sc[i];
            }
            lse_merge(lm, ls, s_lse[i].x, s_lse[i].y);
            if (p.lp_ns >= 0) lse_merge(rm, rs, s_lse[i].z, s_lse[i].w);
        }
        const size_t at = (size_t)b * p.n_parts + block;
        p.part_val[at] = best;
        p.part_idx[at] = bidx;
        p.samp_sc[at] = bsc;
        p.lp_part[at] = make_float4(lm, ls, rm, rs);
    }
}

// ---- timestamp mode (WhisperTimeStampLogitsProcessor, logits_process.py:1331-1396, after Suppress -> SuppressAtBegin -> Force).
// ts_select_kernel, grid (SELECT_CHUNKS, B): the static masks, <|notimestamps|> and the per-row timestamp grammar (pairs; nothing but
// a timestamp or EOS.. after a lone timestamp; the max-initial-timestamp cap), then one TsPart per chunk.  The log-sum-exp of the
// timestamp scores against the text maximum (rule 5) and the forced <|0.00|> (rule 2) are decided by greedy_finish_kernel<true>.
// (sum, max) pairs: s * exp(m - nm) with the empty pair (0, -inf) contributing 0 and a NaN sum staying NaN.
__device__ __forceinline__ float ts_rescale(float s, float m, float nm) { return s == 0.f ? 0.f : s * expf(m - nm); }

// LP (log-probability mode): TsPart also carries the text-side pair (xmax, xsum), and lp_part the raw pair of the chunk (no_speech_prob).
// SAMP (temperature sampling, with LP): tmax / smax become the best Gumbel-max KEYS of the chunk's text / timestamp ids; their scores and
// the chunk's best unperturbed text score (rule 5's side; the timestamp pair (zmax, zsum) is of the scores as before) travel in samp_ts.
struct TsSamp {
    float tsc, ssc, rt;    // score of targ, score of sarg, best text score (NaN-aware, with its index for the order)
    int rti;
};
template <bool LP = false, bool SAMP = false>
__global__ __launch_bounds__(256) void ts_select_kernel(const SelectParams p) {
    static_assert(!SAMP || LP, "sampling runs with the log-sum-exp pairs on");
    __shared__ TsPart s_part[4];
    __shared__ float2 s_raw[4];
    __shared__ TsSamp s_samp[4];
    const DecState* st = p.st;
    if (st->done) return;  // steps enqueued past the stop test are no-ops
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, cur_len = st->cur_len[b], step = st->step;
    [[maybe_unused]] const int samp_t = st->pos[b] + 1;   // SAMP: the draws' position is the row's own (== cur_len unless the id rows are left-padded)
    const bool at_begin = cur_len == p.begin_index;
    const float* lg = p.logits + (size_t)b * p.V;
    float* tr = p.trace ? p.trace + ((size_t)b * (p.max_length - 1) + step) * p.V : nullptr;
    // the grammar of the row's timestamps so far (ids from ts_begin_index on) as two cut points: text ids below text_lo and
    // timestamps above ts_hi are masked
    const int* row = p.ids + (size_t)b * p.max_length;
    const int n = cur_len - p.ts_begin_index;
    const bool last = n >= 1 && row[cur_len - 1] >= p.tb;
    const bool penult = n < 2 || row[cur_len - 2] >= p.tb;
    int text_lo = 0, ts_hi = p.V - 1;
    if (last && penult) ts_hi = p.tb - 1;      // two timestamps in a row: text next
    if (last && !penult) text_lo = p.eos;      // a lone timestamp: its partner (or EOS and above) next
    if (cur_len == p.ts_begin_index && p.max_init >= 0) ts_hi = min(ts_hi, p.tb + p.max_init);
    TsPart r;
    r.tmax = r.smax = r.zmax = -INFINITY;
    r.targ = r.sarg = 0x7fffffff;
    r.zsum = 0.f;
    r.xmax = -INFINITY;
    r.xsum = 0.f;
    float rm = -INFINITY, rs = 0.f;
    TsSamp q;
    q.tsc = q.ssc = q.rt = -INFINITY;
    q.rti = 0x7fffffff;
    unsigned long long seed = 0;
    if constexpr (SAMP) seed = p.samp_seeds[b];
    auto consider = [&](float x, uint8_t mk, int v, unsigned draw) {
        if constexpr (LP) {
            if (p.lp_ns >= 0) {
                lse_add(rm, rs, x);
                if (v == p.lp_ns) p.lp_side[2 * b + 1] = x;
            }
        }
        if ((mk & 1) || ((mk & 2) && at_begin) || v == p.no_ts || v < text_lo || v > ts_hi) x = -INFINITY;
        if constexpr (LP) {
            if (v == p.eos) p.lp_side[2 * b] = x;
        }
        float key = x;
        if constexpr (SAMP) key = sample_key(x, p.samp_temp, draw);
        if (v < p.tb) {
            if (argmax_better(key, v, r.tmax, r.targ)) {
                r.tmax = key;
                r.targ = v;
                if constexpr (SAMP) q.tsc = x;
            }
            if constexpr (SAMP) {
                if (argmax_better(x, v, q.rt, q.rti)) {
                    q.rt = x;
                    q.rti = v;
                }
            }
            if constexpr (LP) lse_add(r.xmax, r.xsum, x);
        } else {
            if (argmax_better(key, v, r.smax, r.sarg)) {
                r.smax = key;
                r.sarg = v;
                if constexpr (SAMP) q.ssc = x;
            }
            if (x > r.zmax) {
                r.zsum = ts_rescale(r.zsum, r.zmax, x) + 1.f;
                r.zmax = x;
            } else if (x != -INFINITY) {
                r.zsum += expf(x - r.zmax);   // (NaN x: the sum becomes NaN)
            }
        }
    };
    if ((p.V & 3) == 0) {  // 16-byte path, as greedy_select_kernel
        const int n4 = p.V >> 2, per = (n4 + SELECT_CHUNKS - 1) / SELECT_CHUNKS;
        const int i0 = chunk * per, i1 = min(n4, i0 + per);
        const float4* lg4 = reinterpret_cast<const float4*>(lg);
        const uchar4* mk4 = reinterpret_cast<const uchar4*>(p.mask);
        float4* tr4 = reinterpret_cast<float4*>(tr);
#pragma unroll 4
        for (int i = i0 + tid; i < i1; i += 256) {
            const float4 x = lg4[i];
            const uchar4 m = mk4[i];
            if (tr) tr4[i] = x;
            unsigned dr[4] = {0u, 0u, 0u, 0u};
            if constexpr (SAMP) sample_draws(seed, samp_t, i, dr);
            consider(x.x, m.x, 4 * i, dr[0]);
            consider(x.y, m.y, 4 * i + 1, dr[1]);
            consider(x.z, m.z, 4 * i + 2, dr[2]);
            consider(x.w, m.w, 4 * i + 3, dr[3]);
        }
    } else {
        const int per = (p.V + SELECT_CHUNKS - 1) / SELECT_CHUNKS;
        const int v0 = chunk * per, v1 = min(p.V, v0 + per);
        for (int v = v0 + tid; v < v1; v += 256) {
            const float x = lg[v];
            if (tr) tr[v] = x;
            unsigned dr[4] = {0u, 0u, 0u, 0u};
            if constexpr (SAMP) sample_draws(seed, samp_t, v >> 2, dr);
            const int k = v & 3;
            consider(x, p.mask[v], v, k == 0 ? dr[0] : k == 1 ? dr[1] : k == 2 ? dr[2] : dr[3]);
        }
    }
    auto merge = [](TsPart& a, const TsPart& o, TsSamp& qa, const TsSamp& qo) {
        if (argmax_better(o.tmax, o.targ, a.tmax, a.targ)) {
            a.tmax = o.tmax;
            a.targ = o.targ;
            if constexpr (SAMP) qa.tsc = qo.tsc;
        }
        if (argmax_better(o.smax, o.sarg, a.smax, a.sarg)) {
            a.smax = o.smax;
            a.sarg = o.sarg;
            if constexpr (SAMP) qa.ssc = qo.ssc;
        }
        if constexpr (SAMP) {
            if (argmax_better(qo.rt, qo.rti, qa.rt, qa.rti)) {
                qa.rt = qo.rt;
                qa.rti = qo.rti;
            }
        }
        const float nm = fmaxf(a.zmax, o.zmax);   // (never NaN: zmax only takes finite or infinite scores)
        a.zsum = ts_rescale(a.zsum, a.zmax, nm) + ts_rescale(o.zsum, o.zmax, nm);
        a.zmax = nm;
        if constexpr (LP) lse_merge(a.xmax, a.xsum, o.xmax, o.xsum);
    };
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        TsPart x;
        x.tmax = __shfl_xor(r.tmax, o);
        x.targ = __shfl_xor(r.targ, o);
        x.smax = __shfl_xor(r.smax, o);
        x.sarg = __shfl_xor(r.sarg, o);
        x.zmax = __shfl_xor(r.zmax, o);
        x.zsum = __shfl_xor(r.zsum, o);
        if constexpr (LP) {
            x.xmax = __shfl_xor(r.xmax, o);
            x.xsum = __shfl_xor(r.xsum, o);
            lse_merge(rm, rs, __shfl_xor(rm, o), __shfl_xor(rs, o));
        }
        TsSamp y = q;
        if constexpr (SAMP) {
            y.tsc = __shfl_xor(q.tsc, o);
            y.ssc = __shfl_xor(q.ssc, o);
            y.rt = __shfl_xor(q.rt, o);
            y.rti = __shfl_xor(q.rti, o);
        }
        merge(r, x, q, y);
    }
    if ((tid & 63) == 0) {
        s_part[tid >> 6] = r;
        if constexpr (LP) s_raw[tid >> 6] = make_float2(rm, rs);
        if constexpr (SAMP) s_samp[tid >> 6] = q;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i) merge(r, s_part[i], q, s_samp[i]);
        p.ts_part[b * SELECT_CHUNKS + chunk] = r;
        if constexpr (SAMP) p.samp_ts[b * SELECT_CHUNKS + chunk] = make_float4(q.tsc, q.ssc, q.rt, 0.f);
        if constexpr (LP) {
            for (int i = 1; i < 4; ++i) lse_merge(rm, rs, s_raw[i].x, s_raw[i].y);
            p.lp_part[b * SELECT_CHUNKS + chunk] = make_float4(-INFINITY, 0.f, rm, rs);
        }
    }
}

// greedy_finish_kernel<true>: the SELECT_CHUNKS partials of a row sit in the first lanes of its lane group (requested before the
// DecState is read, like finish_request)
__device__ __forceinline__ void ts_request(const SelectParams& p, const int b, const int l, TsPart& c) {
    c = p.ts_part[(size_t)min(b, p.B - 1) * SELECT_CHUNKS + min(l, SELECT_CHUNKS - 1)];
}
// log-probability mode: what the finish kernel needs of a row's pick -- the score of the chosen token, the log-sum-exp pair (m, s) of the
// scores it competed with, whether its step is a forced one (one survivor: log-probability 0) and whether rule 5 masked the text ids
struct LpPick {
    float num, m, s;
    bool forced, text_masked;
    float key;             // sampling: the key the token won with
};
// rules 2 and 5 and the argmax of one row; every lane of the group returns the same token
// SAMP: tm / sm are keys; rule 5 compares the timestamps' log-sum-exp with the best unperturbed text score, then the better KEY among the
// surviving region(s) is the token and its carried score the numerator
template <bool LP = false, bool SAMP = false>
__device__ __forceinline__ int ts_pick(const SelectParams& p, const int b, const int l, const int lpb, const TsPart& c, const int cur_len,
                                       LpPick* lp = nullptr, const float4 sc = float4{0.f, 0.f, 0.f, 0.f}) {
    float tm = -INFINITY, sm = -INFINITY, zm = -INFINITY, zs = 0.f;
    int ti = 0x7fffffff, si = 0x7fffffff;
    float xm = -INFINITY, xs = 0.f;
    float tsc = -INFINITY, ssc = -INFINITY, rt = -INFINITY;
    if (b < p.B && l < SELECT_CHUNKS) {
        tm = c.tmax; ti = c.targ; sm = c.smax; si = c.sarg; zm = c.zmax; zs = c.zsum;
        if constexpr (LP) {
            xm = c.xmax; xs = c.xsum;
        }
        if constexpr (SAMP) {
            tsc = sc.x; ssc = sc.y; rt = sc.z;
        }
    }
    float M = zm;
    for (int o = lpb >> 1; o >= 1; o >>= 1) {   // lpb <= 64 and a power of two: a group never straddles a wave
        const float otm = __shfl_xor(tm, o), osm = __shfl_xor(sm, o);
        const int oti = __shfl_xor(ti, o), osi = __shfl_xor(si, o);
        const float otsc = SAMP ? __shfl_xor(tsc, o) : 0.f, ossc = SAMP ? __shfl_xor(ssc, o) : 0.f, ort = SAMP ? __shfl_xor(rt, o) : 0.f;
        if (argmax_better(otm, oti, tm, ti)) {
            tm = otm;
            ti = oti;
            if constexpr (SAMP) tsc = otsc;
        }
        if (argmax_better(osm, osi, sm, si)) {
            sm = osm;
            si = osi;
            if constexpr (SAMP) ssc = ossc;
        }
        if constexpr (SAMP) {
            if (argmax_better(ort, 0, rt, 0)) rt = ort;   // a NaN-aware maximum
        }
        M = fmaxf(M, __shfl_xor(M, o));
    }
    const float text_best = SAMP ? rt : tm;   // rule 5's text side: the best unperturbed text score
    float Z = ts_rescale(zs, zm, M);
    for (int o = lpb >> 1; o >= 1; o >>= 1) Z += __shfl_xor(Z, o);
    const float lse = M + logf(Z);   // -inf when every timestamp is masked (M = -inf, Z = 0); NaN with a NaN timestamp score
    int tok;
    if (cur_len == p.ts_begin_index - 1) tok = p.tb;        // rule 2: <|0.00|> opens the transcript
    else if (lse > text_best) tok = si;                     // rule 5: the timestamps' total mass beats every text token
    else tok = argmax_better(sm, si, tm, ti) ? si : ti;
    if constexpr (LP) {   // rule 5 leaves the timestamps alone in the softmax; otherwise text and timestamps share it
        for (int o = lpb >> 1; o >= 1; o >>= 1) lse_merge(xm, xs, __shfl_xor(xm, o), __shfl_xor(xs, o));
        lp->forced = cur_len == p.ts_begin_index - 1;
        lp->text_masked = !lp->forced && lse > text_best;
        lp->m = M;
        lp->s = Z;
        lp->num = SAMP ? ssc : sm;
        lp->key = sm;
        if (!lp->text_masked) {
            lse_merge(lp->m, lp->s, xm, xs);
            const bool ts_wins = argmax_better(sm, si, tm, ti);
            lp->num = SAMP ? (ts_wins ? ssc : tsc) : (ts_wins ? sm : tm);
            lp->key = ts_wins ? sm : tm;
        }
    }
    if ((unsigned)tok >= (unsigned)p.V) tok = p.eos;        // unreachable with a NaN-aware argmax; never index the embedding out of range
    if (b < p.B && l == 0) {
        if (p.ts_tok) p.ts_tok[b] = tok;
        if (p.ts_stats) {
            p.ts_stats[2 * b] = lse;
            p.ts_stats[2 * b + 1] = text_best;
        }
    }
    return tok;
}

// Final masked argmax of every row over its n_parts partial results (lowest index on ties), shared by the two finish kernels.  All rows
// at once: a group of `lpb` lanes per row (64 at B <= 4, 32 at B <= 8, 16 at B <= 16), every load of the block in flight together -- the
// partials were written by other XCDs a kernel ago, so this is one memory round trip; row by row it was B of them (measured 14 us per
// step at B = 8).  The candidates do not depend on DecState: the first 8 x lpb of a row are requested BEFORE it is read (one dependent
// round trip fewer), by unconditional clamped loads -- `finish_request` / `finish_argmax` are the two halves.
struct FinishCand {
    float pv[8];
    int pi[8];
};
__device__ __forceinline__ void finish_request(const SelectParams& p, const int b, const int l, const int lpb, FinishCand& c) {
    const size_t pbase = (size_t)min(b, p.B - 1) * p.n_parts;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = min(l + k * lpb, p.n_parts - 1);
        c.pv[k] = p.part_val[pbase + i];
        c.pi[k] = p.part_idx[pbase + i];
    }
}
// a row's log-sum-exp pairs over its n_parts partials (log-probability mode): lane l merges partials l, l + lpb, .. in that order, then the
// group's lanes merge by a butterfly -- a fixed order, so the result is bitwise repeatable; every lane of the group ends with the same pairs
__device__ __forceinline__ float4 finish_lse(const SelectParams& p, const int b, const int l, const int lpb) {
    const size_t pbase = (size_t)min(b, p.B - 1) * p.n_parts;
    float m = -INFINITY, s = 0.f, rm = -INFINITY, rs = 0.f;
    for (int i = l; i < p.n_parts; i += lpb) {
        const float4 v = p.lp_part[pbase + i];
        lse_merge(m, s, v.x, v.y);
        lse_merge(rm, rs, v.z, v.w);
    }
    for (int o = lpb >> 1; o >= 1; o >>= 1) {
        lse_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
        lse_merge(rm, rs, __shfl_xor(rm, o), __shfl_xor(rs, o));
    }
    return make_float4(m, s, rm, rs);
}
// SAMP: the partials' values are keys; the winner's score is fetched from samp_sc once the lane's own best partial is known
template <bool LP = false, bool SAMP = false>
__device__ __forceinline__ int finish_argmax(const SelectParams& p, const int b, const int l, const int lpb, const FinishCand& c,
                                             float* best_out = nullptr, float* score_out = nullptr) {
    const size_t pbase = (size_t)min(b, p.B - 1) * p.n_parts;
    float best = -INFINITY;
    int bidx = 0x7fffffff, bpart = -1;
    if (b < p.B) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (l + k * lpb < p.n_parts && argmax_better(c.pv[k], c.pi[k], best, bidx)) {
                best = c.pv[k];
                bidx = c.pi[k];
                if constexpr (SAMP) bpart = l + k * lpb;
            }
        for (int i = l + 8 * lpb; i < p.n_parts; i += lpb) {
            const float v = p.part_val[pbase + i];
            const int ix = p.part_idx[pbase + i];
            if (argmax_better(v, ix, best, bidx)) {
                best = v;
                bidx = ix;
                if constexpr (SAMP) bpart = i;
            }
        }
    }
    float bsc = -INFINITY;
    if constexpr (SAMP) {
        if (bpart >= 0) bsc = p.samp_sc[pbase + bpart];
    }
    for (int o = lpb >> 1; o >= 1; o >>= 1) {   // lpb <= 64 and a power of two: a group never straddles a wave
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        const float osc = SAMP ? __shfl_xor(bsc, o) : 0.f;
        if (argmax_better(ov, oi, best, bidx)) {
            best = ov;
            bidx = oi;
            if constexpr (SAMP) bsc = osc;
        }
    }
    if constexpr (LP) *best_out = best;
    if constexpr (SAMP) *score_out = bsc;
    if ((unsigned)bidx >= (unsigned)p.V) bidx = p.eos;   // unreachable with a NaN-aware argmax; never index the embedding out of range
    return bidx;
}
// input of the next step for every row: x[b] = embed_tokens[tok_b] + embed_positions[pos_b]   (model.py:423-425)
__device__ __forceinline__ void finish_embed(const SelectParams& p, const int* s_tok, const int* s_pos, const int tid) {
    const int d4 = p.d_model >> 2;
    for (int i = tid; i < p.B * d4; i += 256) {
        const int b = i / d4, c = i - b * d4;
        const float4 a = load_emb4(p.tok_emb, (size_t)s_tok[b] * p.d_model + 4 * c, p.emb_half != 0);
        const float4 q = reinterpret_cast<const float4*>(p.pos_emb + (size_t)s_pos[b] * p.d_model)[c];
        reinterpret_cast<float4*>(p.next_x + (size_t)b * p.d_model)[c] = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
    }
}

// TS: the timestamp mode's pick (ts_pick over ts_select_kernel's partials) instead of the plain argmax; the bookkeeping is shared
// LP: the log-probability mode -- token_logprob[b][cur_len] = s[tok] - logsumexp(s) over the step's processed scores s (0 at a forced
// position; the EOS score where a bench switch replaced the token), its running sum while the row is unfinished, and at step 0
// no_speech_prob = softmax(raw logits)[lp_ns].  The LP = false instantiations are the kernels as they were.
// SAMP (with LP): the partials are merged by their Gumbel-max key and the log-probability's numerator is the carried score of the winner.
template <bool TS, bool LP = false, bool SAMP = false>
__global__ __launch_bounds__(256) void greedy_finish_kernel(const SelectParams p) {
    static_assert(!SAMP || LP, "sampling runs with the log-sum-exp pairs on");
    __shared__ int s_tok[MAX_ROWS];
    __shared__ int s_pos[MAX_ROWS];
    __shared__ int s_unf[MAX_ROWS];
    DecState* st = p.st;
    const int tid = threadIdx.x;
    const int lpb = p.B <= 4 ? 64 : p.B <= 8 ? 32 : 16;
    const int b = tid / lpb, l = tid % lpb, bc = min(b, p.B - 1);
    FinishCand cand;
    TsPart tcand;
    float4 tsamp = float4{0.f, 0.f, 0.f, 0.f};
    if constexpr (TS) {
        ts_request(p, b, l, tcand);
        if constexpr (SAMP) tsamp = p.samp_ts[(size_t)bc * SELECT_CHUNKS + min(l, SELECT_CHUNKS - 1)];
    } else {
        finish_request(p, b, l, lpb, cand);
    }
    const int unf = p.unfinished[bc];
    // the rows of a wt_decoder_begin batch stay aligned in the id buffer: row 0's cur_len is everybody's.  The decoder position and the
    // self cache's key count are the row's own (they differ between rows behind prompts of unequal lengths, whose id rows are left-padded)
    const int done = st->done, cur_len = st->cur_len[0], step = st->step, seq = st->seq + 1, epoch = st->epoch;
    const int pos = st->pos[bc], my_pos = st->pos[min(tid, p.B - 1)], my_self_len = st->self_len[min(tid, p.B - 1)];
    if (done) {         // block-uniform: steps enqueued past the stop test are no-ops (the host still sees them retire)
        if (tid == 0) {
            st->seq = seq;
            unsigned unf_mask = 0;   // unchanged since the stop: the host may read this word instead of the stopping step's
            for (int r = 0; r < p.B; ++r) unf_mask |= p.unfinished[r] ? 1u << r : 0u;
            if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(epoch, seq, 1, cur_len, unf_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    // ForceTokensLogitsProcessor; at the language position the row's own token (host-chosen, or lang_select_kernel's earlier in this step)
    const int forced = p.lang_pos > 0 && cur_len == p.lang_pos ? p.lang_tok[bc] : p.forced[cur_len];
    const int row_eos = p.force_eos_rows ? p.force_eos_rows[bc] : -1;
    int tok;
    LpPick pick;
    float4 lse4;
    if constexpr (LP) lse4 = finish_lse(p, b, l, lpb);
    if constexpr (TS) {
        if constexpr (SAMP) tok = ts_pick<true, true>(p, b, l, lpb, tcand, st->cur_len[bc], &pick, tsamp);
        else if constexpr (LP) tok = ts_pick<true>(p, b, l, lpb, tcand, st->cur_len[bc], &pick);
        else tok = ts_pick(p, b, l, lpb, tcand, st->cur_len[bc]);
    } else {
        if constexpr (SAMP) {
            tok = finish_argmax<true, true>(p, b, l, lpb, cand, &pick.key, &pick.num);
            pick.m = lse4.x; pick.s = lse4.y; pick.forced = false; pick.text_masked = false;
        } else if constexpr (LP) {
            tok = finish_argmax<true>(p, b, l, lpb, cand, &pick.num);
            pick.m = lse4.x; pick.s = lse4.y; pick.forced = false; pick.text_masked = false;
        } else {
            tok = finish_argmax(p, b, l, lpb, cand);
        }
    }
    if (b < p.B && l == 0) {
        if constexpr (SAMP) {
            if (p.samp_key) p.samp_key[b] = pick.key;
        }
        if (forced >= 0) tok = forced;
        if (p.force_eos_step >= 0 && step == p.force_eos_step) tok = p.eos;  // bench-only transcript length
        if (row_eos >= 0 && step == row_eos) tok = p.eos;                    // ... per row (variable-length workload)
        if constexpr (LP) {
            if (unf) {
                float lpv;
                if (forced >= 0 || pick.forced) {   // one survivor at 0, the rest -inf (a bench switch may still have replaced it)
                    lpv = tok == (forced >= 0 ? forced : p.tb) ? 0.f : -INFINITY;
                } else {
                    float num = pick.num;
                    if ((p.force_eos_step >= 0 && step == p.force_eos_step) || (row_eos >= 0 && step == row_eos))
                        num = pick.text_masked && p.eos < p.tb ? -INFINITY : p.lp_side[2 * b];   // the switches replace the token, not the scores
                    lpv = (num - pick.m) - logf(pick.s);
                }
                p.lp_tok[(size_t)b * p.max_length + cur_len] = lpv;
                p.lp_sum[b] += lpv;
            }
            if (p.lp_ns >= 0 && step == 0) p.lp_nsp[b] = expf(p.lp_side[2 * b + 1] - lse4.z) / lse4.w;
        }
        if (!unf) tok = p.pad;                                 // finished rows keep emitting pad
        p.ids[(size_t)b * p.max_length + cur_len] = tok;
        if (tok == p.eos) p.unfinished[b] = 0;
        s_tok[b] = tok;
        s_pos[b] = pos + 1;
        s_unf[b] = (tok == p.eos) ? 0 : unf;
    }
    __syncthreads();   // (every thread has read the counters above before any of them is advanced)
    if (tid < p.B) {
        st->cur_len[tid] = cur_len + 1;
        st->pos[tid] = my_pos + 1;
        st->self_len[tid] = my_self_len + 1;
    }
    if (tid == 0) {
        int nu = 0;
        unsigned unf_mask = 0;
        for (int r = 0; r < p.B; ++r)
            if (s_unf[r]) {
                ++nu;
                unf_mask |= 1u << r;
            }
        st->n_unfinished = nu;
        st->step = step + 1;
        const int now_done = nu == 0 || cur_len + 1 >= p.max_length;   // run.py:219-226
        if (now_done) st->done = 1;
        st->seq = seq;
        // progress report for wt_decoder_run: one self-contained 64-bit word, written through to the pinned host page (the ids
        // themselves are fetched later by a stream-ordered copy, so no release fence -- and no L2 write-back -- is needed here)
        if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(epoch, seq, now_done, cur_len + 1, unf_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!p.next_x || cur_len + 1 >= p.max_length) return;
    finish_embed(p, s_tok, s_pos, tid);
}

// ---- language detection (wt_decoder_set_languages): openai-whisper's detect_language as a rule of the first step.  The step whose input is
// the start token already holds the hidden state detect_language computes, so one workgroup per row takes the logits of the listed
// language ids alone -- z[l] = dot(LayerNorm(x_b), E[lang_ids[l]]), the suppress lists do not apply --, their softmax and the argmax with
// torch.argmax's semantics over the masked vocabulary (NaN beats every number, equals go to the LOWEST TOKEN ID).  Every reduction runs in
// one fixed order inside the row's own workgroup: a row's result depends neither on its slot nor on B.  The embedding rows (<= 128 x d
// x 4 B) come from L2 once the first workgroup has read them.
__device__ __forceinline__ bool lang_better(const float az, const int ai, const float bz, const int bi) {
    const bool an = az != az, bn = bz != bz;
    if (an != bn) return an;
    if (!an && az != bz) return az > bz;
    return ai < bi;
}
__global__ __launch_bounds__(256) void lang_select_kernel(const LangSelectParams p) {
    __shared__ float4 xs[LANG_D_MAX / 4];
    __shared__ float zs[LANG_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = p.d, d4 = d >> 2;
    const float4* xrow = reinterpret_cast<const float4*>(p.x + (size_t)b * d);
    for (int i = tid; i < d4; i += 256) xs[i] = xrow[i];
    __syncthreads();
    if (p.ln_w) {   // every wave takes the statistics of the whole row, in the same order: no exchange between waves
        float sum = 0.f;
        for (int i = lane; i < d4; i += 64) sum += (xs[i].x + xs[i].y) + (xs[i].z + xs[i].w);
        const float mean = wave_allreduce_sum_d(sum) / d;
        float q = 0.f;
        for (int i = lane; i < d4; i += 64) {
            const float a = xs[i].x - mean, c = xs[i].y - mean, e = xs[i].z - mean, f = xs[i].w - mean;
            q += (a * a + c * c) + (e * e + f * f);
        }
        const float rstd = rsqrtf(wave_allreduce_sum_d(q) / d + 1e-5f);
        __syncthreads();   // every wave has read the raw row
        for (int i = tid; i < d4; i += 256) {
            const float4 v = xs[i], g = reinterpret_cast<const float4*>(p.ln_w)[i], be = reinterpret_cast<const float4*>(p.ln_b)[i];
            xs[i] = make_float4((v.x - mean) * rstd * g.x + be.x, (v.y - mean) * rstd * g.y + be.y, (v.z - mean) * rstd * g.z + be.z,
                                (v.w - mean) * rstd * g.w + be.w);
        }
        __syncthreads();
    }
    // a wave per language: 16-byte loads of the embedding row (d4 <= 5 x 64 chunks, all requested before the first use)
    for (int l = wave; l < p.n_lang; l += 4) {
        const size_t row = (size_t)p.lang_ids[l] * d;
        float4 ev[LANG_D_MAX / 256];
#pragma unroll
        for (int v = 0; v < LANG_D_MAX / 256; ++v) {
            const int i = lane + 64 * v;
            ev[v] = i < d4 ? load_emb4(p.emb, row + 4 * (size_t)i, p.emb_half != 0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < LANG_D_MAX / 256; ++v) {
            const int i = lane + 64 * v;
            if (i < d4) acc += dot4(xs[i], ev[v]);
        }
        acc = wave_allreduce_sum_d(acc);
        if (lane == 0) zs[l] = acc;
    }
    __syncthreads();
    if (wave != 0) return;
    const int l0 = lane, l1 = lane + 64;
    const float z0 = l0 < p.n_lang ? zs[l0] : -INFINITY, z1 = l1 < p.n_lang ? zs[l1] : -INFINITY;
    float m = fmaxf(z0, z1);   // (fmaxf drops a NaN: the maximum of the numbers; a NaN logit then makes the sum, and every probability, NaN)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float e0 = l0 < p.n_lang ? expf(z0 - m) : 0.f, e1 = l1 < p.n_lang ? expf(z1 - m) : 0.f;
    const float sum = wave_allreduce_sum_d(e0 + e1);
    if (l0 < p.n_lang) p.lang_prob[(size_t)b * p.n_lang + l0] = e0 / sum;
    if (l1 < p.n_lang) p.lang_prob[(size_t)b * p.n_lang + l1] = e1 / sum;
    const int i0 = l0 < p.n_lang ? p.lang_ids[l0] : 0x7fffffff, i1 = l1 < p.n_lang ? p.lang_ids[l1] : 0x7fffffff;
    float bz = z0;
    int bi = i0;
    if (lang_better(z1, i1, bz, bi)) { bz = z1; bi = i1; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {   // a strict total order over distinct ids: the winner does not depend on the order of the exchange
        const float oz = __shfl_xor(bz, o);
        const int oi = __shfl_xor(bi, o);
        if (lang_better(oz, oi, bz, bi)) { bz = oz; bi = oi; }
    }
    if (lane == 0 && p.lang_tok[b] < 0) p.lang_tok[b] = bi;
}
hipError_t launch_lang_select(const LangSelectParams& p, hipStream_t s) {
    if (!p.x || !p.emb || !p.lang_ids || !p.lang_tok || !p.lang_prob || (p.ln_w == nullptr) != (p.ln_b == nullptr)) return hipErrorInvalidValue;
    if (p.B < 1 || p.B > MAX_ROWS || p.n_lang < 1 || p.n_lang > LANG_MAX || p.d < 4 || p.d > LANG_D_MAX || (p.d & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lang_select_kernel, dim3(p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---- continuous mode (wt_decoder_stream_*): every slot at its own position; a row that stops is replaced AT ONCE, by this kernel, with
// the next utterance of the waiting queue (its cross K/V were projected into a pool row beforehand): no step is spent on a finished
// row and no host round trip sits between an EOS and the next utterance's first token.  The reference gets per-utterance stopping from
// decoding one clip at a time (run.py:219-226); here the batch stays full instead.
// Host visibility: every token of an active slot also goes to the pinned id row of its pool row, and a stopping row publishes its final
// length there behind a system-scope fence -- the host never copies ids from the device in this mode.
__device__ __forceinline__ bool stream_admit(const SelectParams& p, DecState* st, const int b, int* s_tok, int* s_pos) {
    const int head = st->q_head;
    if (head >= st->q_tail) {   // nothing waiting: the slot idles (pad at its frozen position: finite, unused)
        st->slot_row[b] = -1;
        p.unfinished[b] = 0;
        s_tok[b] = p.pad;
        s_pos[b] = 0;
        return false;
    }
    const int r = st->queue[head % STREAM_QCAP];
    st->q_head = head + 1;
    st->slot_row[b] = r;
    st->cur_len[b] = 1;
    st->pos[b] = 0;
    st->self_len[b] = 0;
    st->row_force[b] = st->rec_force[r];
    p.unfinished[b] = 1;
    p.ids[(size_t)b * p.max_length] = p.start_token;
    __hip_atomic_store(p.host_ids + (size_t)r * p.max_length, p.start_token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    s_tok[b] = p.start_token;
    s_pos[b] = 0;
    return true;
}
__device__ __forceinline__ void stream_report(const SelectParams& p, DecState* st, const int seq) {   // thread 0, after the admissions
    int na = 0;
    unsigned mask = 0;
    for (int r = 0; r < p.B; ++r)
        if (st->slot_row[r] >= 0) {
            ++na;
            mask |= 1u << r;
        }
    st->n_unfinished = na;
    st->done = na == 0;
    st->seq = seq;
    if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(st->epoch, seq, na == 0, st->q_head & 0x7fff, mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void stream_finish_kernel(const SelectParams p) {
    __shared__ int s_tok[MAX_ROWS];
    __shared__ int s_pos[MAX_ROWS];
    __shared__ int s_fin[MAX_ROWS];
    DecState* st = p.st;
    const int tid = threadIdx.x;
    const int lpb = p.B <= 4 ? 64 : p.B <= 8 ? 32 : 16;
    const int b = tid / lpb, l = tid % lpb, bc = min(b, p.B - 1);
    FinishCand cand;
    finish_request(p, b, l, lpb, cand);
    const int row = st->slot_row[bc], cur_len = st->cur_len[bc], pos = st->pos[bc], eos_at = st->row_force[bc];
    const int done = st->done, seq = st->seq + 1;
    if (done) {   // block-uniform: nothing active, nothing waiting -- a surplus step behind the last utterance
        if (tid == 0) {
            st->seq = seq;
            if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(st->epoch, seq, 1, st->q_head & 0x7fff, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const int forced = p.forced[min(cur_len, p.max_length)];
    int tok = finish_argmax(p, b, l, lpb, cand);
    if (b < p.B && l == 0) {
        int fin = 0;
        if (row >= 0) {
            if (forced >= 0) tok = forced;
            if (eos_at >= 0 && cur_len - 1 == eos_at) tok = p.eos;   // bench only: this utterance's transcript length
            p.ids[(size_t)b * p.max_length + cur_len] = tok;
            __hip_atomic_store(p.host_ids + (size_t)row * p.max_length + cur_len, tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            fin = tok == p.eos || cur_len + 1 >= p.max_length;        // this utterance's own stop test (run.py:219-226 at batch 1)
            if (fin) {   // release: every id of the row (this thread's own stores, this step's and the earlier kernels') is in host memory
                         // before its length says so
                __hip_atomic_store(p.host_len + row, cur_len + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                st->cur_len[b] = cur_len + 1;
                st->pos[b] = pos + 1;
                st->self_len[b] = pos + 1;
                s_tok[b] = tok;
                s_pos[b] = pos + 1;
            }
        }
        s_fin[b] = fin || row < 0;   // stopped just now, or idle: both take the next waiting utterance if there is one
    }
    __syncthreads();
    if (tid == 0) {
        for (int r = 0; r < p.B; ++r)
            if (s_fin[r]) stream_admit(p, st, r, s_tok, s_pos);
        st->step += 1;
        stream_report(p, st, seq);
    }
    __syncthreads();
    if (!p.next_x) return;
    finish_embed(p, s_tok, s_pos, tid);
}

// host -> device hand-over of prepared utterances (stream-ordered behind their cross-K/V projection): append to the waiting queue,
// then fill idle slots directly -- so a decode that had drained (or has not started) begins without a wasted step
__global__ __launch_bounds__(256) void stream_publish_kernel(const SelectParams p, const StreamPublish pub) {
    __shared__ int s_tok[MAX_ROWS];
    __shared__ int s_pos[MAX_ROWS];
    __shared__ int s_new[MAX_ROWS];
    DecState* st = p.st;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int tail = st->q_tail;
        for (int i = 0; i < pub.n; ++i) {
            st->queue[tail % STREAM_QCAP] = pub.rows[i];
            st->rec_force[pub.rows[i]] = pub.force[i];
            ++tail;
        }
        st->q_tail = tail;
        for (int r = 0; r < p.B; ++r) s_new[r] = st->slot_row[r] < 0 ? (stream_admit(p, st, r, s_tok, s_pos) ? 1 : 0) : 0;
        int na = 0;
        for (int r = 0; r < p.B; ++r) na += st->slot_row[r] >= 0;
        st->n_unfinished = na;
        st->done = na == 0;
    }
    __syncthreads();
    // the first input of the admitted slots (the others keep the input their last step left)
    const int d4 = p.d_model >> 2;
    for (int i = tid; i < p.B * d4; i += 256) {
        const int b = i / d4, c = i - b * d4;
        if (!s_new[b]) continue;
        const float4 a = load_emb4(p.tok_emb, (size_t)s_tok[b] * p.d_model + 4 * c, p.emb_half != 0);
        const float4 q = reinterpret_cast<const float4*>(p.pos_emb + (size_t)s_pos[b] * p.d_model)[c];
        reinterpret_cast<float4*>(p.next_x + (size_t)b * p.d_model)[c] = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
    }
}
hipError_t launch_stream_publish(const SelectParams& p, const StreamPublish& pub, hipStream_t s) {
    if (p.B < 1 || p.B > MAX_ROWS || pub.n < 0 || pub.n > MAX_ROWS || !p.host_ids || !p.host_len || !p.next_x) return hipErrorInvalidValue;
    for (int i = 0; i < pub.n; ++i)
        if (pub.rows[i] < 0 || pub.rows[i] >= STREAM_QCAP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_publish_kernel, dim3(1), dim3(256), 0, s, p, pub);
    return hipGetLastError();
}

// ---- beam search (wt_decoder_set_beam_search): the reference's beam_search (transformers generation/utils.py) with BeamSearchScorer /
// BeamHypotheses (generation/beam_search.py), one group and one returned hypothesis per utterance.  Rows are [utterance][beam].  Per
// step: scores = log_softmax(logits) over the whole vocabulary, THEN Suppress -> SuppressAtBegin -> Force on the log-probabilities,
// plus the row's running beam score; per utterance the 2 * nb best of the nb * V candidates, sorted, lowest flat index (beam * V + id)
// first among equals; walking them, an EOS candidate of rank < nb becomes a finished hypothesis and the first nb others the next beams.
//   beam_select_kernel  grid (SELECT_CHUNKS, B): per chunk the (max, sum-exp) pair over ALL ids and the 2 * nb best ids under the masks;
//   beam_finish_kernel  one block, a wave per utterance: merge, top 2 * nb, the scorer's `process` (hypothesis store, is_done), then
//                       the block re-parents id history and ancestry table and does greedy_finish_kernel's bookkeeping;
//   beam_finalize_kernel grid (U): BeamSearchScorer.finalize (open beams of unfinished utterances join, best hypothesis out).
// A NaN logit is a candidate that ranks first (as in the argmax kernels) and is left out of the log-sum-exp of its row.
constexpr int BEAM_NONE = 0x7fffffff;

__device__ __forceinline__ void beam_wave_best(float& v, int& i) {   // all-reduce of the best (v, i) over a wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (argmax_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}
__device__ __forceinline__ void beam_wave_lse(float& m, float& s) {   // all-reduce of an online (max, sum-exp) pair over a wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float om = __shfl_xor(m, o), os = __shfl_xor(s, o);
        const float nm = fmaxf(m, om);
        s = ts_rescale(s, m, nm) + ts_rescale(os, om, nm);
        m = nm;
    }
}

__global__ __launch_bounds__(256) void beam_select_kernel(const SelectParams p) {
    __shared__ float s_v[4][BEAM_KMAX];
    __shared__ int s_i[4][BEAM_KMAX];
    __shared__ float s_m[4], s_s[4];
    const DecState* st = p.st;
    if (st->done) return;  // steps enqueued past the stop test are no-ops
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x, b = blockIdx.y;
    const bool at_begin = st->cur_len[b] == p.begin_index;
    const int K = 2 * p.beam.nb;
    const float* lg = p.logits + (size_t)b * p.V;
    const int per = (p.V + SELECT_CHUNKS - 1) / SELECT_CHUNKS;
    const int v0 = chunk * per, v1 = min(p.V, v0 + per);
    // the log-softmax denominator runs over every id, masked or not (the processors act on the log-probabilities)
    float m = -INFINITY, z = 0.f;
    for (int v = v0 + tid; v < v1; v += 256) {
        const float x = lg[v];
        if (x > m) {
            z = ts_rescale(z, m, x) + 1.f;
            m = x;
        } else if (x == x && x != -INFINITY) {
            z += expf(x - m);
        }
    }
    beam_wave_lse(m, z);
    if (lane == 0) {
        s_m[wave] = m;
        s_s[wave] = z;
    }
    // every wave's K best ids, in order: round r takes the best id that ranks after round r - 1's (the chunk stays in L1 / L2)
    float pv = 0.f;
    int pi = -1;
    for (int r = 0; r < K; ++r) {
        float bv = -INFINITY;
        int bi = BEAM_NONE;
        for (int v = v0 + tid; v < v1; v += 256) {
            float x = lg[v];
            const uint8_t mk = p.mask[v];
            if ((mk & 1) || ((mk & 2) && at_begin)) x = -INFINITY;
            if ((r == 0 || argmax_better(pv, pi, x, v)) && argmax_better(x, v, bv, bi)) {
                bv = x;
                bi = v;
            }
        }
        beam_wave_best(bv, bi);
        if (lane == 0) {
            s_v[wave][r] = bv;
            s_i[wave][r] = bi;
        }
        pv = bv;
        pi = bi;
        if (bi == BEAM_NONE) {   // wave-uniform: the wave's ids are used up
            if (lane == 0)
                for (int k = r + 1; k < K; ++k) s_i[wave][k] = BEAM_NONE;
            break;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // the four sorted lists, one candidate per lane, merged into the chunk's K best
    const int w = lane / BEAM_KMAX, k = lane % BEAM_KMAX;
    float cv = -INFINITY;
    int ci = BEAM_NONE;
    if (k < K) {
        cv = s_v[w][k];
        ci = s_i[w][k];
    }
    float M = lane < 4 ? s_m[lane] : -INFINITY, Z = lane < 4 ? s_s[lane] : 0.f;
    beam_wave_lse(M, Z);
    BeamPart* out = p.beam.part + (size_t)b * SELECT_CHUNKS + chunk;
    if (lane == 0) {
        out->m = M;
        out->s = Z;
    }
    for (int r = 0; r < K; ++r) {
        float bv = ci == BEAM_NONE ? -INFINITY : cv;
        int bi = ci;
        beam_wave_best(bv, bi);
        if (bi != BEAM_NONE && bi == ci) ci = BEAM_NONE;   // taken
        if (lane == 0) {
            out->val[r] = bv;
            out->idx[r] = bi == BEAM_NONE ? -1 : bi;
        }
    }
}

// BeamHypotheses.add for utterance u (a whole wave calls it; lane 0 keeps the books, every lane copies ids): `sum` = the candidate's
// sum of log-probabilities, `src` = the hypothesis' ids (length len, the EOS not included)
__device__ __forceinline__ void beam_hyp_add(const BeamParams& bp, const int u, const int* src, const int len, const float sum, const int lane) {
    int slot = -1;
    if (lane == 0) {
        const int nb = bp.nb;
        const double score = (double)sum / pow((double)len, (double)bp.length_penalty);
        const int n = bp.hyp_n[u];
        const double worst = bp.hyp_worst[u];
        double* hs = bp.hyp_score + (size_t)u * nb;
        if (n < nb) {
            slot = n;
            bp.hyp_n[u] = n + 1;
            bp.hyp_worst[u] = score < worst ? score : worst;
        } else if (score > worst) {   // the worst kept hypothesis leaves; the new worst is the smallest of the rest and the newcomer
            int lo = 0;
            for (int k = 1; k < nb; ++k)
                if (hs[k] < hs[lo]) lo = k;
            double nw = score;
            for (int k = 0; k < nb; ++k)
                if (k != lo && hs[k] < nw) nw = hs[k];
            slot = lo;
            bp.hyp_worst[u] = nw;
        }
        if (slot >= 0) {
            hs[slot] = score;
            bp.hyp_len[u * nb + slot] = len;
        }
    }
    slot = __shfl(slot, 0);
    if (slot < 0) return;
    int* dst = bp.hyp_ids + ((size_t)u * bp.nb + slot) * bp.hyp_ld;
    for (int i = lane; i < len; i += 64) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void beam_finish_kernel(const SelectParams p) {
    __shared__ int s_tok[MAX_ROWS];
    __shared__ int s_pos[MAX_ROWS];
    __shared__ int s_unf[MAX_ROWS];
    __shared__ int s_src[MAX_ROWS];     // the row whose history row b continues
    __shared__ float s_sc[MAX_ROWS];
    __shared__ float s_tv[4][BEAM_KMAX];
    __shared__ int s_tf[4][BEAM_KMAX];
    DecState* st = p.st;
    const BeamParams& bp = p.beam;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = bp.nb, U = bp.U, K = 2 * nb, R = p.B;
    // the rows of a wt_decoder_begin batch stay aligned: row 0's counters are everybody's
    const int done = st->done, cur_len = st->cur_len[0], step = st->step, pos = st->pos[0], self_len = st->self_len[0], seq = st->seq + 1,
              epoch = st->epoch;
    if (done) {         // block-uniform: steps enqueued past the stop test are no-ops (the host still sees them retire)
        if (tid == 0) {
            st->seq = seq;
            unsigned unf_mask = 0;
            for (int r = 0; r < R; ++r) unf_mask |= p.unfinished[r] ? 1u << r : 0u;
            if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(epoch, seq, 1, cur_len, unf_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const int forced = p.forced[cur_len];                          // ForceTokensLogitsProcessor: 0 at the forced id, -inf elsewhere
    const int par = step & 1;
    const int* ids_cur = par ? bp.ids2 : p.ids;
    int* ids_nxt = par ? p.ids : bp.ids2;
    const int* anc_cur = bp.anc + (size_t)par * MAX_ROWS * bp.anc_ld;
    int* anc_nxt = bp.anc + (size_t)(par ^ 1) * MAX_ROWS * bp.anc_ld;
    for (int u = wave; u < U; u += 4) {   // wave-uniform
        const int r0 = u * nb;
        if (bp.hyp_done[u]) {   // a finished utterance's rows are padded
            if (lane < nb) {
                s_tok[r0 + lane] = p.pad;
                s_src[r0 + lane] = r0 + lane;
                s_sc[r0 + lane] = 0.f;
                s_unf[r0 + lane] = 0;
            }
            if (bp.dbg_cand && lane < BEAM_KMAX) bp.dbg_cand[(u * BEAM_KMAX + lane) * 3] = -1;
            continue;
        }
        // lane j keeps beam j's log-sum-exp and running score
        float my_lse = 0.f;
        const float my_bs = bp.scores[r0 + min(lane, nb - 1)];
        for (int j = 0; j < nb; ++j) {
            float m = -INFINITY, z = 0.f;
            if (lane < SELECT_CHUNKS) {
                const BeamPart* q = bp.part + (size_t)(r0 + j) * SELECT_CHUNKS + lane;
                m = q->m;
                z = q->s;
            }
            beam_wave_lse(m, z);
            if (lane == j) my_lse = m + logf(z);
        }
        // the utterance's nb * SELECT_CHUNKS * K candidates, up to 16 per lane: score and flat index beam * V + id
        const int n_c = nb * SELECT_CHUNKS * K;
        float cv[16];
        int cf[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = lane + 64 * i;
            const int j = min(forced >= 0 ? c : c / (SELECT_CHUNKS * K), nb - 1);
            const float lse_j = __shfl(my_lse, j), bs_j = __shfl(my_bs, j);
            cv[i] = -INFINITY;
            cf[i] = BEAM_NONE;
            if (forced >= 0) {
                if (c < nb) {
                    cv[i] = 0.f + bs_j;
                    cf[i] = c * p.V + forced;
                }
            } else if (c < n_c) {
                const int rem = c - j * (SELECT_CHUNKS * K);
                const BeamPart* q = bp.part + (size_t)(r0 + j) * SELECT_CHUNKS + rem / K;
                const int idx = q->idx[rem % K];
                if (idx >= 0) {
                    cv[i] = (q->val[rem % K] - lse_j) + bs_j;
                    cf[i] = j * p.V + idx;
                }
            }
        }
        unsigned taken = 0;
        for (int r = 0; r < K; ++r) {
            float bv = -INFINITY;
            int bf = BEAM_NONE;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (!((taken >> i) & 1u) && cf[i] != BEAM_NONE && argmax_better(cv[i], cf[i], bv, bf)) {
                    bv = cv[i];
                    bf = cf[i];
                }
            beam_wave_best(bv, bf);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (bf != BEAM_NONE && cf[i] == bf) taken |= 1u << i;
            if (lane == 0) {
                s_tv[wave][r] = bv;
                s_tf[wave][r] = bf;
                if (bp.dbg_cand) {
                    int* dc = bp.dbg_cand + (u * BEAM_KMAX + r) * 3;
                    dc[0] = bf == BEAM_NONE ? -1 : bf % p.V;
                    dc[1] = bf == BEAM_NONE ? -1 : bf / p.V;
                    dc[2] = __float_as_int(bv);
                }
            }
        }
        if (bp.dbg_cand && lane >= K && lane < BEAM_KMAX) bp.dbg_cand[(u * BEAM_KMAX + lane) * 3] = -1;
        __builtin_amdgcn_wave_barrier();
        // BeamSearchScorer.process
        int bi = 0;
        for (int r = 0; r < K && bi < nb; ++r) {
            const float sc = s_tv[wave][r];
            const int f = s_tf[wave][r];
            if (f == BEAM_NONE) break;
            const int j = f / p.V, tok = f - j * p.V;
            if (tok == p.eos) {
                if (r >= nb) continue;   // an EOS below the top nb is dropped
                beam_hyp_add(bp, u, ids_cur + (size_t)(r0 + j) * p.max_length, cur_len, sc, lane);
            } else {
                if (lane == 0) {
                    s_tok[r0 + bi] = tok;
                    s_src[r0 + bi] = r0 + j;
                    s_sc[r0 + bi] = sc;
                }
                ++bi;
            }
        }
        for (; bi < nb; ++bi)   // fewer than nb continuations (the reference raises): the row dies with a score of -inf
            if (lane == 0) {
                s_tok[r0 + bi] = p.pad;
                s_src[r0 + bi] = r0 + bi;
                s_sc[r0 + bi] = -INFINITY;
            }
        int udone = 0;
        if (lane == 0) {   // BeamHypotheses.is_done(best candidate score of the step, cur_len + 1)
            if (bp.hyp_n[u] >= nb) {
                if (bp.early_stopping) udone = 1;
                else udone = bp.hyp_worst[u] >= (double)s_tv[wave][0] / pow((double)(cur_len + 1), (double)bp.length_penalty);
            }
            bp.hyp_done[u] = udone;
        }
        udone = __shfl(udone, 0);
        if (lane < nb) s_unf[r0 + lane] = !udone;
    }
    __syncthreads();
    // every row: re-parent the id history and the ancestry table into the other buffer, append the token
    for (int i = tid; i < R * cur_len; i += 256) {
        const int b = i / cur_len, c = i - b * cur_len;
        ids_nxt[(size_t)b * p.max_length + c] = ids_cur[(size_t)s_src[b] * p.max_length + c];
    }
    for (int i = tid; i < R * self_len; i += 256) {
        const int b = i / self_len, c = i - b * self_len;
        anc_nxt[(size_t)b * bp.anc_ld + c] = anc_cur[(size_t)s_src[b] * bp.anc_ld + c];
    }
    if (tid < R) {
        const int b = tid;
        ids_nxt[(size_t)b * p.max_length + cur_len] = s_tok[b];
        anc_nxt[(size_t)b * bp.anc_ld + self_len] = s_src[b];            // this step's key was appended to the source row
        if (self_len + 1 < bp.anc_ld) anc_nxt[(size_t)b * bp.anc_ld + self_len + 1] = b;   // the next step's key goes to the row itself
        bp.scores[b] = s_sc[b];
        p.unfinished[b] = s_unf[b];
        s_pos[b] = pos + 1;
        st->cur_len[b] = cur_len + 1;
        st->pos[b] = pos + 1;
        st->self_len[b] = self_len + 1;
        if (bp.trace) {
            int* tr = bp.trace + ((size_t)step * R + b) * 4;
            tr[0] = s_tok[b];
            tr[1] = s_src[b] - (b / nb) * nb;
            tr[2] = __float_as_int(s_sc[b]);
            tr[3] = !s_unf[b];
        }
    }
    if (tid == 0) {
        int nu = 0;
        unsigned unf_mask = 0;
        for (int r = 0; r < R; ++r)
            if (s_unf[r]) {
                ++nu;
                unf_mask |= 1u << r;
            }
        st->n_unfinished = nu;
        st->step = step + 1;
        const int now_done = nu == 0 || cur_len + 1 >= p.max_length;   // beam_scorer.is_done or MaxLengthCriteria
        if (now_done) st->done = 1;
        st->seq = seq;
        if (p.mailbox) __hip_atomic_store(p.mailbox, mailbox_word(epoch, seq, now_done, cur_len + 1, unf_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!p.next_x || cur_len + 1 >= p.max_length) return;
    __syncthreads();   // s_pos
    finish_embed(p, s_tok, s_pos, tid);
}

__global__ __launch_bounds__(256) void beam_finalize_kernel(const SelectParams p) {
    __shared__ int s_pick[2];
    __shared__ float s_score;
    const BeamParams& bp = p.beam;
    const DecState* st = p.st;
    const int u = blockIdx.x, tid = threadIdx.x, nb = bp.nb, cur_len = st->cur_len[0];
    const int* ids_cur = (st->step & 1) ? bp.ids2 : p.ids;
    if (tid == 0) {   // a copy of the utterance's store, joined by its open beams unless it is done (the store itself is left alone)
        double sc[MAX_BEAMS];
        int src[MAX_BEAMS], len[MAX_BEAMS];
        int n = bp.hyp_n[u];
        double worst = bp.hyp_worst[u];
        for (int k = 0; k < n; ++k) {
            sc[k] = bp.hyp_score[(size_t)u * nb + k];
            src[k] = k;
            len[k] = bp.hyp_len[u * nb + k];
        }
        if (!bp.hyp_done[u])
            for (int j = 0; j < nb; ++j) {
                const double score = (double)bp.scores[u * nb + j] / pow((double)cur_len, (double)bp.length_penalty);
                int slot = -1;
                if (n < nb) {
                    slot = n++;
                    worst = score < worst ? score : worst;
                } else if (score > worst) {
                    int lo = 0;
                    for (int k = 1; k < nb; ++k)
                        if (sc[k] < sc[lo]) lo = k;
                    worst = score;
                    for (int k = 0; k < nb; ++k)
                        if (k != lo && sc[k] < worst) worst = sc[k];
                    slot = lo;
                }
                if (slot >= 0) {
                    sc[slot] = score;
                    src[slot] = nb + j;
                    len[slot] = cur_len;
                }
            }
        int best = 0;   // (exactly equal scores: the highest slot; the reference's choice there is its sort's, whisper_trtllm_amd.h (9c))
        for (int k = 1; k < n; ++k)
            if (sc[k] >= sc[best]) best = k;
        s_pick[0] = n > 0 ? src[best] : nb;
        s_pick[1] = n > 0 ? len[best] : cur_len;
        s_score = n > 0 ? (float)sc[best] : 0.f;
    }
    __syncthreads();
    const int pick = s_pick[0], len = s_pick[1];
    const int* src = pick < nb ? bp.hyp_ids + ((size_t)u * nb + pick) * bp.hyp_ld : ids_cur + (size_t)(u * nb + pick - nb) * p.max_length;
    int* row = bp.out_ids + (size_t)u * p.max_length;
    for (int i = tid; i < p.max_length; i += 256) row[i] = i < len ? src[i] : i == len ? p.eos : p.pad;
    if (tid == 0) bp.out_scores[u] = s_score;
}

__global__ void beam_init_kernel(const SelectParams p) {
    const BeamParams& bp = p.beam;
    const int t = threadIdx.x;
    if (t < MAX_ROWS) {
        bp.urow[t] = min(t / bp.nb, bp.U - 1);
        bp.anc[(size_t)t * bp.anc_ld] = t;
        if (t < p.B) bp.scores[t] = t % bp.nb == 0 ? 0.f : -1e9f;
    }
    if (t < bp.U) {
        bp.hyp_n[t] = 0;
        bp.hyp_done[t] = 0;
        bp.hyp_worst[t] = 1e9;
    }
}
static bool beam_params_ok(const SelectParams& p) {
    const BeamParams& b = p.beam;
    return b.nb >= 2 && b.nb <= MAX_BEAMS && b.U >= 1 && b.U * b.nb == p.B && p.B <= MAX_ROWS && !p.fused && !p.stream && !p.ts_on && !p.trace &&
           b.part && b.scores && b.ids2 && b.anc && b.urow && b.hyp_n && b.hyp_done && b.hyp_worst && b.hyp_score && b.hyp_len && b.hyp_ids &&
           b.out_ids && b.out_scores && b.hyp_ld >= p.max_length && b.anc_ld >= p.max_length && p.V >= 1 && (long long)b.nb * p.V < BEAM_NONE;
}
hipError_t launch_beam_init(const SelectParams& p, hipStream_t s) {
    if (!beam_params_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_init_kernel, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_beam_finalize(const SelectParams& p, hipStream_t s) {
    if (!beam_params_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(p.beam.U), dim3(256), 0, s, p);
    return hipGetLastError();
}

// temperature sampling over logits in memory: sample_select_kernel in the plan of the sampling GEMV for (B, V, samp_K), then the finish kernel
static hipError_t launch_sample_select(const SelectParams& p, hipStream_t s) {
    if (!p.lp_on || p.stream || p.beam_on || !p.samp_seeds || !p.samp_sc || !(p.samp_temp > 0.f) || !p.lp_part || !p.lp_side || !p.lp_tok ||
        !p.lp_sum || p.lp_ns >= p.V || (p.lp_ns >= 0 && !p.lp_nsp))
        return hipErrorInvalidValue;
    SkinnyParams k;
    memset(&k, 0, sizeof k);
    k.B = p.B; k.N = p.V; k.K = p.samp_K; k.ymode = YMODE_ARGMAX; k.am_samp = 1;
    SkinnyPlan pl;
    int nw = 0;   // waves per workgroup of the sampling shape
    const hipError_t e = skinny_for_batch<true>(p.B, [&](auto sh) {
        nw = sh.NW;
        return skinny_plan<decltype(sh)>(k, &pl);
    });
    if (e != hipSuccess) return e;
    const int G = nw / pl.nsplit;
    if (p.samp_parts_cap < pl.grid) return hipErrorInvalidValue;
    SelectParams q = p;
    q.n_parts = pl.grid;
    hipLaunchKernelGGL(sample_select_kernel, dim3(pl.grid, p.B), dim3(64), 0, s, q, pl.rows_per_group, G);
    hipLaunchKernelGGL((greedy_finish_kernel<false, true, true>), dim3(1), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_greedy_select(const SelectParams& p, hipStream_t s) {
    if (p.B > MAX_ROWS || p.n_parts < 1 || (!p.fused && p.n_parts != SELECT_CHUNKS)) return hipErrorInvalidValue;
    if (p.samp_on && !p.fused && !p.ts_on) return launch_sample_select(p, s);
    if (p.stream && (!p.host_ids || !p.host_len || p.trace)) return hipErrorInvalidValue;
    if (p.lp_on && (p.beam_on || !p.lp_part || !p.lp_side || !p.lp_tok || !p.lp_sum || p.lp_ns >= p.V || (p.lp_ns >= 0 && !p.lp_nsp)))
        return hipErrorInvalidValue;
    if (p.samp_on && (!p.lp_on || p.stream || !p.samp_seeds || !(p.samp_temp > 0.f) || (p.ts_on ? !p.samp_ts : !p.samp_sc)))
        return hipErrorInvalidValue;
    if (p.beam_on) {   // beam search: batch decodes only, over logits in HBM
        if (!beam_params_ok(p)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(beam_select_kernel, dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);
        hipLaunchKernelGGL(beam_finish_kernel, dim3(1), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    if (p.ts_on) {   // timestamp mode: batch decodes only, over logits in HBM
        if (p.fused || p.stream || !p.ts_part || p.tb <= 0 || p.tb >= p.V || p.no_ts < 0 || p.no_ts >= p.tb || p.ts_begin_index < 2)
            return hipErrorInvalidValue;
        if (p.samp_on) {
            hipLaunchKernelGGL((ts_select_kernel<true, true>), dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);
            hipLaunchKernelGGL((greedy_finish_kernel<true, true, true>), dim3(1), dim3(256), 0, s, p);
        } else if (p.lp_on) {
            hipLaunchKernelGGL(ts_select_kernel<true>, dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);
            hipLaunchKernelGGL((greedy_finish_kernel<true, true>), dim3(1), dim3(256), 0, s, p);
        } else {
            hipLaunchKernelGGL(ts_select_kernel<false>, dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);
            hipLaunchKernelGGL(greedy_finish_kernel<true>, dim3(1), dim3(256), 0, s, p);
        }
        return hipGetLastError();
    }
    if (p.lp_on) {   // log-probability mode: batch decodes only; the same launch count as the plain tail
        if (p.stream) return hipErrorInvalidValue;
        if (p.samp_on) {   // temperature sampling, fused: the GEMV's sampling epilogue wrote the partials (else: launch_sample_select)
            hipLaunchKernelGGL((greedy_finish_kernel<false, true, true>), dim3(1), dim3(256), 0, s, p);
            return hipGetLastError();
        }
        if (!p.fused) hipLaunchKernelGGL(greedy_select_kernel<true>, dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);
        hipLaunchKernelGGL((greedy_finish_kernel<false, true>), dim3(1), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    if (!p.fused) hipLaunchKernelGGL(greedy_select_kernel<false>, dim3(SELECT_CHUNKS, p.B), dim3(256), 0, s, p);  // else: done by the vocabulary GEMV
    if (p.stream) hipLaunchKernelGGL(stream_finish_kernel, dim3(1), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(greedy_finish_kernel<false>, dim3(1), dim3(256), 0, s, p);
    return hipGetLastError();
}

__global__ void dec_init_kernel(DecState* st, int* ids, int* unfinished, int B, int max_length, int start_token, int epoch) {
    const int t = threadIdx.x;
    if (t == 0) {
        st->done = max_length <= 1 ? 1 : 0;
        st->n_unfinished = B;
        st->step = 0;
        st->seq = 0;
        st->epoch = epoch;
        st->q_head = st->q_tail = 0;
    }
    if (t < MAX_ROWS) {
        st->cur_len[t] = 1;
        st->pos[t] = 0;
        st->self_len[t] = 0;
        st->slot_row[t] = t;
        st->row_force[t] = -1;
    }
    for (int b = t; b < B; b += blockDim.x) {
        ids[(size_t)b * max_length] = start_token;
        unfinished[b] = 1;
    }
}
hipError_t launch_dec_init(DecState* st, int* ids, int* unfinished, int B, int max_length, int start_token, int epoch, hipStream_t s) {
    hipLaunchKernelGGL(dec_init_kernel, dim3(1), dim3(64), 0, s, st, ids, unfinished, B, max_length, start_token, epoch);
    return hipGetLastError();
}

__global__ void stream_init_kernel(DecState* st, int* unfinished, int B, int epoch) {
    const int t = threadIdx.x;
    if (t == 0) {
        st->done = 1;            // drained until the first publish
        st->n_unfinished = 0;
        st->step = 0;
        st->seq = 0;
        st->epoch = epoch;
        st->q_head = st->q_tail = 0;
    }
    if (t < MAX_ROWS) {
        st->cur_len[t] = 1;
        st->pos[t] = 0;
        st->self_len[t] = 0;
        st->slot_row[t] = -1;
        st->row_force[t] = -1;
        if (t < B) unfinished[t] = 0;
    }
}
hipError_t launch_stream_init(DecState* st, int* unfinished, int B, int epoch, hipStream_t s) {
    hipLaunchKernelGGL(stream_init_kernel, dim3(1), dim3(64), 0, s, st, unfinished, B, epoch);
    return hipGetLastError();
}

__global__ void set_state_kernel(DecState* st, int cur_len, int pos, int self_len) {
    st->cur_len[0] = cur_len;
    st->pos[0] = pos;
    st->self_len[0] = self_len;
    st->slot_row[0] = 0;
    st->done = 0;
    st->n_unfinished = 1;
    st->step = 0;
    st->seq = 0;
}
hipError_t launch_set_state(DecState* st, int cur_len, int pos, int self_len, hipStream_t s) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, s, st, cur_len, pos, self_len);
    return hipGetLastError();
}

// src [LH][src_rows][64] -> dst [LH][dst_rows][64], first n_rows rows of every (layer, head) slab
__global__ __launch_bounds__(256) void copy_cache_rows_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                              int LH, int src_rows, int dst_rows, int n_rows) {
    const long long per = (long long)n_rows * 16, total = per * LH;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long lh = i / per, r = i - lh * per;
        dst[lh * dst_rows * 16 + r] = src[lh * src_rows * 16 + r];
    }
}
hipError_t launch_copy_cache_rows(const float* src, float* dst, int LH, int src_rows, int dst_rows, int n_rows,
                                  hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const long long total = (long long)LH * n_rows * 16;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(copy_cache_rows_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4*>(src),
                       reinterpret_cast<float4*>(dst), LH, src_rows, dst_rows, n_rows);
    return hipGetLastError();
}

}  // namespace wt
