// Token-level timestamps: the device post-pass of wt_decoder_read_token_timestamps (TokTsParams, wt_common.h).  It restates transformers'
// WhisperForConditionalGeneration._extract_token_timestamps / _median_filter / _dynamic_time_warping (models/whisper/modeling_whisper.py)
// over the queries the cross-attention launches captured (DecAttnParams.qh) and the resident cross-K cache.  Nothing here is built with
// fast-math: the DTW's comparisons and the 0 / 0 of a one-token column are IEEE.
#include "wt_common.h"

#include <math.h>

namespace wt {

__device__ __forceinline__ int tt_tokens(const TokTsParams& p) {
    const int n = p.st ? p.st->cur_len[0] - 1 : p.n_fixed;
    return n < p.n_cap ? n : p.n_cap;
}

// ---- a. softmax rows: W[sel][t][s] = softmax_s(q_hist[sel][b][t] . K[layer][b][head][s]).  Grid (ceil(n_cap / TQ), n_sel): a block carries
// TQ query rows against every key (the head's K is read once per TQ rows, from L2), one key per thread and pass, the scores in LDS.
constexpr int TT_TQ = 4;
template <bool KVH>
__global__ __launch_bounds__(256) void tt_softmax_kernel(const TokTsParams p, const int b) {
    extern __shared__ float tt_sc[];          // [TT_TQ][S] scores, then [TT_TQ][64] queries, then [8] reduction scratch
    const int S = p.S, N = tt_tokens(p);
    const int t0 = blockIdx.x * TT_TQ, sel = blockIdx.y, tid = threadIdx.x;
    if (t0 >= N) return;                      // block-uniform
    float* sq = tt_sc + (size_t)TT_TQ * S;
    float* red = sq + TT_TQ * HEAD_DIM;
    for (int i = tid; i < TT_TQ * HEAD_DIM; i += 256) {
        const int t = min(t0 + i / HEAD_DIM, N - 1);
        sq[i] = p.q_hist[(((size_t)sel * p.qh_rows + b) * p.qh_steps + t) * HEAD_DIM + (i % HEAD_DIM)];
    }
    __syncthreads();
    const size_t krow = (((size_t)p.layer[sel] * p.cross_rows + b) * p.H + p.head[sel]) * S;
    for (int s = tid; s < S; s += 256) {
        float k[HEAD_DIM];
        if constexpr (KVH) {
            const _Float16* kp = reinterpret_cast<const _Float16*>(p.cross_k) + (krow + s) * HEAD_DIM;
#pragma unroll
            for (int i = 0; i < HEAD_DIM; i += 8) {
                typedef _Float16 h8v __attribute__((ext_vector_type(8)));
                const h8v v = *reinterpret_cast<const h8v*>(kp + i);
#pragma unroll
                for (int j = 0; j < 8; ++j) k[i + j] = (float)v[j];
            }
        } else {
            const float* kp = reinterpret_cast<const float*>(p.cross_k) + (krow + s) * HEAD_DIM;
#pragma unroll
            for (int i = 0; i < HEAD_DIM; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(kp + i);
                k[i] = v.x; k[i + 1] = v.y; k[i + 2] = v.z; k[i + 3] = v.w;
            }
        }
#pragma unroll
        for (int q = 0; q < TT_TQ; ++q) {
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < HEAD_DIM; ++i) dot = fmaf(sq[q * HEAD_DIM + i], k[i], dot);
            tt_sc[(size_t)q * S + s] = dot;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int q = 0; q < TT_TQ; ++q) {         // block-uniform trip count; rows past N are skipped as a block
        const int t = t0 + q;
        if (t >= N) break;
        float* row = tt_sc + (size_t)q * S;
        float m = -INFINITY;
        for (int s = tid; s < S; s += 256) m = fmaxf(m, row[s]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float sum = 0.f;
        for (int s = tid; s < S; s += 256) {
            const float e = expf(row[s] - m);
            row[s] = e;
            sum += e;
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) red[4 + wave] = sum;
        __syncthreads();
        sum = (red[4] + red[5]) + (red[6] + red[7]);
        float* out = p.W + ((size_t)sel * p.n_cap + t) * S;
        for (int s = tid; s < S; s += 256) out[s] = row[s] / sum;
        __syncthreads();                      // red[] is reused by the next row
    }
}

// ---- b. statistics over the token axis (std_mean(dim = tokens, unbiased = False)): one thread per (head, frame), two passes
__global__ __launch_bounds__(256) void tt_colstats_kernel(const TokTsParams p) {
    const int S = p.S, N = tt_tokens(p);
    const int s = blockIdx.x * 256 + threadIdx.x, sel = blockIdx.y;
    if (s >= S || N < 1) return;
    const float* w = p.W + (size_t)sel * p.n_cap * S + s;
    float sum = 0.f;
    for (int t = 0; t < N; ++t) sum += w[(size_t)t * S];
    const float mean = sum / (float)N;
    float sq = 0.f;
    for (int t = 0; t < N; ++t) {
        const float d = w[(size_t)t * S] - mean;
        sq = fmaf(d, d, sq);
    }
    p.mean[(size_t)sel * S + s] = mean;
    p.sdev[(size_t)sel * S + s] = sqrtf(sq / (float)N);
}

// ---- c + d. median of WIDTH along the frames (reflect padding) of the normalised rows, then the mean over the heads.  The median is a
// selection by rank in torch.sort's order (NaN last), so no arithmetic touches the values.  One thread per (token, frame).
__device__ __forceinline__ bool tt_less(float a, float b) { return (a == a && b != b) || a < b; }
template <int WIDTH>
__global__ __launch_bounds__(256) void tt_median_mean_kernel(const TokTsParams p, const int b) {
    const int S = p.S, N = tt_tokens(p);
    const int s = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (s >= S || t >= N) return;
    constexpr int PAD = WIDTH / 2;
    int idx[WIDTH];
#pragma unroll
    for (int k = 0; k < WIDTH; ++k) {
        int i = s + k - PAD;
        if (i < 0) i = -i;
        if (i >= S) i = 2 * (S - 1) - i;
        idx[k] = i;                            // (WIDTH > 1 only when S > PAD, so one reflection lands inside)
    }
    float acc = 0.f;
    for (int sel = 0; sel < p.n_sel; ++sel) {
        const float* w = p.W + ((size_t)sel * p.n_cap + t) * S;
        float v[WIDTH];
#pragma unroll
        for (int k = 0; k < WIDTH; ++k) {
            float x = w[idx[k]];
            if (p.mean) x = (x - p.mean[(size_t)sel * S + idx[k]]) / p.sdev[(size_t)sel * S + idx[k]];
            v[k] = x;
        }
        float med = v[0];
        if constexpr (WIDTH > 1) {
#pragma unroll
            for (int i = 0; i < WIDTH; ++i) {
                int rank = 0;
#pragma unroll
                for (int j = 0; j < WIDTH; ++j) rank += (tt_less(v[j], v[i]) || (!tt_less(v[i], v[j]) && j < i)) ? 1 : 0;
                if (rank == PAD) med = v[i];
            }
        }
        acc += med;
    }
    p.matrix[((size_t)b * p.n_cap + t) * S + s] = acc / (float)p.n_sel;
}

// ---- e + f. DTW, one workgroup per utterance, one thread per token row, a wavefront over the anti-diagonals k = i + j: thread r (row
// i = r + 1) keeps cost[i][j - 1] in a register and reads cost[i - 1][j] and cost[i - 1][j - 1] from its neighbour's entries of the last
// two diagonals in LDS (three rotating diagonals, one barrier per diagonal).  The predecessor codes go to device memory as bytes, four
// columns of a row per 32-bit store; thread 0 walks them back from (N, S).
__global__ __launch_bounds__(TT_MAX_TOKENS) void tt_dtw_kernel(const TokTsParams p) {
    __shared__ float diag[3][TT_MAX_TOKENS + 1];
    const int b = blockIdx.x, tid = threadIdx.x, S = p.S, N = tt_tokens(p);
    float* out = p.out + (size_t)b * p.out_ld;
    for (int i = tid; i < p.out_ld; i += blockDim.x) out[i] = 0.f;
    if (N < 1 || S < 1) {
        if (tid == 0 && p.path_len) p.path_len[b] = 0;
        return;                               // block-uniform
    }
    for (int i = tid; i < 3 * (TT_MAX_TOKENS + 1); i += blockDim.x) (&diag[0][0])[i] = INFINITY;
    __syncthreads();
    if (tid == 0) diag[0][0] = 0.f;           // cost[0][0]
    __syncthreads();
    const int i = tid + 1;                    // this thread's row of the cost matrix
    const bool row = i <= N;
    const float* m = p.matrix + ((size_t)b * p.n_cap + (row ? i - 1 : 0)) * S;
    uint32_t* tr = reinterpret_cast<uint32_t*>(p.trace + ((size_t)b * p.n_cap + (row ? i - 1 : 0)) * p.trace_ld);
    float mine = INFINITY;                    // cost[i][j - 1]; cost[i][0] = inf
    uint32_t pack = 0;
    float m_next = 0.f;
    if (row && 2 - i >= 1 && 2 - i <= S) m_next = m[2 - i - 1];
    for (int k = 2; k <= N + S; ++k) {
        const int j = k - i;
        const bool active = row && j >= 1 && j <= S;
        const float mv = m_next;
        const int jn = j + 1;                 // the next diagonal's matrix entry is requested before this one's barrier
        if (row && jn >= 1 && jn <= S) m_next = m[jn - 1];
        float* cur = diag[k % 3];
        if (tid == 0) cur[0] = INFINITY;      // cost[0][k], k >= 1
        if (active) {
            const float c0 = diag[(k + 1) % 3][i - 1];   // diagonal k - 2: cost[i - 1][j - 1]
            const float c1 = diag[(k + 2) % 3][i - 1];   // diagonal k - 1: cost[i - 1][j]
            const float c2 = mine;
            float c;
            uint32_t t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
            else { c = c2; t = 2; }
            mine = (float)((double)(-mv) + (double)c);
            cur[i] = mine;
            pack |= t << (8 * (j & 3));
            if ((j & 3) == 3 || j == S) {
                tr[j >> 2] = pack;
                pack = 0;
            }
        } else if (row && j < 1) {
            cur[i] = INFINITY;                // cost[i][0] and the cells left of it
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    if (tid != 0) return;
    // backtrace (trace[0][:] = 2, trace[:][0] = 1): the entries come out last-first; out[1 + text] keeps the LAST one written for a text
    // index, which is the first of that index along the path -- the reference's `jumps`
    const uint8_t* tb = p.trace + (size_t)b * p.n_cap * p.trace_ld;
    int* path_t = p.path ? p.path + (size_t)b * 2 * (p.n_cap + S) : nullptr;
    int* path_s = path_t ? path_t + (p.n_cap + S) : nullptr;
    int bi = N, bj = S, n = 0;
    while (bi > 0 || bj > 0) {
        if (path_t) { path_t[n] = bi - 1; path_s[n] = bj - 1; }
        ++n;
        if (bi >= 1 && bi < p.out_ld) out[bi] = (float)((double)(bj - 1) * p.time_precision);
        const int t = bi == 0 ? 2 : bj == 0 ? 1 : tb[(size_t)(bi - 1) * p.trace_ld + bj];
        if (t == 0) { --bi; --bj; }
        else if (t == 1) --bi;
        else --bj;
    }
    if (p.path_len) p.path_len[b] = n;
}

static bool tt_params_ok(const TokTsParams& p) {
    return p.S >= 1 && p.n_cap >= 1 && p.n_cap <= TT_MAX_TOKENS && p.width >= 1 && p.width <= TT_MAX_WIDTH && (p.width & 1) &&
           p.n_sel >= 1 && p.n_sel <= TT_MAX_HEADS;
}

hipError_t launch_tt_median(const TokTsParams& p, int b, hipStream_t s) {
    if (!tt_params_ok(p)) return hipErrorInvalidValue;
    const dim3 grid((p.S + 255) / 256, p.n_cap);
    const int w = p.S <= p.width / 2 ? 1 : p.width;   // _median_filter returns its input when the row is no longer than the padding
    switch (w) {
    case 1: hipLaunchKernelGGL(tt_median_mean_kernel<1>, grid, dim3(256), 0, s, p, b); break;
    case 3: hipLaunchKernelGGL(tt_median_mean_kernel<3>, grid, dim3(256), 0, s, p, b); break;
    case 5: hipLaunchKernelGGL(tt_median_mean_kernel<5>, grid, dim3(256), 0, s, p, b); break;
    case 7: hipLaunchKernelGGL(tt_median_mean_kernel<7>, grid, dim3(256), 0, s, p, b); break;
    case 9: hipLaunchKernelGGL(tt_median_mean_kernel<9>, grid, dim3(256), 0, s, p, b); break;
    case 11: hipLaunchKernelGGL(tt_median_mean_kernel<11>, grid, dim3(256), 0, s, p, b); break;
    case 13: hipLaunchKernelGGL(tt_median_mean_kernel<13>, grid, dim3(256), 0, s, p, b); break;
    case 15: hipLaunchKernelGGL(tt_median_mean_kernel<15>, grid, dim3(256), 0, s, p, b); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tt_matrix(const TokTsParams& p, int b, hipStream_t s) {
    if (!tt_params_ok(p) || !p.mean || !p.sdev) return hipErrorInvalidValue;
    const size_t lds = ((size_t)TT_TQ * p.S + TT_TQ * HEAD_DIM + 8) * 4;
    if (lds > 64 * 1024) return hipErrorInvalidValue;   // S <= 4000 frames
    const dim3 grid((p.n_cap + TT_TQ - 1) / TT_TQ, p.n_sel);
    if (p.kv_half) hipLaunchKernelGGL(tt_softmax_kernel<true>, grid, dim3(256), lds, s, p, b);
    else hipLaunchKernelGGL(tt_softmax_kernel<false>, grid, dim3(256), lds, s, p, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tt_colstats_kernel, dim3((p.S + 255) / 256, p.n_sel), dim3(256), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_tt_median(p, b, s);
}

hipError_t launch_tt_dtw(const TokTsParams& p, hipStream_t s) {
    if (!tt_params_ok(p) || p.B < 1 || p.trace_ld < p.S + 1 || (p.trace_ld & 3) || p.out_ld < 1) return hipErrorInvalidValue;
    const int threads = (p.n_cap + 63) / 64 * 64;
    hipLaunchKernelGGL(tt_dtw_kernel, dim3(p.B), dim3(threads), 0, s, p);
    return hipGetLastError();
}

}  // namespace wt
