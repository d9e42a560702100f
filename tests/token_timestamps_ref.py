"""float64 / numpy restatement of the token-level timestamp post-pass (include/whisper_trtllm_amd.h (9d)): softmax rows of the alignment
heads, normalisation over the tokens, median filter along the frames, mean over the heads, dynamic time warping and the jump times --
what transformers' _extract_token_timestamps / _median_filter / _dynamic_time_warping compute.  A helper of the tests (not a test module,
not the oracle): the CPU tests hold it against the reference-recorded goldens, the GPU tests hold the kernels against it."""
import numpy as np


def softmax_rows(q, k):
    """q [N][64], k [S][64] -> float64 softmax over the frames of q k^T, [N][S]."""
    s = np.asarray(q, np.float64) @ np.asarray(k, np.float64).T
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def normalize_tokens(w):
    """(w - mean) / std over the token axis (-2), population std; a single token gives 0 / 0 = NaN, as torch does."""
    w = np.asarray(w)
    mean = w.mean(-2, keepdims=True)
    std = np.sqrt(((w - mean) ** 2).mean(-2, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (w - mean) / std


def median_filter(x, width):
    """Median of odd `width` along the last axis with reflect padding; the input itself when the axis is no longer than width // 2.  NaN
    sorts last (torch.sort's and numpy's order)."""
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    x = np.asarray(x)
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def matrix_from_weights(w, width, dtype=np.float64):
    """w [heads][N][S] softmax rows -> matrix [N][S]: normalise over the tokens, median along the frames, mean over the heads."""
    w = np.asarray(w, dtype)
    return median_filter(normalize_tokens(w), width).mean(0)


def matrix_from_queries(q, k, width):
    """q [heads][N][64], k [heads][S][64] -> (float64 matrix [N][S], softmax rows [heads][N][S])."""
    w = np.stack([softmax_rows(q[i], k[i]) for i in range(len(q))])
    return matrix_from_weights(w, width), w


def matrix_from_queries_fp32(q, k, width):
    """The same formula in the reference's arithmetic -- float32 torch on the CPU: bmm scores, softmax, std_mean over the tokens, the
    reflect-padded unfold + sort median, the mean over the heads.  Its distance from the float64 evaluation is the fp32 noise of the
    formula on these inputs (after the 1 / std amplification), the yardstick of the matrix bars where no reference run exists."""
    import torch
    q, k = torch.from_numpy(np.asarray(q, np.float32)), torch.from_numpy(np.asarray(k, np.float32))
    w = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)[None]            # [1][heads][N][S]
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    w = (w - mean) / std
    pad = width // 2
    if w.shape[-1] > pad and width > 1:
        w = torch.nn.functional.pad(w, (pad, pad, 0, 0), mode="reflect").unfold(-1, width, 1).sort()[0][..., pad]
    return w.mean(dim=1)[0].numpy()


def dtw(matrix):
    """_dynamic_time_warping on -matrix: fp32 cost, each cell (float)((double)(-m) + (double)c), predecessor 0 if c0 < c1 and c0 < c2, else 1
    if c1 < c0 and c1 < c2, else 2 (IEEE comparisons: NaN and equal costs fall through to 2); borders trace[0][:] = 2, trace[:][0] = 1;
    backtrace from (N, S).  Returns (text_indices, time_indices) in path order."""
    m = -np.asarray(matrix, np.float32).astype(np.float64)
    N, S = m.shape
    cost = np.full((N + 1, S + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, S + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    # anti-diagonals: every cell of one depends on the two before it only, so a diagonal is one vector operation
    for d in range(2, N + S + 1):
        i = np.arange(max(1, d - S), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        with np.errstate(invalid="ignore"):
            t0 = (c0 < c1) & (c0 < c2)
            t1 = ~t0 & (c1 < c0) & (c1 < c2)
        c = np.where(t0, c0, np.where(t1, c1, c2))
        with np.errstate(invalid="ignore"):
            cost[i, j] = (m[i - 1, j - 1] + c.astype(np.float64)).astype(np.float32)
        trace[i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, S
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64)


def token_timestamps(matrix, time_precision=0.02):
    """float32 [N + 1]: 0, then time_precision x the frame at which the DTW path reaches each token (the reference's jumps / jump_times).
    Returns (timestamps, text_indices, time_indices)."""
    text, time = dtw(matrix)
    out = np.zeros(np.asarray(matrix).shape[0] + 1, dtype=np.float32)
    if len(text):
        jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
        out[1:] = (time[jumps] * time_precision).astype(np.float32)
    return out, text, time


def decoder_queries_f64(weights, cfg, ids, enc_out, heads):
    """float64 restatement of the decoder's cross-attention queries and keys (HF WhisperDecoderLayer order, pre-LayerNorm, q scaled by
    head_dim ** -0.5): the decoder is run teacher-forced over the inputs ids[:, :-1] (pad inputs of finished rows included) with a causal
    mask, which equals the step-by-step decode.  weights: the numpy state dict, enc_out [B][S][d].
    Returns (q [heads][B][N][64], k [heads][B][S][64])."""
    import torch
    import torch.nn.functional as F
    W = {n: torch.from_numpy(np.asarray(v)).double() for n, v in weights.items()}
    D, H, L = cfg["d_model"], cfg["decoder_attention_heads"], cfg["decoder_layers"]
    dh = D // H
    inp = torch.from_numpy(np.asarray(ids)[:, :-1]).long()
    enc = torch.from_numpy(np.asarray(enc_out)).double()
    B, N = inp.shape
    sh = lambda t: t.view(B, -1, H, dh).transpose(1, 2)
    mask = torch.full((N, N), float("-inf"), dtype=torch.float64).triu(1)
    h = F.embedding(inp, W["model.decoder.embed_tokens.weight"]) + W["model.decoder.embed_positions.weight"][:N]
    qs, ks = {}, {}

    def attend(x, kv, p, m):
        q = sh(F.linear(x, W[p + "q_proj.weight"], W[p + "q_proj.bias"]) * dh ** -0.5)
        k = sh(F.linear(kv, W[p + "k_proj.weight"]))
        v = sh(F.linear(kv, W[p + "v_proj.weight"], W[p + "v_proj.bias"]))
        s = q @ k.transpose(-1, -2)
        if m is not None:
            s = s + m
        ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, -1, D)
        return F.linear(ctx, W[p + "out_proj.weight"], W[p + "out_proj.bias"]), q, k

    for i in range(L):
        p = f"model.decoder.layers.{i}."
        x = F.layer_norm(h, (D,), W[p + "self_attn_layer_norm.weight"], W[p + "self_attn_layer_norm.bias"], 1e-5)
        h = h + attend(x, x, p + "self_attn.", mask)[0]
        x = F.layer_norm(h, (D,), W[p + "encoder_attn_layer_norm.weight"], W[p + "encoder_attn_layer_norm.bias"], 1e-5)
        a, q, k = attend(x, enc, p + "encoder_attn.", None)
        qs[i], ks[i] = q.numpy(), k.numpy()
        h = h + a
        x = F.layer_norm(h, (D,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], 1e-5)
        h = h + F.linear(F.gelu(F.linear(x, W[p + "fc1.weight"], W[p + "fc1.bias"])), W[p + "fc2.weight"], W[p + "fc2.bias"])
    return (np.stack([qs[l][:, hd] for l, hd in heads]), np.stack([ks[l][:, hd] for l, hd in heads]))


def apply_overrides(weights, overrides):
    """The golden generator's weight overrides: {"q_scale": s} multiplies the cross-attention q_proj weight and bias of every layer by s
    (sharper alignment heads on random weights).  Returns a new dict."""
    out = dict(weights)
    s = float(overrides.get("q_scale", 1.0))
    if s != 1.0:
        for n in list(out):
            if ".encoder_attn.q_proj." in n:
                out[n] = (np.asarray(out[n]) * np.float32(s)).astype(np.float32)
    return out
