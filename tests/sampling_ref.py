"""CPU reference of the temperature sampler (DESIGN.md "Temperature sampling"; include/whisper_trtllm_amd.h (9f)): Philox-4x32-10 in
numpy, the Gumbel noise and the key of a vocabulary id, one step in fp64, and a whole decode that drives oracle/cpu_ref.py's decoder from
outside.  Shared by tests/test_sampling_host.py, tests/test_gpu_sampling.py and tests/golden/make_golden_sampling.py.

  x   = Philox4x32-10(counter = (v >> 2, t, 0, 0), key = (seed & 0xffffffff, seed >> 32))[v & 3]
  u   = ((x >> 9) + 0.5) * 2^-23        exact in fp32, strictly inside (0, 1)
  g   = -log(-log(u))
  key = s[v] / T + g                    token = NaN-aware argmax, lowest index among equals
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two ints.  Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        n0 = ((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK
        n2 = ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK
        c = [n0, p1 & MASK, n2, p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def draws(seed, t, V):
    """The 32-bit draw of every vocabulary id 0 .. V-1 for a row with `seed` writing sequence position t."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    n4 = (V + 3) // 4
    out = philox4x32_10((np.arange(n4), np.full(n4, t), np.zeros(n4), np.zeros(n4)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, 1).reshape(-1)[:V]


def uniform_of(x):
    """u of a 32-bit draw, computed in fp32 as the device does."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel(seed, t, V, dtype=np.float64):
    """Standard Gumbel noise per id: fp64 logs of the exact u (dtype float64), or fp32 logs as the device computes them (float32)."""
    u = uniform_of(draws(seed, t, V)).astype(dtype)
    return -np.log(-np.log(u))


def keys(s, T, seed, t, dtype=np.float64):
    """key[v] = s[v] / T + g[v] in `dtype` (float32: the device's arithmetic, IEEE division then one addition)."""
    s = np.asarray(s, dtype=dtype)
    with np.errstate(invalid="ignore"):
        return (s / dtype(T) + gumbel(seed, t, s.shape[-1], dtype)).astype(dtype)


def nan_argmax(k):
    """torch.argmax's rule: the first NaN if there is one, else the first maximum."""
    k = np.asarray(k)
    return int(np.argmax(np.isnan(k))) if np.isnan(k).any() else int(np.argmax(k))


def sample_step(s, T, seed, t):
    """One step in fp64 over the PROCESSED scores s [V]: (token, log-probability under the untempered scores, winning key, top-2 gap of
    the key -- inf with fewer than two finite keys)."""
    s = np.asarray(s, dtype=np.float64)
    k = keys(s, T, seed, t)
    tok = nan_argmax(k)
    fin = s[s > -np.inf]
    if fin.size == 0 or np.isnan(s).any():
        lp = np.nan
    else:
        m = fin.max()
        lp = s[tok] - (m + np.log(np.exp(fin - m).sum()))
    live = np.sort(k[np.isfinite(k)])
    gap = float(live[-1] - live[-2]) if live.size >= 2 else np.inf
    return tok, lp, k[tok], gap


def sample_decode(cfg, weights, mel, T, seeds, timestamp_mode=False, max_length=None):
    """A whole sampled decode on the CPU: cpu_ref's encoder and decoder_forward, the processors (cpu_ref.apply_logits_processors, or in
    timestamp mode the package's restated WhisperTimeStampLogitsProcessor list), then the fp32 key as the device computes it.
    Returns (ids int64 [B, len], token_logprobs float64 [B, len] -- log_softmax of the processed scores in fp64 at the chosen id, 0 at
    position 0 and behind a row's EOS)."""
    import cpu_ref
    import torch
    from whisper_trtllm_amd import generation
    W = cpu_ref.to_torch(weights)
    B = mel.shape[0]
    max_length = cfg["max_length"] if max_length is None else max_length
    eos, pad = cfg["eos_token_id"], cfg["pad_token_id"]
    procs = generation.get_logits_processor(dict(cfg, max_length=max_length), 1, return_timestamps=True) if timestamp_mode else None
    with torch.no_grad():
        enc = cpu_ref.encoder_forward(W, cfg, torch.from_numpy(mel))
        ids = torch.full((B, 1), cfg["decoder_start_token_id"], dtype=torch.long)
        unfinished = np.ones(B, dtype=bool)
        lps = [np.zeros(B)]
        past = None
        while True:
            logits, past = cpu_ref.decoder_forward(W, cfg, ids[:, -1:], enc, past)
            t = ids.shape[1]
            raw = logits[:, -1, :]
            s = procs(ids, raw.clone()) if timestamp_mode else cpu_ref.apply_logits_processors(cfg, t, 1, raw)
            s = s.numpy()
            nxt, lp = np.zeros(B, dtype=np.int64), np.zeros(B)
            for b in range(B):
                nxt[b] = nan_argmax(keys(s[b], T, seeds[b], t, np.float32))
                if unfinished[b]:
                    sd = s[b].astype(np.float64)
                    fin = sd[sd > -np.inf]
                    lp[b] = sd[nxt[b]] - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))
                else:
                    nxt[b] = pad
            lps.append(lp)
            ids = torch.cat([ids, torch.from_numpy(nxt)[:, None]], dim=-1)
            unfinished &= nxt != eos
            if not unfinished.any() or ids.shape[1] >= max_length:
                break
    return ids.numpy(), np.stack(lps, 1)
