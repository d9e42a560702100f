"""Reference of the decoder-prompt prefill: the HF Whisper decoder over all prompt positions at once, with the causal mask, in any dtype.

`prompt_self_kv(weights, cfg, prompt, enc_out, dtype)` runs WhisperDecoder.forward's layers (modeling_whisper.py: pre-LN self attention
with the causal mask of _prepare_decoder_attention_mask, cross attention over the encoder memory, erf-GELU FFN) over prompt [B][n] from
the synthetic weights and returns what the prefill leaves in the self caches: K and V of every layer, [L][B][H][n][64].  It shares no
code with the engine (no folded query, no head caches) and none with the stepping oracle (oracle/cpu_ref.py feeds one position a time
and needs no mask)."""
import torch
import torch.nn.functional as F


def prompt_self_kv(weights, cfg, prompt, enc_out, dtype=torch.float64):
    W = {k: torch.as_tensor(v).to(dtype) for k, v in weights.items() if k.startswith("model.decoder.")}
    D, H, L = cfg["d_model"], cfg["decoder_attention_heads"], cfg["decoder_layers"]
    prompt = torch.as_tensor(prompt, dtype=torch.long)
    B, n = prompt.shape
    enc = enc_out.to(dtype)
    sh = lambda t: t.view(B, -1, H, D // H).transpose(1, 2)
    ln = lambda x, p: F.layer_norm(x, (D,), W[p + ".weight"], W[p + ".bias"], 1e-5)
    mask = torch.full((n, n), float("-inf"), dtype=dtype).triu(1)

    def attend(x, kv, p, m):
        q = sh(F.linear(x, W[p + "q_proj.weight"], W[p + "q_proj.bias"]) * (D // H) ** -0.5)
        k, v = sh(F.linear(kv, W[p + "k_proj.weight"])), sh(F.linear(kv, W[p + "v_proj.weight"], W[p + "v_proj.bias"]))
        s = q @ k.transpose(-1, -2)
        ctx = (torch.softmax(s + m if m is not None else s, -1) @ v).transpose(1, 2).reshape(B, -1, D)
        return F.linear(ctx, W[p + "out_proj.weight"], W[p + "out_proj.bias"]), k, v

    h = F.embedding(prompt, W["model.decoder.embed_tokens.weight"]) + W["model.decoder.embed_positions.weight"][:n]
    ks, vs = [], []
    for i in range(L):
        p = f"model.decoder.layers.{i}."
        a, k, v = attend(ln(h, p + "self_attn_layer_norm"), ln(h, p + "self_attn_layer_norm"), p + "self_attn.", mask)
        ks.append(k)
        vs.append(v)
        h = h + a
        h = h + attend(ln(h, p + "encoder_attn_layer_norm"), enc, p + "encoder_attn.", None)[0]
        x = F.gelu(F.linear(ln(h, p + "final_layer_norm"), W[p + "fc1.weight"], W[p + "fc1.bias"]))
        h = h + F.linear(x, W[p + "fc2.weight"], W[p + "fc2.bias"])
    return torch.stack(ks), torch.stack(vs)
