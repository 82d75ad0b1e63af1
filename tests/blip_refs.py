"""float64 restatements of the ImageReward scorer (mixgrpo_amd/image_reward.py, csrc/blip.hip), plain torch, device-agnostic:
BLIP's ViT, the BERT text encoder with a cross-attention sub-layer in every layer, the MLP head and the whole score.
tests/test_blip_refs.py holds them to transformers' BlipVisionModel and BlipTextModel on the CPU; tests/test_hip_image_reward.py
holds the kernels and the encoders to them.

Both encoders have a second arm, `emulate_bf16=True`, as tests/text_refs.py has: the same float64 arithmetic with a bf16 rounding
at exactly the points where the HIP path stores bf16 -- the patch rows, the embedding sums, every GEMM output, every LayerNorm
output, the activation, each residual sum and the attention's O.  Its distance from the float64 arm is the error the number
format alone causes.  The head runs in fp32 on the device, 2^-16 of a bf16 step: the emulation arm does not round it."""
import torch

import clip_refs as R
from clip_refs import bf, rel_l2  # noqa: F401  (re-exported for the tests)

F64 = torch.float64


# -------------------------------------------------------------------------------------------------------------- attention
def _admitted(kv_len, B, Skv, device):
    """[B, 1, 1, Skv] bool: key t of sample b counts"""
    if kv_len is None:
        return torch.ones(B, 1, 1, Skv, dtype=torch.bool, device=device)
    return (torch.arange(Skv, device=device)[None] < kv_len.to(device)[:, None])[:, None, None, :]


def _probs(q, k, scale, kv_len):
    B, Skv = q.shape[0], k.shape[-2]
    keep = _admitted(kv_len, B, Skv, q.device)
    k = torch.where(keep.transpose(-1, -2), k.to(F64), torch.zeros((), dtype=F64, device=q.device))   # what an excluded row holds
    s = (q.to(F64) @ k.transpose(-1, -2)) * scale                                                       # never matters
    return torch.softmax(s.masked_fill(~keep, float("-inf")), -1), keep


def xattention(q, k, v, scale, kv_len=None):
    """q [B, H, Sq, d], k, v [B, H, Skv, d] -> softmax(scale q k^T over the keys t < kv_len[b]) v, float64.  Excluded keys are
    excluded exactly: whatever their rows of k and v hold, inf and NaN included, does not reach the result."""
    P, keep = _probs(q, k, scale, kv_len)
    return P @ torch.where(keep.transpose(-1, -2), v.to(F64), torch.zeros((), dtype=F64, device=q.device))


def xattention_budget(q, k, v, scale, kv_len=None):
    """Per-row budget of the bf16 attention output, the rule of tests/attn_refs.py for O with the exclusion inside the scores:
    u (|O_r| + sqrt(sum_d sum_j P_rj^2 V_jd^2)), u = 2^-9."""
    P, keep = _probs(q, k, scale, kv_len)
    v = torch.where(keep.transpose(-1, -2), v.to(F64), torch.zeros((), dtype=F64, device=q.device))
    return 2.0 ** -9 * ((P @ v).norm(dim=-1) + ((P ** 2) @ (v ** 2)).sum(-1).sqrt())


# --------------------------------------------------------------------------------------------------------------- encoders
def _f64(P, device):
    return {k: v.to(F64).to(device) for k, v in P.items()}


def vit_encoder(P, config, pixel_values, emulate_bf16=False):
    """P: the internal layout of image_reward.convert_state_dict (`vis.*` is read); pixel_values [B, 3, R, R] -> the final
    LayerNorm of every token, [B, tokens, width] float64.  No pre-LayerNorm, a patch bias, no projection."""
    c = config
    r = bf if emulate_bf16 else (lambda t: t)
    P = _f64({k[4:]: v for k, v in P.items() if k.startswith("vis.")}, pixel_values.device)
    w, S, H, d, eps = c.width, c.tokens, c.heads, c.head_dim, c.layer_norm_eps
    B = pixel_values.shape[0]
    patches = r(R.patchify(pixel_values.to(F64), c.patch_size))
    pe = r(patches @ P["patch.weight"].reshape(w, -1).t() + P["patch.bias"]).view(B, S - 1, w)
    x = r(torch.cat([(P["cls"] + P["pos"][0]).expand(B, 1, w), pe + P["pos"][1:]], 1))
    for i in range(c.layers):
        L = f"layers.{i}."
        n = r(R.layer_norm(x, P[L + "ln_1.weight"], P[L + "ln_1.bias"], eps))
        qkv = r(n @ P[L + "qkv.weight"].t() + P[L + "qkv.bias"])
        q, k, v = (t.view(B, S, H, d).transpose(1, 2) for t in qkv.split(w, -1))
        o = r(R.attention(q, k, v, d ** -0.5).transpose(1, 2).reshape(B, S, w))
        x = r(x + r(o @ P[L + "out.weight"].t() + P[L + "out.bias"]))
        n = r(R.layer_norm(x, P[L + "ln_2.weight"], P[L + "ln_2.bias"], eps))
        h = r(R.gelu(r(n @ P[L + "fc1.weight"].t() + P[L + "fc1.bias"])))
        x = r(x + r(h @ P[L + "fc2.weight"].t() + P[L + "fc2.bias"]))
    return r(R.layer_norm(x, P["ln_post.weight"], P["ln_post.bias"], eps))


def text_encoder(P, config, input_ids, lengths, image_tokens, emulate_bf16=False):
    """P: the internal layout (`txt.*` is read); input_ids [B, S], lengths [B], image_tokens [B, T, encoder_width] -> the last
    layer's hidden states [B, S, width] float64.  Post-LayerNorm BERT; each layer: self-attention over the keys below
    lengths[b], cross-attention over all image tokens, FFN with the exact GELU.  The rows from lengths[b] on are computed like
    any other and mean nothing."""
    c = config
    r = bf if emulate_bf16 else (lambda t: t)
    device = image_tokens.device
    P = _f64({k[4:]: v for k, v in P.items() if k.startswith("txt.")}, device)
    ids = input_ids.to(device).long()
    B, S = ids.shape
    w, H, d, eps = c.width, c.heads, c.head_dim, c.layer_norm_eps
    heads = lambda t: t.reshape(B, -1, H, d).transpose(1, 2)
    ln = lambda t, name: r(R.layer_norm(t, P[name + ".weight"], P[name + ".bias"], eps))
    x = ln(r(P["tok"][ids] + P["pos"][:S]), "ln_emb")
    kv = r(image_tokens.to(F64) @ P["xkv.weight"].t() + P["xkv.bias"])              # [B, T, layers 2 w]: all layers at once
    for i in range(c.layers):
        L = f"layers.{i}."
        qkv = r(x @ P[L + "qkv.weight"].t() + P[L + "qkv.bias"])
        q, k, v = (heads(t) for t in qkv.split(w, -1))
        o = r(xattention(q, k, v, d ** -0.5, lengths).transpose(1, 2).reshape(B, S, w))
        x = ln(r(x + r(o @ P[L + "out.weight"].t() + P[L + "out.bias"])), L + "ln_attn")
        q = heads(r(x @ P[L + "xq.weight"].t() + P[L + "xq.bias"]))
        k, v = heads(kv[..., 2 * w * i:2 * w * i + w]), heads(kv[..., 2 * w * i + w:2 * w * (i + 1)])
        o = r(xattention(q, k, v, d ** -0.5).transpose(1, 2).reshape(B, S, w))
        x = ln(r(x + r(o @ P[L + "xout.weight"].t() + P[L + "xout.bias"])), L + "ln_x")
        h = r(R.gelu(r(x @ P[L + "fc1.weight"].t() + P[L + "fc1.bias"])))
        x = ln(r(x + r(h @ P[L + "fc2.weight"].t() + P[L + "fc2.bias"])), L + "ln_out")
    return x


def head_layers(P, h0):
    """The five Linears one after the other (no activation between them), float64: h0 [B, width] -> [B]"""
    x = h0.to(F64)
    j = 0
    while f"head.{j}.weight" in P:
        x = x @ P[f"head.{j}.weight"].to(F64).to(x.device).t() + P[f"head.{j}.bias"].to(F64).to(x.device)
        j += 1
    return x[:, 0]


def head_composed(P, h0):
    """The same function as ONE affine map: the product of the five matrices, taken first"""
    dev = h0.device
    A = torch.eye(h0.shape[1], dtype=F64, device=dev)
    b = torch.zeros(h0.shape[1], dtype=F64, device=dev)
    j = 0
    while f"head.{j}.weight" in P:
        W, c = P[f"head.{j}.weight"].to(F64).to(dev), P[f"head.{j}.bias"].to(F64).to(dev)
        A, b = W @ A, W @ b + c
        j += 1
    return (h0.to(F64) @ A.t() + b)[:, 0]


def score(P, vision_config, text_config, pixel_values, input_ids, lengths, mean, std, emulate_bf16=False):
    """(scores [B], hidden [B, S, width], image tokens [B, T, width]) float64"""
    tokens = vit_encoder(P, vision_config, pixel_values, emulate_bf16)
    hidden = text_encoder(P, text_config, input_ids, lengths, tokens, emulate_bf16)
    return (head_layers(P, hidden[:, 0]) - mean) / std, hidden, tokens


# ---------------------------------------------------------------------------------------------------------- stub tokenizer
def stub_tokenizer(length=35, vocab=1000):
    """prompts -> (ids [n, length] int64, lengths [n] int64), no vocabulary file exists offline: id 1 (a [CLS]) first, then one
    id per character, truncated to `length`, padded with zeros.  An empty prompt has length 1."""
    def tok(prompts):
        ids = torch.zeros(len(prompts), length, dtype=torch.long)
        lens = torch.zeros(len(prompts), dtype=torch.long)
        for i, p in enumerate(prompts):
            v = ([1] + [3 + ord(ch) % (vocab - 3) for ch in p])[:length]
            ids[i, :len(v)] = torch.tensor(v, dtype=torch.long)
            lens[i] = len(v)
        return ids, lens
    return tok
