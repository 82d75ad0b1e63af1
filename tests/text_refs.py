"""float64 restatements of the text encoders (mixgrpo_amd/clip_text.py, mixgrpo_amd/t5.py, csrc/text.hip), plain torch,
device-agnostic.  tests/test_text_refs.py holds them to transformers' CLIPTextModelWithProjection and T5EncoderModel on the CPU;
tests/test_hip_text.py holds the kernels and the towers to them.

Each tower has a second arm, `emulate_bf16=True`: the same float64 arithmetic with a bf16 rounding at exactly the points where
the HIP path stores bf16 -- the embedding sum, every GEMM output, every LayerNorm / RMS-norm output, the activation (the gated
product for T5), each residual sum and the attention's O.  Its distance from the float64 arm is the error the number format
alone causes; the HIP result may be twice that (a different fp32 summation order inside GEMM and attention)."""
import math

import torch

import clip_refs as R
from clip_refs import bf, one_minus_cos, rel_l2  # noqa: F401  (re-exported for the tests)
from mixgrpo_amd.clip_text import pooled_positions
from mixgrpo_amd.t5 import relative_position_bucket

F64 = torch.float64


# -------------------------------------------------------------------------------------------------------------- attention
def bias_matrix(table, S):
    """table [H, 2 S - 1] -> [H, S, S]: element (h, q, k) = table[h][k - q + S - 1]"""
    pos = torch.arange(S, device=table.device)
    return table.to(F64)[:, pos[None, :] - pos[:, None] + S - 1]


def scores(q, k, scale, causal=False, table=None):
    """[B, H, S, S] float64: scale q k^T + bias, -inf above the diagonal when causal"""
    S = q.shape[-2]
    s = (q.to(F64) @ k.to(F64).transpose(-1, -2)) * scale
    if table is not None:
        s = s + bias_matrix(table, S)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    return s


def attention(q, k, v, scale, causal=False, table=None):
    """[..., S, d] float64"""
    return torch.softmax(scores(q, k, scale, causal, table), -1) @ v.to(F64)


def attention_budget(q, k, v, scale, causal=False, table=None):
    """Per-row budget of the bf16 attention output, the rule of tests/attn_refs.py for O with the mask and the bias inside the
    scores: u (|O_r| + sqrt(sum_d sum_j P_rj^2 V_jd^2)), u = 2^-9."""
    P = torch.softmax(scores(q, k, scale, causal, table), -1)
    O = P @ v.to(F64)
    return 2.0 ** -9 * (O.norm(dim=-1) + ((P ** 2) @ (v.to(F64) ** 2)).sum(-1).sqrt())


# ------------------------------------------------------------------------------------------------- norm and activations
def rms_norm(x, g, eps, hf_variance=False):
    """T5LayerNorm in float64.  `hf_variance`: the mean of squares with transformers' own operations, which are float32 whatever
    the model's dtype (`hidden_states.to(torch.float32).pow(2).mean(-1, keepdim=True)`) -- a float64 T5EncoderModel carries
    that float32 step, about 5e-7 relative at the output, so the comparison with it at 1e-10 has to carry it too; everything
    that is compared with a kernel uses the plain float64 mean."""
    x = x.to(F64)
    var = x.to(torch.float32).pow(2).mean(-1, keepdim=True) if hf_variance else x.pow(2).mean(-1, keepdim=True)
    return x * torch.rsqrt(var + eps) * g.to(F64)


def gelu_tanh(x):
    """transformers' NewGELUActivation (`gelu_new`)"""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def gelu_tanh_stable(x):
    """the same function as x sigmoid(2 u): exact in float64 where 1 + tanh u cancels (x << 0)"""
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3)))


ACT = {"gelu": R.gelu, "quick_gelu": R.quick_gelu, "gelu_tanh": gelu_tanh_stable}


# ----------------------------------------------------------------------------------------------------------------- towers
def clip_text_tower(P, config, input_ids, emulate_bf16=False, device=None):
    """P: the internal layout of clip_text.convert_state_dict; input_ids [B, S] -> (text_embeds [B, embed_dim] not
    normalised -- None without a text_projection --, pooled [B, width]) float64."""
    c = config
    r = bf if emulate_bf16 else (lambda t: t)
    device = device or P["tok"].device
    P = {k: v.to(F64).to(device) for k, v in P.items()}
    ids = input_ids.to(device).long()
    B, S = ids.shape
    w, H, d = c.width, c.heads, c.head_dim
    x = r(P["tok"][ids] + P["pos"][:S])
    for i in range(c.layers):
        L = f"layers.{i}."
        n = r(R.layer_norm(x, P[L + "ln_1.weight"], P[L + "ln_1.bias"], c.layer_norm_eps))
        qkv = r(n @ P[L + "qkv.weight"].t() + P[L + "qkv.bias"])
        q, k, v = (t.view(B, S, H, d).transpose(1, 2) for t in qkv.split(w, -1))
        o = r(attention(q, k, v, d ** -0.5, causal=True).transpose(1, 2).reshape(B, S, w))
        x = r(x + r(o @ P[L + "out.weight"].t() + P[L + "out.bias"]))
        n = r(R.layer_norm(x, P[L + "ln_2.weight"], P[L + "ln_2.bias"], c.layer_norm_eps))
        h = r(n @ P[L + "fc1.weight"].t() + P[L + "fc1.bias"])
        h = r(R.ACT[c.act](h))
        x = r(x + r(h @ P[L + "fc2.weight"].t() + P[L + "fc2.bias"]))
    n = r(R.layer_norm(x, P["ln_final.weight"], P["ln_final.bias"], c.layer_norm_eps))
    pooled = n[torch.arange(B, device=device), pooled_positions(ids, c.eos_token_id).to(device)]
    return (r(pooled @ P["proj.weight"].t()) if "proj.weight" in P else None), pooled


def t5_encoder(P, config, input_ids, emulate_bf16=False, device=None, hf_variance=False):
    """P: the internal layout of t5.convert_state_dict; input_ids [B, S] -> last_hidden_state [B, S, d_model] float64.  The
    bias table is taken in float64 from `relative_position_bucket` (mixgrpo_amd/t5.py), which this pins against transformers.
    `hf_variance`: see `rms_norm`."""
    c = config
    r = bf if emulate_bf16 else (lambda t: t)
    device = device or P["tok"].device
    P = {k: v.to(F64).to(device) for k, v in P.items()}
    ids = input_ids.to(device).long()
    B, S = ids.shape
    H, d, inner, ff = c.heads, c.d_kv, c.inner, c.d_ff
    delta = torch.arange(-(S - 1), S, dtype=torch.long)
    table = P["rel_bias"][relative_position_bucket(delta, c.num_buckets, c.max_distance).to(device)].t()
    x = r(P["tok"][ids])
    for i in range(c.layers):
        L = f"layers.{i}."
        n = r(rms_norm(x, P[L + "ln_1.weight"], c.eps, hf_variance))
        qkv = r(n @ P[L + "qkv.weight"].t())
        q, k, v = (t.view(B, S, H, d).transpose(1, 2) for t in qkv.split(inner, -1))
        o = r(attention(q, k, v, 1.0, table=table).transpose(1, 2).reshape(B, S, inner))
        x = r(x + r(o @ P[L + "o.weight"].t()))
        n = r(rms_norm(x, P[L + "ln_2.weight"], c.eps, hf_variance))
        h = r(n @ P[L + "wi.weight"].t())
        a = r(gelu_tanh(h[..., :ff]) * h[..., ff:])
        x = r(x + r(a @ P[L + "wo.weight"].t()))
    return r(rms_norm(x, P["ln_final.weight"], c.eps, hf_variance))


# ---------------------------------------------------------------------------------------------------------- stub tokenizer
def stub_tokenizer(length, vocab=1000):
    """prompts -> [B, length] int64 (no vocabulary file exists offline): one id per character, then the largest id -- the
    end-of-text token of the legacy pooling rule --, then padding zeros"""
    def tok(prompts):
        ids = torch.zeros(len(prompts), length, dtype=torch.long)
        for i, p in enumerate(prompts):
            v = [3 + ord(ch) % (vocab - 4) for ch in p][:length - 1]
            ids[i, :len(v)] = torch.tensor(v, dtype=torch.long)
            ids[i, len(v)] = vocab - 1
        return ids
    return tok
