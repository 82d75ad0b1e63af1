"""T5 encoder (v1.1, gated GELU) on the HIP kernels: FLUX's `text_encoder_2`, the T5-XXL behind `pipe.encode_prompt` in the
reference's fastvideo/data_preprocess/preprocess_flux_embedding.py:89 (diffusers' FluxPipeline._get_t5_prompt_embeds).
Inference only.

Layout, as clip_vision.py: all prompts of a call are one batch of M = B S token rows, bf16; every Linear (none has a bias) is a
launch of the persistent GEMM (`ops.gemm(..., stream_k=False)`: a prompt's rows do not depend on how many prompts share the
call), q | k | v and wi_0 | wi_1 each as one fused GEMM, residual sums in the `o` and `wo` GEMMs' epilogue with a ones gate.
csrc/text.hip holds the rest: the embedding gather, T5LayerNorm (`mgx_rms_norm_affine`) and the gated tanh GELU; the attention
takes the relative-position bias as a compact [H, 2 S - 1] table (`mgx_text_attn_fwd`, csrc/encoder_attn.hip; the bias depends on
(head, k - q) only).  The layer is encoder_host.py's pre-norm walk, with T5's norm, attention, activation and Linear names.

No attention mask: FLUX's `encode_prompt` passes none to T5, so the padding tokens of a prompt are attended like any other.
`encode` has no `attention_mask` argument that works: giving one raises.

Stated deviation: transformers' T5LayerNorm under bf16 rounds twice (after the normalisation and after the weight),
`mgx_rms_norm_affine` rounds once.

Key names are transformers' `T5EncoderModel` names, pinned against it by tests/test_text_refs.py."""
import math
from dataclasses import dataclass, replace

import torch

from . import ops
from .encoder_host import EncoderHost, convert_names, draw_state_dict, read_checkpoint_dir
from .ops import BF16, F32


@dataclass
class T5EncoderConfig:
    vocab: int = 32128
    d_model: int = 4096
    layers: int = 24
    heads: int = 64
    d_kv: int = 64
    d_ff: int = 10240
    num_buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6

    @property
    def inner(self):
        return self.heads * self.d_kv

    def check(self):
        if self.d_kv % 16 or not 16 <= self.d_kv <= 128:
            raise ValueError(f"d_kv {self.d_kv}: the attention kernel takes multiples of 16 up to 128")
        if self.d_model % 64 or self.d_model > 4096 or self.d_ff % 64 or self.inner % 64:
            raise ValueError("d_model (<= 4096), d_ff and heads * d_kv must be multiples of 64")
        if self.num_buckets % 2 or self.num_buckets < 4 or self.max_distance <= self.num_buckets // 4 or self.vocab < 1:
            raise ValueError("num_buckets must be even and >= 4, max_distance above num_buckets / 4")
        return self


T5_XXL = T5EncoderConfig()
PRESETS = {"T5_XXL": T5_XXL}


# ------------------------------------------------------------------------------------------------------- relative positions
def relative_position_bucket(delta, num_buckets=32, max_distance=128):
    """transformers' T5Attention._relative_position_bucket(bidirectional=True) of delta = key - query (an int64 tensor), with
    the same torch operations, its float32 `log` included."""
    nb = num_buckets // 2
    buckets = (delta > 0).to(torch.long) * nb
    rp = delta.abs()
    max_exact = nb // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rp, large)


def t5_relative_bias_table(weight, S, num_buckets=32, max_distance=128):
    """weight [num_buckets, H] (block 0's relative_attention_bias.weight) -> [H, 2 S - 1] fp32 on the weight's device:
    table[h][k - q + S - 1] = weight[bucket(k - q)][h], the whole of T5Attention.compute_bias for S queries and S keys."""
    delta = torch.arange(-(S - 1), S, dtype=torch.long, device=weight.device)
    return weight.float()[relative_position_bucket(delta, num_buckets, max_distance)].t().contiguous()


# ------------------------------------------------------------------------------------------------------------- key formats
def param_shapes(c):
    """name -> shape of the internal layout."""
    s = {"tok": (c.vocab, c.d_model), "rel_bias": (c.num_buckets, c.heads), "ln_final.weight": (c.d_model,)}
    for i in range(c.layers):
        L = f"layers.{i}."
        s[L + "ln_1.weight"] = s[L + "ln_2.weight"] = (c.d_model,)
        s[L + "qkv.weight"] = (3 * c.inner, c.d_model)
        s[L + "o.weight"] = (c.d_model, c.inner)
        s[L + "wi.weight"] = (2 * c.d_ff, c.d_model)
        s[L + "wo.weight"] = (c.d_model, c.d_ff)
    return s


def _hf_names(c):
    """internal name -> transformers' T5EncoderModel name, a tuple of names to concatenate along dim 0, or -- for the token
    table -- a list of alternatives (the tied `shared.weight` / `encoder.embed_tokens.weight`)"""
    e = "encoder."
    m = {"tok": ["shared.weight", e + "embed_tokens.weight"],
         "rel_bias": e + "block.0.layer.0.SelfAttention.relative_attention_bias.weight", "ln_final.weight": e + "final_layer_norm.weight"}
    for i in range(c.layers):
        L, B = f"layers.{i}.", e + f"block.{i}.layer."
        m[L + "ln_1.weight"], m[L + "ln_2.weight"] = B + "0.layer_norm.weight", B + "1.layer_norm.weight"
        m[L + "qkv.weight"] = tuple(B + f"0.SelfAttention.{n}.weight" for n in "qkv")
        m[L + "o.weight"] = B + "0.SelfAttention.o.weight"
        m[L + "wi.weight"] = tuple(B + f"1.DenseReluDense.{n}.weight" for n in ("wi_0", "wi_1"))
        m[L + "wo.weight"] = B + "1.DenseReluDense.wo.weight"
    return m


def convert_state_dict(sd, config):
    """A T5EncoderModel state dict -> the internal dict.  q | k | v and wi_0 | wi_1 are fused along dim 0.  Missing, unknown
    (`shared.` / `encoder.` keys the layout does not know) and wrongly shaped tensors raise a ValueError that names them; keys
    of other networks are ignored."""
    return convert_names(sd, _hf_names(config), param_shapes(config), ("shared.", "encoder."), "T5 encoder")


def config_from_json(raw):
    """`config.json` of a transformers T5EncoderModel, or `{"preset": "T5_XXL", ...overrides}`.  Only the gated GELU of T5 v1.1
    is built."""
    if "preset" in raw:
        return replace(PRESETS[raw["preset"]], **{k: v for k, v in raw.items() if k in T5EncoderConfig.__dataclass_fields__})
    ff = raw.get("feed_forward_proj", "relu")
    if ff != "gated-gelu":
        raise ValueError(f"feed_forward_proj {ff!r}: only T5 v1.1's \"gated-gelu\" is supported")
    return T5EncoderConfig(vocab=raw["vocab_size"], d_model=raw["d_model"], layers=raw["num_layers"], heads=raw["num_heads"],
                           d_kv=raw["d_kv"], d_ff=raw["d_ff"], num_buckets=raw.get("relative_attention_num_buckets", 32),
                           max_distance=raw.get("relative_attention_max_distance", 128), eps=raw.get("layer_norm_epsilon", 1e-6))


class T5Encoder(EncoderHost):
    def __init__(self, config: T5EncoderConfig = None, device="cuda"):
        self.config = (config or T5_XXL).check()
        super().__init__(device, self.config.d_model)
        self._tables = {}

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, path, device="cuda"):
        """A directory with `config.json` (see `config_from_json`) and one or more `*.safetensors` files."""
        raw, sd = read_checkpoint_dir(path)
        return cls(config_from_json(raw), device=device).load_state_dict(sd)

    def load_state_dict(self, sd):
        """Matrices and the token table go to bf16 on the device, the norm weights to fp32 there; the relative-attention weight
        stays on the host in fp32 (the bias table is built there, once per sequence length)."""
        t = convert_state_dict(sd, self.config)
        rel_bias = t.pop("rel_bias")
        self.P, self._tables = self._place(t), {}
        self.P["rel_bias"] = rel_bias.detach().to("cpu", F32).contiguous()
        return self

    def init_synthetic(self, seed=0):
        """Random weights of the configured architecture drawn on the encoder's device, every value a bf16 number."""
        return self.load_state_dict(synthetic_state_dict(self.config, seed, self.device))

    def bias_table(self, S):
        """[H, 2 S - 1] fp32 on the device: from block 0's weight, for every layer; built on the host once per S"""
        t = self._tables.get(S)
        if t is None:
            c = self.config
            t = self._tables[S] = t5_relative_bias_table(self.P["rel_bias"], S, c.num_buckets, c.max_distance).to(self.device)
        return t

    # ---------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def encode(self, input_ids, attention_mask=None):
        """token ids [B, S] -> `last_hidden_state` [B, S, d_model] bf16, a fresh tensor.  `attention_mask` is not supported and
        raises: FLUX's `encode_prompt` passes none to T5, so padding tokens are attended."""
        if attention_mask is not None:
            raise NotImplementedError("T5Encoder.encode takes no attention_mask: FLUX's encode_prompt passes none to T5")
        if self.P is None:
            raise RuntimeError("T5 weights not loaded")
        c, P = self.config, self.P
        if input_ids.dim() != 2 or not 1 <= input_ids.shape[1] <= 4096:
            raise ValueError(f"input_ids must be [B, 1 .. 4096], not {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        D, H, d, inner, ff, eps = c.d_model, c.heads, c.d_kv, c.inner, c.d_ff, c.eps
        M = B * S
        x = self._plain("x", M, D)
        ops.token_embed(input_ids, P["tok"], None, x)           # checks the ids on the host first: nothing launched on a bad one
        table = self.bias_table(S)
        n, qkv, o = self._plain("n", M, D), self._plain("qkv", M, 3 * inner), self._plain("o", M, inner)
        h, a = self._plain("h", M, 2 * ff), self._plain("a", M, ff)

        def norm(src, name, dst):                               # T5LayerNorm: no mean, no bias, one rounding
            ops.rms_norm_affine(src, D, P[name + ".weight"], dst, D, M, D, eps)

        def attend(qkv, o):                                     # scale 1: T5 does not scale q.k
            if not ops.text_attn_fwd(qkv, 3 * inner, o, inner, B, H, S, d, 1.0, causal=False, rel_bias=table):
                raise RuntimeError(f"mgx_text_attn_fwd refused {S} tokens")

        def activate(h):                                        # gelu(wi_0 x) * wi_1 x: the two halves of h's rows -> a
            ops.gated_act_rows(h, 2 * ff, h[:, ff:], 2 * ff, a, ff, M, ff, ops.ACT_GELU_TANH)
            return a

        for i in range(c.layers):
            self._prenorm_layer(f"layers.{i}.", x, n, qkv, o, h, norm, attend, activate, ("qkv", "o", "wi", "wo"))
        out = torch.empty(B, S, D, dtype=BF16, device=self.device)
        norm(x, "ln_final", out)
        return out


def synthetic_state_dict(config, seed=0, device="cpu"):
    """A random T5EncoderModel-named state dict of `config`, drawn on `device`, every value a bf16 number held in fp32.  The
    scales keep the residual stream of order 1: T5 has no bias and no mean subtraction to rein it in."""
    def std(name, key, s):
        if name in ("tok", "rel_bias"):
            return 1.0
        if len(s) == 1:
            return None
        if key.endswith("SelfAttention.q.weight"):               # T5 does not scale q.k by d_kv^-0.5: its initialisation does
            return (s[1] * config.d_kv) ** -0.5
        return s[1] ** -0.5
    return draw_state_dict(_hf_names(config), param_shapes(config), std, seed, device)
