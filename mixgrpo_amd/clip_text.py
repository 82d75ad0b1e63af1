"""CLIP text tower on the HIP kernels: the text half of the reference's three usual rewards,
    HPSClipRewardModel (fastvideo/models/reward_model/hps_score.py:69-72: the tokenized prompt goes through open_clip's text tower
    inside `self.reward_model(image, text)`), PickScoreRewardModel (pick_score.py:64-77: `get_text_features`) and
    CLIPScoreRewardModel (clip_score.py: `encode_text`),
and the CLIP-L text model whose `pooler_output` FLUX's `encode_prompt` takes
(fastvideo/data_preprocess/preprocess_flux_embedding.py:89).  Inference only.

Layout, as clip_vision.py: all prompts of a call are one batch of M = B S token rows, bf16; every Linear is a launch of the
persistent GEMM (`ops.gemm(..., stream_k=False)`, so that a prompt's rows do not depend on how many prompts share the call),
residual sums ride the GEMM epilogue with a ones gate (encoder_host.py: the host scaffold shared with the other encoders);
csrc/text.hip holds the token + position embedding, csrc/encoder_attn.hip the causal attention that reads the packed q | k | v
projection, csrc/clip.hip LayerNorm and the exact / quick GELU.  EOS pooling needs
no kernel: the positions are known on the host, the final LayerNorm runs on all rows and `index_select` picks the pooled ones.

Weights: HF `CLIPModel` / `CLIPTextModelWithProjection` / `CLIPTextModel` key names (pinned against transformers by
tests/test_text_refs.py) or open_clip's names (recollected: the library is absent offline, PARITY UNPINNED), both converted to
one internal layout with the fused q | k | v weight [3 width, width] (`convert_state_dict`).  The tokenizer is not part of this
module: every entry point takes token ids (text_encoders.load_tokenizer delegates tokenising to transformers)."""
from dataclasses import dataclass, replace

import torch

from . import ops
from .encoder_host import EncoderHost, convert_names, draw_state_dict, layer_norm_net_std, read_checkpoint_dir
from .ops import F32

ACTS = {"gelu": ops.ACT_GELU, "quick_gelu": ops.ACT_QUICK_GELU}


@dataclass
class ClipTextConfig:
    vocab: int = 49408
    context: int = 77
    width: int = 768
    layers: int = 12
    heads: int = 12
    mlp_width: int = 3072
    embed_dim: int = 768
    act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    eos_token_id: int = 2                   # transformers' legacy value (what FLUX's text_encoder ships): pool at argmax(ids)

    @property
    def head_dim(self):
        return self.width // self.heads

    def check(self):
        d = self.head_dim
        if self.width % self.heads or d % 16 or d > 128:
            raise ValueError(f"head dim {self.width}/{self.heads}: the attention kernel takes multiples of 16 up to 128")
        if self.width % 64 or self.width > 2048 or self.mlp_width % 64 or self.embed_dim % 4:
            raise ValueError("width and mlp_width must be multiples of 64 (width <= 2048), embed_dim a multiple of 4")
        if not 1 <= self.context <= 4096 or self.vocab < 1:
            raise ValueError("context must be 1 .. 4096 tokens and the vocabulary non-empty")
        if self.act not in ACTS:
            raise ValueError(f"act must be one of {sorted(ACTS)}, not {self.act!r}")
        return self


CLIP_L_TEXT = ClipTextConfig()
VIT_H_14_TEXT = ClipTextConfig(width=1024, layers=24, heads=16, mlp_width=4096, embed_dim=1024, act="gelu")
PRESETS = {"CLIP_L_TEXT": CLIP_L_TEXT, "VIT_H_14_TEXT": VIT_H_14_TEXT}
OPTIONAL = ("proj.weight",)                 # a bare CLIPTextModel (FLUX's text_encoder) has no text_projection


# ------------------------------------------------------------------------------------------------------------- key formats
def param_shapes(c):
    """name -> shape of the internal layout."""
    w = c.width
    s = {"tok": (c.vocab, w), "pos": (c.context, w), "proj.weight": (c.embed_dim, w)}
    s["ln_final.weight"] = s["ln_final.bias"] = (w,)
    for i in range(c.layers):
        L = f"layers.{i}."
        for n in ("ln_1", "ln_2"):
            s[L + n + ".weight"] = s[L + n + ".bias"] = (w,)
        s[L + "qkv.weight"], s[L + "qkv.bias"] = (3 * w, w), (3 * w,)
        s[L + "out.weight"], s[L + "out.bias"] = (w, w), (w,)
        s[L + "fc1.weight"], s[L + "fc1.bias"] = (c.mlp_width, w), (c.mlp_width,)
        s[L + "fc2.weight"], s[L + "fc2.bias"] = (w, c.mlp_width), (w,)
    return s


def _hf_names(c):
    """internal name -> HF name, or a tuple of three (q, k, v) to concatenate"""
    t = "text_model."
    m = {"tok": t + "embeddings.token_embedding.weight", "pos": t + "embeddings.position_embedding.weight",
         "proj.weight": "text_projection.weight"}
    for p in ("weight", "bias"):
        m[f"ln_final.{p}"] = t + f"final_layer_norm.{p}"
        for i in range(c.layers):
            L, H = f"layers.{i}.", t + f"encoder.layers.{i}."
            m[L + f"ln_1.{p}"], m[L + f"ln_2.{p}"] = H + f"layer_norm1.{p}", H + f"layer_norm2.{p}"
            m[L + f"qkv.{p}"] = tuple(H + f"self_attn.{n}_proj.{p}" for n in "qkv")
            m[L + f"out.{p}"] = H + f"self_attn.out_proj.{p}"
            m[L + f"fc1.{p}"], m[L + f"fc2.{p}"] = H + f"mlp.fc1.{p}", H + f"mlp.fc2.{p}"
    return m


def _open_clip_names(c):
    """UNPINNED: open_clip's CLIP text names as recollected (the library is absent offline)."""
    m = {"tok": "token_embedding.weight", "pos": "positional_embedding",
         "proj.weight": "text_projection"}                               # [width, embed]: transposed on conversion
    for p in ("weight", "bias"):
        m[f"ln_final.{p}"] = f"ln_final.{p}"
        for i in range(c.layers):
            L, R = f"layers.{i}.", f"transformer.resblocks.{i}."
            m[L + f"ln_1.{p}"], m[L + f"ln_2.{p}"] = R + f"ln_1.{p}", R + f"ln_2.{p}"
            m[L + f"qkv.{p}"] = R + f"attn.in_proj_{p}"
            m[L + f"out.{p}"] = R + f"attn.out_proj.{p}"
            m[L + f"fc1.{p}"], m[L + f"fc2.{p}"] = R + f"mlp.c_fc.{p}", R + f"mlp.c_proj.{p}"
    return m


_OPEN_CLIP_OWN = ("token_embedding.", "positional_embedding", "transformer.", "ln_final.", "text_projection")


def convert_state_dict(sd, config):
    """A state dict in HF or open_clip names -> (internal dict, logit_scale or None).  Tensors keep their dtype; q | k | v are
    fused, open_clip's `text_projection` is transposed to [embed, width].  Tensors of the text tower that are missing, of the
    wrong shape, or text-tower tensors the layout does not know raise a ValueError that names them; image-tower tensors are
    ignored.  `text_projection` alone may be absent (a bare CLIPTextModel): `encode_text` then raises, `pooled_output` works."""
    if any(k.startswith("text_model.") for k in sd):
        names, own, fixups = _hf_names(config), ("text_model.", "text_projection."), None
    else:
        names, own, fixups = _open_clip_names(config), _OPEN_CLIP_OWN, {"proj.weight": lambda t: t.t()}
    out = convert_names(sd, names, param_shapes(config), own, "CLIP text", OPTIONAL, fixups)
    ls = sd.get("logit_scale")
    return out, (None if ls is None else float(ls))


def config_from_json(raw):
    """`config.json` of a HF CLIPModel (nested `text_config` + `projection_dim`), of a CLIPTextModel[WithProjection] (flat), or
    `{"preset": "CLIP_L_TEXT", ...overrides}`."""
    if "preset" in raw:
        return replace(PRESETS[raw["preset"]], **{k: v for k, v in raw.items() if k in ClipTextConfig.__dataclass_fields__})
    t = raw.get("text_config", raw)
    return ClipTextConfig(vocab=t["vocab_size"], context=t["max_position_embeddings"], width=t["hidden_size"],
                          layers=t["num_hidden_layers"], heads=t["num_attention_heads"], mlp_width=t["intermediate_size"],
                          embed_dim=raw.get("projection_dim", t.get("projection_dim", 512)), act=t.get("hidden_act", "quick_gelu"),
                          layer_norm_eps=t.get("layer_norm_eps", 1e-5), eos_token_id=t.get("eos_token_id", 2))


def pooled_positions(input_ids, eos_token_id):
    """transformers' rule (CLIPTextTransformer.forward): with the legacy eos_token_id == 2 the position of the largest id
    (open_clip's `text.argmax(dim=-1)`: the end-of-text token has the largest id of the vocabulary), otherwise the first
    position that holds eos_token_id.  [B] int64 on the host."""
    ids = input_ids.detach().cpu().long()
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


class ClipTextTower(EncoderHost):
    def __init__(self, config: ClipTextConfig = None, device="cuda"):
        self.config = (config or CLIP_L_TEXT).check()
        super().__init__(device, self.config.width)
        self.logit_scale = None

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, path, device="cuda"):
        """A directory with `config.json` (see `config_from_json`) and one or more `*.safetensors` files in HF or open_clip key
        names; a whole CLIPModel checkpoint loads here and into ClipVisionTower alike."""
        raw, sd = read_checkpoint_dir(path)
        return cls(config_from_json(raw), device=device).load_state_dict(sd)

    def load_state_dict(self, sd):
        """HF or open_clip names (`convert_state_dict`).  Matrices, biases and the token table go to bf16 (the GEMM's operands,
        the gather's rows), LayerNorm parameters and position embeddings stay fp32."""
        t, self.logit_scale = convert_state_dict(sd, self.config)
        self.P = self._place(t)
        return self

    def init_synthetic(self, seed=0):
        """Random weights of the configured architecture drawn on the tower's device, every value a bf16 number, HF key names."""
        return self.load_state_dict(synthetic_state_dict(self.config, seed, self.device))

    # ---------------------------------------------------------------------------------------------- forward
    def _hidden(self, input_ids):
        """token ids [B, S <= context] -> the final LayerNorm of every row, [B S, width] bf16 (a shared buffer)"""
        if self.P is None:
            raise RuntimeError("CLIP text weights not loaded")
        c, P = self.config, self.P
        if input_ids.dim() != 2 or not 1 <= input_ids.shape[1] <= c.context:
            raise ValueError(f"input_ids must be [B, 1 .. {c.context}], not {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        w, H, d, mlp, eps = c.width, c.heads, c.head_dim, c.mlp_width, c.layer_norm_eps
        M = B * S
        x = self._plain("x", M, w)
        ops.token_embed(input_ids, P["tok"], P["pos"], x)       # checks the ids on the host first: nothing launched on a bad one
        n, qkv, o, h = self._plain("n", M, w), self._plain("qkv", M, 3 * w), self._plain("o", M, w), self._plain("h", M, mlp)

        def norm(src, name, dst):
            self._layer_norm(src, name, dst, M, w, eps)

        def attend(qkv, o):
            if not ops.text_attn_fwd(qkv, 3 * w, o, w, B, H, S, d, d ** -0.5, causal=True):
                raise RuntimeError(f"mgx_text_attn_fwd refused {S} tokens")

        def activate(h):
            ops.act_rows(h, mlp, h, mlp, M, mlp, ACTS[c.act])
            return h

        for i in range(c.layers):
            self._prenorm_layer(f"layers.{i}.", x, n, qkv, o, h, norm, attend, activate)
        norm(x, "ln_final", n)
        return n

    @torch.no_grad()
    def pooled_output(self, input_ids):
        """-> [B, width] bf16, a fresh tensor: the final LayerNorm's row at the pooled position (`pooled_positions`) --
        CLIPTextModel's `pooler_output`, which FLUX's `encode_prompt` uses as `pooled_prompt_embeds`."""
        n = self._hidden(input_ids)
        B, S = input_ids.shape
        rows = torch.arange(B) * S + pooled_positions(input_ids, self.config.eos_token_id)
        return n.index_select(0, rows.to(self.device))

    @torch.no_grad()
    def encode_text(self, input_ids, normalize=True):
        """-> [B, embed_dim] fp32: `text_projection` (no bias) of the pooled rows (bf16 values), L2-normalised if `normalize`."""
        pooled = self.pooled_output(input_ids)
        c = self.config
        if "proj.weight" not in self.P:
            raise RuntimeError("this checkpoint has no text_projection (a bare CLIPTextModel): only pooled_output is available")
        B = pooled.shape[0]
        feat = self._plain("feat", B, c.embed_dim)
        ops.skinny_linear(pooled, self.P["proj.weight"], None, feat, c.embed_dim, c.width)
        if not normalize:
            return feat.float()
        out = torch.empty(B, c.embed_dim, dtype=F32, device=self.device)
        ops.l2_normalize_rows(feat, out)
        return out


def synthetic_state_dict(config, seed=0, device="cpu"):
    """A random HF-named state dict of `config`, drawn on `device`, every value a bf16 number held in fp32; logit_scale = ln 100."""
    sd = draw_state_dict(_hf_names(config), param_shapes(config), layer_norm_net_std, seed, device)
    sd["logit_scale"] = torch.tensor(4.605170185988092)
    return sd
