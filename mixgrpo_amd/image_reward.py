"""ImageReward on the HIP kernels: the reference's ImageRewardModel (fastvideo/models/reward_model/image_reward.py:24-40:
`RM.load(...)` builds the network, `self.model.inference_rank(text, [image])` :38 scores one pair).  Three parts:
    BlipVisionEncoder   BLIP's ViT (ViT-L/16 at 224: 197 tokens): no pre-LayerNorm, a patch convolution with a bias, LayerNorm eps
                        1e-6, exact GELU, the final `norm` on every token, no projection;
    BlipTextEncoder     BERT-base, post-LayerNorm with eps 1e-12, word + position embeddings, and in every layer a cross-attention
                        sub-layer between self-attention and FFN whose keys and values come from the image tokens; the prompt is
                        padded to 35 tokens and the self-attention skips the padding keys;
    the head            five Linears without activations on the hidden state of token 0, in fp32, then `(r - mean) / std`.
Inference only.

Layout, as clip_vision.py and clip_text.py: all pairs of a call are one batch of token rows, bf16; every Linear of the two
encoders is a launch of the persistent GEMM without its stream-K workspace (a pair's rows do not depend on what shares the
call), residual sums ride the GEMM epilogue with a ones gate (encoder_host.py).  The image encoder is clip_vision.VitTrunk with
its own tail; the text encoder's post-norm layer is a loop of its own on the shared helpers.  The image tokens are the same for
every text layer, so the cross-attention keys and values of ALL layers come from ONE GEMM, weight [layers x 2 x width,
encoder_width]; layer i reads its K and V out of that buffer through `mgx_xattn_fwd`'s row strides.  Padded query rows are
computed like any other; only row 0 of a prompt is used.  Excluded keys are excluded exactly: upstream adds -10000
(transformers: finfo.min) to their scores, a weight that underflows to exactly 0 in fp32 and fp64 alike.

Weights: one state dict in either of two key formats, converted to one internal layout (`convert_state_dict`):
    (a) transformers' names: `vision_model.` + BlipVisionModel's keys, `text_encoder.` + BlipTextModel's keys (pinned against
        transformers by tests/test_blip_refs.py), `mlp.layers.{0,2,4,6,7}` for the head;
    (b) upstream ImageReward's names, `blip.visual_encoder.*`, `blip.text_encoder.*`, `mlp.layers.*` -- recollected: the library is
        absent offline, PARITY UNPINNED.
The default mean and std are recollected from upstream ImageReward as well.  The tokenizer is delegated to transformers."""
import json
import math
from dataclasses import dataclass, replace

import torch

from . import ops
from .clip_vision import ClipVisionConfig, VitTrunk
from .encoder_host import EncoderHost, convert_names, draw_state_dict, layer_norm_net_std
from .ops import BF16, F32

MEAN, STD = 0.16717362830052426, 1.0333394966054072      # recollected from upstream ImageReward (ImageReward.py), unpinned
HEAD_WIDTHS = (1024, 128, 64, 16, 1)
HEAD_LAYERS = (0, 2, 4, 6, 7)                             # the Linears of upstream's nn.Sequential (dropouts in between)
MAX_LENGTH = 35


@dataclass
class BlipVisionConfig(ClipVisionConfig):
    """ClipVisionConfig's fields with BLIP's ViT-L/16 as defaults; `embed_dim` is unused (there is no projection)."""
    width: int = 1024
    layers: int = 24
    heads: int = 16
    mlp_width: int = 4096
    patch_size: int = 16
    image_size: int = 224
    embed_dim: int = 0
    act: str = "gelu"
    layer_norm_eps: float = 1e-6


@dataclass
class BertXattnConfig:
    vocab: int = 30524
    positions: int = 512
    width: int = 768
    layers: int = 12
    heads: int = 12
    mlp_width: int = 3072
    layer_norm_eps: float = 1e-12
    encoder_width: int = 1024

    @property
    def head_dim(self):
        return self.width // self.heads

    def check(self):
        d = self.head_dim
        if self.width % self.heads or d % 16 or d > 128:
            raise ValueError(f"head dim {self.width}/{self.heads}: the attention kernel takes multiples of 16 up to 128")
        if self.width % 64 or self.width > 2048 or self.mlp_width % 64 or self.encoder_width % 64:
            raise ValueError("width, mlp_width and encoder_width must be multiples of 64 (width <= 2048)")
        if not 1 <= self.positions <= 4096 or self.vocab < 1:
            raise ValueError("positions must be 1 .. 4096 and the vocabulary non-empty")
        return self


BLIP_VIT_L_16 = BlipVisionConfig()
BERT_BASE_XATTN = BertXattnConfig()


def bert_config_from_json(raw, encoder_width):
    """BLIP's `med_config.json` (a BertConfig).  `encoder_width` is the image encoder's width: BLIP overwrites the file's own
    value with it (`med_config.encoder_width = vision_width`)."""
    if raw.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act {raw['hidden_act']!r}: only the exact GELU is built")
    return BertXattnConfig(vocab=raw["vocab_size"], positions=raw["max_position_embeddings"], width=raw["hidden_size"],
                           layers=raw["num_hidden_layers"], heads=raw["num_attention_heads"], mlp_width=raw["intermediate_size"],
                           layer_norm_eps=raw.get("layer_norm_eps", 1e-12), encoder_width=encoder_width)


# ------------------------------------------------------------------------------------------------------------- key formats
def param_shapes(vc, tc):
    """name -> shape of the internal layout: `vis.*`, `txt.*`, `head.*`."""
    w, p = vc.width, vc.patch_size
    s = {"vis.patch.weight": (w, 3, p, p), "vis.patch.bias": (w,), "vis.cls": (w,), "vis.pos": (vc.tokens, w)}
    s["vis.ln_post.weight"] = s["vis.ln_post.bias"] = (w,)
    for i in range(vc.layers):
        L = f"vis.layers.{i}."
        for n in ("ln_1", "ln_2"):
            s[L + n + ".weight"] = s[L + n + ".bias"] = (w,)
        s[L + "qkv.weight"], s[L + "qkv.bias"] = (3 * w, w), (3 * w,)
        s[L + "out.weight"], s[L + "out.bias"] = (w, w), (w,)
        s[L + "fc1.weight"], s[L + "fc1.bias"] = (vc.mlp_width, w), (vc.mlp_width,)
        s[L + "fc2.weight"], s[L + "fc2.bias"] = (w, vc.mlp_width), (w,)
    w, e = tc.width, tc.encoder_width
    s["txt.tok"], s["txt.pos"] = (tc.vocab, w), (tc.positions, w)
    s["txt.ln_emb.weight"] = s["txt.ln_emb.bias"] = (w,)
    s["txt.xkv.weight"], s["txt.xkv.bias"] = (tc.layers * 2 * w, e), (tc.layers * 2 * w,)     # layer i: k at 2 w i, v at 2 w i + w
    for i in range(tc.layers):
        L = f"txt.layers.{i}."
        for n in ("ln_attn", "ln_x", "ln_out"):
            s[L + n + ".weight"] = s[L + n + ".bias"] = (w,)
        s[L + "qkv.weight"], s[L + "qkv.bias"] = (3 * w, w), (3 * w,)
        for n in ("out", "xq", "xout"):
            s[L + n + ".weight"], s[L + n + ".bias"] = (w, w), (w,)
        s[L + "fc1.weight"], s[L + "fc1.bias"] = (tc.mlp_width, w), (tc.mlp_width,)
        s[L + "fc2.weight"], s[L + "fc2.bias"] = (w, tc.mlp_width), (w,)
    k = w
    for j, n in enumerate(HEAD_WIDTHS):
        s[f"head.{j}.weight"], s[f"head.{j}.bias"] = (n, k), (n,)
        k = n
    return s


def _text_names(tc, t):
    """internal name -> name under the prefix `t`, or a tuple of names to concatenate: transformers' BlipTextModel and
    upstream's BertModel share these leaf names"""
    m = {"txt.tok": t + "embeddings.word_embeddings.weight", "txt.pos": t + "embeddings.position_embeddings.weight"}
    for p in ("weight", "bias"):
        m[f"txt.ln_emb.{p}"] = t + f"embeddings.LayerNorm.{p}"
        m[f"txt.xkv.{p}"] = tuple(t + f"encoder.layer.{i}.crossattention.self.{n}.{p}" for i in range(tc.layers) for n in ("key", "value"))
        for i in range(tc.layers):
            L, S = f"txt.layers.{i}.", t + f"encoder.layer.{i}."
            m[L + f"qkv.{p}"] = tuple(S + f"attention.self.{n}.{p}" for n in ("query", "key", "value"))
            m[L + f"out.{p}"], m[L + f"ln_attn.{p}"] = S + f"attention.output.dense.{p}", S + f"attention.output.LayerNorm.{p}"
            m[L + f"xq.{p}"] = S + f"crossattention.self.query.{p}"
            m[L + f"xout.{p}"], m[L + f"ln_x.{p}"] = S + f"crossattention.output.dense.{p}", S + f"crossattention.output.LayerNorm.{p}"
            m[L + f"fc1.{p}"], m[L + f"fc2.{p}"] = S + f"intermediate.dense.{p}", S + f"output.dense.{p}"
            m[L + f"ln_out.{p}"] = S + f"output.LayerNorm.{p}"
    return m


def _head_names():
    return {f"head.{j}.{p}": f"mlp.layers.{n}.{p}" for j, n in enumerate(HEAD_LAYERS) for p in ("weight", "bias")}


def _hf_names(vc, tc):
    """(a): `vision_model.` + BlipVisionModel's keys, `text_encoder.` + BlipTextModel's keys, the head"""
    v = "vision_model."
    m = {"vis.patch.weight": v + "embeddings.patch_embedding.weight", "vis.patch.bias": v + "embeddings.patch_embedding.bias",
         "vis.cls": v + "embeddings.class_embedding", "vis.pos": v + "embeddings.position_embedding"}
    for p in ("weight", "bias"):
        m[f"vis.ln_post.{p}"] = v + f"post_layernorm.{p}"
        for i in range(vc.layers):
            L, S = f"vis.layers.{i}.", v + f"encoder.layers.{i}."
            m[L + f"ln_1.{p}"], m[L + f"ln_2.{p}"] = S + f"layer_norm1.{p}", S + f"layer_norm2.{p}"
            m[L + f"qkv.{p}"], m[L + f"out.{p}"] = S + f"self_attn.qkv.{p}", S + f"self_attn.projection.{p}"
            m[L + f"fc1.{p}"], m[L + f"fc2.{p}"] = S + f"mlp.fc1.{p}", S + f"mlp.fc2.{p}"
    return {**m, **_text_names(tc, "text_encoder."), **_head_names()}


def _upstream_names(vc, tc):
    """(b) UNPINNED: upstream ImageReward's names as recollected (BLIP's VisionTransformer and BertModel under `blip.`)"""
    v = "blip.visual_encoder."
    m = {"vis.patch.weight": v + "patch_embed.proj.weight", "vis.patch.bias": v + "patch_embed.proj.bias",
         "vis.cls": v + "cls_token", "vis.pos": v + "pos_embed"}
    for p in ("weight", "bias"):
        m[f"vis.ln_post.{p}"] = v + f"norm.{p}"
        for i in range(vc.layers):
            L, S = f"vis.layers.{i}.", v + f"blocks.{i}."
            m[L + f"ln_1.{p}"], m[L + f"ln_2.{p}"] = S + f"norm1.{p}", S + f"norm2.{p}"
            m[L + f"qkv.{p}"], m[L + f"out.{p}"] = S + f"attn.qkv.{p}", S + f"attn.proj.{p}"
            m[L + f"fc1.{p}"], m[L + f"fc2.{p}"] = S + f"mlp.fc1.{p}", S + f"mlp.fc2.{p}"
    return {**m, **_text_names(tc, "blip.text_encoder."), **_head_names()}


_PREFIXES = {True: ("vision_model.", "text_encoder.", "mlp."), False: ("blip.visual_encoder.", "blip.text_encoder.", "mlp.")}


def _is_upstream(sd):
    return any(k.startswith("blip.") for k in sd)


def convert_state_dict(sd, vision_config, text_config):
    """A state dict in format (a) or (b) (module docstring) -> the internal dict of `param_shapes`.  Tensors keep their dtype;
    q | k | v of the self-attention are fused, the cross-attention keys and values of all layers are stacked into `txt.xkv`,
    the class token [1, 1, w] and the position embeddings [1, S, w] lose their leading ones.  Tensors that are missing, of the
    wrong shape, or unknown under the format's prefixes raise a ValueError that names them; `position_ids` buffers are ignored."""
    hf = not _is_upstream(sd)
    names = _hf_names(vision_config, text_config) if hf else _upstream_names(vision_config, text_config)
    fixups = {"vis.cls": lambda t: t[0, 0] if t.dim() == 3 and tuple(t.shape[:2]) == (1, 1) else t,
              "vis.pos": lambda t: t[0] if t.dim() == 3 and t.shape[0] == 1 else t}
    return convert_names(sd, names, param_shapes(vision_config, text_config), _PREFIXES[hf], "ImageReward", fixups=fixups)


def vision_config_from_state_dict(sd):
    """The image encoder's sizes as the checkpoint's own tensors give them (ImageReward ships no config file for it): width,
    patch size, token count, depth and MLP width; heads = width / 64, as in every BLIP ViT."""
    hf = not _is_upstream(sd)
    n = (_hf_names if hf else _upstream_names)(replace(BLIP_VIT_L_16, layers=1), replace(BERT_BASE_XATTN, layers=0))
    need = [n["vis.patch.weight"], n["vis.pos"], n["vis.layers.0.fc1.weight"]]
    miss = [k for k in need if k not in sd]
    if miss:
        raise ValueError(f"ImageReward state dict: missing {miss}")
    pw, pos, fc1 = (sd[k] for k in need)
    stem = n["vis.layers.0.fc1.weight"].split("0.mlp.fc1.weight")[0]
    layers = 1 + max(int(k[len(stem):].split(".")[0]) for k in sd if k.startswith(stem))
    grid = math.isqrt(pos.shape[-2] - 1)
    return replace(BLIP_VIT_L_16, width=pw.shape[0], patch_size=pw.shape[-1], image_size=grid * pw.shape[-1], layers=layers,
                   mlp_width=fc1.shape[0], heads=max(pw.shape[0] // 64, 1))


# -------------------------------------------------------------------------------------------------------------- tokenizer
def load_tokenizer(path, max_length=MAX_LENGTH):
    """A tokenizer directory (BLIP's BertTokenizer) -> `prompts -> (input_ids [n, max_length] int64, lengths [n] int64)` on the
    host, as inference_rank tokenises: padding="max_length", truncation=True.  transformers is imported here, on first use."""
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(path)

    def tokenize(prompts):
        enc = tok(list(prompts), padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
        return enc.input_ids, enc.attention_mask.sum(-1)
    return tokenize


# ------------------------------------------------------------------------------------------------------------ image encoder
class BlipVisionEncoder(VitTrunk):
    """BLIP's ViT on the trunk ClipVisionTower runs: its buffers, preprocessing (`mgx_clip_preprocess`) and kernels.  `P`: the
    `vis.*` entries of the internal layout, without the prefix.  The weights come through ImageRewardModel only, and there is no
    projection: the tower's entry points for those refuse."""
    label = "BLIP vision"

    def __init__(self, config: BlipVisionConfig = None, device="cuda"):
        super().__init__(config or BLIP_VIT_L_16, device)

    @classmethod
    def from_pretrained(cls, path, device="cuda"):
        raise NotImplementedError("load an ImageReward checkpoint with ImageRewardModel.from_pretrained")

    def load_state_dict(self, sd):
        raise NotImplementedError("load an ImageReward checkpoint with ImageRewardModel.load_state_dict")

    def init_synthetic(self, seed=0):
        raise NotImplementedError("ImageRewardModel.init_synthetic draws the weights of all three parts")

    def load_internal(self, t):
        """The `vis.*` tensors (prefix stripped).  Matrices and biases go to bf16, LayerNorm parameters, class token and position
        embeddings stay fp32; the patch weight is flattened to [width, 3 p p], zero-padded to the GEMM's K % 64 == 0."""
        return self._load(t)

    def encode_image(self, *a, **k):
        raise NotImplementedError("BLIP's ViT has no projection: use encode_tokens")

    @torch.no_grad()
    def encode_tokens(self, images=None, pixel_values=None):
        """-> [B tokens, width] bf16 (a shared buffer): the final LayerNorm of every token.  Give decoded `images`
        (VitTrunk.preprocess) or `pixel_values` [B, 3, R, R] already resized and normalised."""
        x, B = self._trunk(images, pixel_values, ops.ACT_GELU)
        c = self.config
        tokens = self._plain("tokens", B * c.tokens, c.width)
        self._layer_norm(x, "ln_post", tokens, B * c.tokens, c.width, c.layer_norm_eps)
        return tokens


# ------------------------------------------------------------------------------------------------------------- text encoder
class BlipTextEncoder(EncoderHost):
    """BERT with a cross-attention sub-layer in every layer.  `P`: the `txt.*` entries of the internal layout, without the
    prefix."""

    def __init__(self, config: BertXattnConfig = None, device="cuda"):
        self.config = (config or BERT_BASE_XATTN).check()
        super().__init__(device, self.config.width)
        self.launches = 0                   # kernel launches of the last `encode` (the rows are few: the encoder is latency-bound)

    def load_internal(self, t):
        """Matrices, biases and the word table go to bf16, LayerNorm parameters and position embeddings stay fp32."""
        self.P = self._place(t)
        return self

    @torch.no_grad()
    def encode(self, input_ids, lengths, image_tokens):
        """input_ids [B, S] and lengths [B] (integer tensors, normally on the host: both are checked there), image_tokens
        [B T, encoder_width] bf16 (T image tokens per prompt) -> the last layer's hidden states [B S, width] bf16, a shared buffer.
        The self-attention of prompt b sees its first lengths[b] tokens; the rows from lengths[b] on are computed, and mean
        nothing."""
        if self.P is None:
            raise RuntimeError("BLIP text weights not loaded")
        c, P = self.config, self.P
        if input_ids.dim() != 2 or not 1 <= input_ids.shape[1] <= c.positions:
            raise ValueError(f"input_ids must be [B, 1 .. {c.positions}], not {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        w, H, d, mlp, eps, e = c.width, c.heads, c.head_dim, c.mlp_width, c.layer_norm_eps, c.encoder_width
        if image_tokens.dim() != 2 or image_tokens.shape[1] != e or image_tokens.shape[0] % B or image_tokens.dtype != BF16:
            raise ValueError(f"image_tokens must be bf16 [{B} T, {e}], not {image_tokens.dtype} {tuple(image_tokens.shape)}")
        T = image_tokens.shape[0] // B
        M = B * S
        count = [0]

        def linear(a, name, out, residual=False):
            count[0] += 1
            self._linear(a, name, out, residual)

        def norm(name):
            count[0] += 1
            self._layer_norm(x, name, x, M, w, eps)

        def attend(*a, **kw):
            count[0] += 1
            if not ops.xattn_fwd(*a, **kw):
                raise RuntimeError(f"mgx_xattn_fwd refused {S} queries against {max(S, T)} keys")

        x = self._plain("x", M, w)
        qkv, q, o, h = self._plain("qkv", M, 3 * w), self._plain("q", M, w), self._plain("o", M, w), self._plain("h", M, mlp)
        ops.check_kv_len(lengths, B, S)                         # both host checks come first: nothing is launched on a bad
        ops.token_embed(input_ids, P["tok"], P["pos"], x)              # id or a bad length
        count[0] += 1
        norm("ln_emb")
        ldkv = c.layers * 2 * w
        kv = self._plain("xkv", B * T, ldkv)
        linear(image_tokens, "xkv", kv)
        lens = lengths.to(device=self.device, dtype=torch.int32)
        for i in range(c.layers):
            L = f"layers.{i}."
            linear(x, L + "qkv", qkv)
            attend(qkv, 3 * w, qkv[:, w:], 3 * w, qkv[:, 2 * w:], 3 * w, o, w, B, H, S, S, d, d ** -0.5, kv_len=lens,
                   kv_len_checked=True)
            linear(o, L + "out", x, residual=True)
            norm(L + "ln_attn")
            linear(x, L + "xq", q)
            attend(q, w, kv[:, 2 * w * i:], ldkv, kv[:, 2 * w * i + w:], ldkv, o, w, B, H, S, T, d, d ** -0.5)
            linear(o, L + "xout", x, residual=True)
            norm(L + "ln_x")
            linear(x, L + "fc1", h)
            ops.act_rows(h, mlp, h, mlp, M, mlp, ops.ACT_GELU)
            count[0] += 1
            linear(h, L + "fc2", x, residual=True)
            norm(L + "ln_out")
        self.launches = count[0]
        return x


# ------------------------------------------------------------------------------------------------------------------ scorer
def _split(t, prefix):
    return {k[len(prefix):]: v for k, v in t.items() if k.startswith(prefix)}


class ImageRewardModel(EncoderHost):
    """`(images, prompts) -> list[float]`, the order reward_adapter.compute_reward uses; all pairs of a call run as one batch.
    Images are [3, H, W] device tensors as AutoencoderKL.decode returns them (PIL images take ClipVisionTower's host path).
    `tokenizer`: a callable `prompts -> (input_ids [n, 35], lengths [n])` or a tokenizer directory (`load_tokenizer`, on first
    use).  The score is `(head(h[:, 0]) - mean) / std`."""

    def __init__(self, vision_config=None, text_config=None, tokenizer=None, mean=MEAN, std=STD, device="cuda"):
        self.vision = BlipVisionEncoder(vision_config, device=device)
        self.text = BlipTextEncoder(text_config or replace(BERT_BASE_XATTN, encoder_width=self.vision.config.width), device=device)
        if self.text.config.encoder_width != self.vision.config.width:
            raise ValueError(f"encoder_width {self.text.config.encoder_width} is not the image encoder's width {self.vision.config.width}")
        super().__init__(self.vision.device)
        self.tokenizer, self.mean, self.std = tokenizer, float(mean), float(std)
        if self.std == 0.0:
            raise ValueError("std must not be 0")
        self.head = None

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, checkpoint, med_config, tokenizer=None, mean=MEAN, std=STD, device="cuda"):
        """`checkpoint`: a .safetensors file, or a .pt file (a plain state dict, read with weights_only=True), in key format (a)
        or (b); `med_config`: BLIP's med_config.json.  The image encoder's sizes are read off the checkpoint's tensors."""
        if str(checkpoint).endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(str(checkpoint))
        else:
            sd = torch.load(str(checkpoint), map_location="cpu", weights_only=True)
        with open(med_config) as f:
            raw = json.load(f)
        vc = vision_config_from_state_dict(sd)
        return cls(vc, bert_config_from_json(raw, vc.width), tokenizer, mean, std, device).load_state_dict(sd)

    def load_state_dict(self, sd):
        """Key format (a) or (b) (`convert_state_dict`).  The head stays fp32."""
        t = convert_state_dict(sd, self.vision.config, self.text.config)
        self.vision.load_internal(_split(t, "vis."))
        self.text.load_internal(_split(t, "txt."))
        self.head = [(t[f"head.{j}.weight"].to(self.device, F32).contiguous(), t[f"head.{j}.bias"].to(self.device, F32).contiguous())
                     for j in range(len(HEAD_WIDTHS))]
        return self

    def init_synthetic(self, seed=0):
        """Random weights of the configured architecture drawn on the model's device, transformers' key names."""
        return self.load_state_dict(synthetic_state_dict(self.vision.config, self.text.config, seed, self.device))

    # ---------------------------------------------------------------------------------------------- forward
    def tokenize(self, prompts):
        if self.tokenizer is None:
            raise ValueError("ImageRewardModel needs a tokenizer: a callable prompts -> (ids, lengths) or a tokenizer directory")
        if not callable(self.tokenizer):                       # a directory: transformers is imported on first use only
            self.tokenizer = load_tokenizer(self.tokenizer, MAX_LENGTH)
        ids, lengths = self.tokenizer(prompts)
        if ids.dim() != 2 or ids.shape[0] != len(prompts) or tuple(lengths.shape) != (len(prompts),):
            raise ValueError(f"the tokenizer returned ids {tuple(ids.shape)} and lengths {tuple(lengths.shape)} for {len(prompts)} prompts")
        return ids, lengths

    @torch.no_grad()
    def score_tokens(self, input_ids, lengths, images=None, pixel_values=None):
        """-> [B] fp32 on the device: the scores of B (image, tokenised prompt) pairs"""
        if self.head is None:
            raise RuntimeError("ImageReward weights not loaded")
        tokens = self.vision.encode_tokens(images, pixel_values)
        hidden = self.text.encode(input_ids, lengths, tokens)
        B, S = input_ids.shape
        x = hidden.view(B, S * self.text.config.width)[:, :self.text.config.width]     # row 0 of every prompt, strided
        for j, (W, b) in enumerate(self.head):
            last = j == len(self.head) - 1
            y = self._plain(f"head{j}", B, W.shape[0], F32) if not last else torch.empty(B, 1, dtype=F32, device=self.device)
            ops.linear_rows_f32(x, W, b, y, *((self.mean, self.std) if last else ()))
            x = y
        return x.view(B)

    @torch.no_grad()
    def __call__(self, images, prompts):
        if isinstance(prompts, str):
            prompts = [prompts]
        if torch.is_tensor(images):
            images = list(images) if images.dim() == 4 else [images]
        elif not isinstance(images, (list, tuple)):
            images = [images]
        if len(images) != len(prompts):
            raise ValueError(f"{len(images)} images for {len(prompts)} prompts")
        ids, lengths = self.tokenize(list(prompts))            # before anything is launched
        return self.score_tokens(ids, lengths, images=images).tolist()


def synthetic_state_dict(vision_config, text_config, seed=0, device="cpu"):
    """A random state dict of the two configurations in transformers' names (format (a)), drawn on `device`, every value a bf16
    number held in fp32.  The text encoder's query weights are drawn four times as large as fan-in scaling would, so that the
    attention is not nearly uniform."""
    def std(name, key, s):
        sigma = layer_norm_net_std(name, key, s)
        return 4.0 * sigma if key.endswith("self.query.weight") else sigma
    names = _hf_names(vision_config, text_config)
    sd = draw_state_dict(names, param_shapes(vision_config, text_config), std, seed, device)
    for name, lead in (("vis.cls", (1, 1)), ("vis.pos", (1,))):     # transformers keeps them [1, 1, w] and [1, S, w]
        sd[names[name]] = sd[names[name]].view(lead + tuple(sd[names[name]].shape))
    return sd
