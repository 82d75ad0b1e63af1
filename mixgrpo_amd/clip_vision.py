"""CLIP ViT image tower on the HIP kernels: the network behind the reference's three usual rewards,
    HPSClipRewardModel (fastvideo/models/reward_model/hps_score.py: open_clip ViT-H/14, `self.reward_model(image, text)` :71),
    PickScoreRewardModel (pick_score.py: transformers CLIPModel, `get_image_features` :73) and
    CLIPScoreRewardModel (clip_score.py: open_clip, `encode_image` :63).
Only the image tower runs in the training loop; the text feature of a prompt is constant and cached (mixgrpo_amd/rewards.py).

Layout: all images of a call are one batch of M = B S token rows, bf16; every Linear is a launch of the persistent GEMM
(`ops.gemm`, without its stream-K workspace, so that an image's rows do not depend on how many images share the call), residual
sums ride the GEMM epilogue with a ones gate, as vae._attention does; csrc/clip.hip holds the rest: the preprocessing (PIL's
antialiased bicubic resize, crop, normalise, patch rows), the embedding, LayerNorm, the exact / quick GELU and the scores' tail;
csrc/encoder_attn.hip the attention that reads the packed q | k | v projection.  The host scaffold (checkpoint reader, key
conversion, synthetic weights, buffers, the Linear launch, the pre-norm layer) is encoder_host.py's, shared with the other
encoders; `VitTrunk` here is the ViT up to its last layer, which image_reward.BlipVisionEncoder runs as well.

Weights: HF `CLIPModel` / `CLIPVisionModelWithProjection` key names (pinned against transformers by tests/test_clip_refs.py) or
open_clip's `visual.*` names (recollected: the library is absent offline, PARITY UNPINNED), both converted to one internal
layout with the fused q | k | v weight [3 width, width] (`convert_state_dict`)."""
import json
import os
from dataclasses import dataclass, replace
from typing import Tuple

import torch

from . import ops
from .encoder_host import EncoderHost, convert_names, draw_state_dict, layer_norm_net_std, read_checkpoint_dir
from .ops import BF16, F32

OPENAI_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_STD = (0.26862954, 0.26130258, 0.27577711)
ACTS = {"gelu": ops.ACT_GELU, "quick_gelu": ops.ACT_QUICK_GELU}


@dataclass
class ClipVisionConfig:
    width: int = 1280
    layers: int = 32
    heads: int = 16
    mlp_width: int = 5120
    patch_size: int = 14
    image_size: int = 224
    embed_dim: int = 1024
    act: str = "gelu"
    layer_norm_eps: float = 1e-5
    image_mean: Tuple[float, ...] = OPENAI_MEAN
    image_std: Tuple[float, ...] = OPENAI_STD

    @property
    def head_dim(self):
        return self.width // self.heads

    @property
    def grid(self):
        return self.image_size // self.patch_size

    @property
    def tokens(self):
        return 1 + self.grid * self.grid

    def check(self):
        d = self.head_dim
        if self.width % self.heads or d % 16 or d > 128:
            raise ValueError(f"head dim {self.width}/{self.heads}: the attention kernel takes multiples of 16 up to 128")
        if self.width % 64 or self.width > 2048 or self.mlp_width % 64 or self.embed_dim % 4:
            raise ValueError("width and mlp_width must be multiples of 64 (width <= 2048), embed_dim a multiple of 4")
        if self.image_size % self.patch_size or self.tokens > 4096:
            raise ValueError("image_size must be a multiple of patch_size, with at most 4096 tokens")
        if self.act not in ACTS:
            raise ValueError(f"act must be one of {sorted(ACTS)}, not {self.act!r}")
        return self


VIT_H_14 = ClipVisionConfig()
VIT_L_14 = ClipVisionConfig(width=1024, layers=24, heads=16, mlp_width=4096, embed_dim=768, act="quick_gelu")
PRESETS = {"VIT_H_14": VIT_H_14, "VIT_L_14": VIT_L_14}


# ------------------------------------------------------------------------------------------------------------- key formats
def param_shapes(c):
    """name -> shape of the internal layout."""
    w, p = c.width, c.patch_size
    s = {"patch.weight": (w, 3, p, p), "cls": (w,), "pos": (c.tokens, w), "proj.weight": (c.embed_dim, w)}
    for n in ("ln_pre", "ln_post"):
        s[n + ".weight"] = s[n + ".bias"] = (w,)
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
    v = "vision_model."
    m = {"patch.weight": v + "embeddings.patch_embedding.weight", "cls": v + "embeddings.class_embedding",
         "pos": v + "embeddings.position_embedding.weight", "proj.weight": "visual_projection.weight"}
    for t in ("weight", "bias"):
        m[f"ln_pre.{t}"] = v + f"pre_layrnorm.{t}"                       # (sic: transformers' spelling)
        m[f"ln_post.{t}"] = v + f"post_layernorm.{t}"
        for i in range(c.layers):
            L, H = f"layers.{i}.", v + f"encoder.layers.{i}."
            m[L + f"ln_1.{t}"], m[L + f"ln_2.{t}"] = H + f"layer_norm1.{t}", H + f"layer_norm2.{t}"
            m[L + f"qkv.{t}"] = tuple(H + f"self_attn.{n}_proj.{t}" for n in "qkv")
            m[L + f"out.{t}"] = H + f"self_attn.out_proj.{t}"
            m[L + f"fc1.{t}"], m[L + f"fc2.{t}"] = H + f"mlp.fc1.{t}", H + f"mlp.fc2.{t}"
    return m


def _open_clip_names(c):
    v = "visual."
    m = {"patch.weight": v + "conv1.weight", "cls": v + "class_embedding", "pos": v + "positional_embedding",
         "proj.weight": v + "proj"}                                      # proj is [width, embed]: transposed on conversion
    for t in ("weight", "bias"):
        m[f"ln_pre.{t}"], m[f"ln_post.{t}"] = v + f"ln_pre.{t}", v + f"ln_post.{t}"
        for i in range(c.layers):
            L, R = f"layers.{i}.", v + f"transformer.resblocks.{i}."
            m[L + f"ln_1.{t}"], m[L + f"ln_2.{t}"] = R + f"ln_1.{t}", R + f"ln_2.{t}"
            m[L + f"qkv.{t}"] = R + f"attn.in_proj_{t}"
            m[L + f"out.{t}"] = R + f"attn.out_proj.{t}"
            m[L + f"fc1.{t}"], m[L + f"fc2.{t}"] = R + f"mlp.c_fc.{t}", R + f"mlp.c_proj.{t}"
    return m


def convert_state_dict(sd, config):
    """A state dict in HF or open_clip names -> (internal dict, logit_scale or None).  Tensors keep their dtype; q | k | v are
    fused, open_clip's `visual.proj` is transposed to [embed, width].  Tensors of the tower that are missing, of the wrong shape,
    or vision-tower tensors the layout does not know raise a ValueError that names them; text-tower tensors are ignored."""
    if any(k.startswith("vision_model.") for k in sd):
        names, own, fixups = _hf_names(config), ("vision_model.", "visual_projection."), None
    else:
        names, own, fixups = _open_clip_names(config), ("visual.",), {"proj.weight": lambda t: t.t()}
    out = convert_names(sd, names, param_shapes(config), own, "CLIP vision", fixups=fixups)
    ls = sd.get("logit_scale")
    return out, (None if ls is None else float(ls))


def config_from_json(raw):
    """`config.json` of a HF CLIPModel (nested `vision_config` + `projection_dim`) or CLIPVisionModelWithProjection (flat), or
    `{"preset": "VIT_H_14", ...overrides}`."""
    if "preset" in raw:
        return replace(PRESETS[raw["preset"]], **{k: v for k, v in raw.items() if k in ClipVisionConfig.__dataclass_fields__})
    v = raw.get("vision_config", raw)
    return ClipVisionConfig(width=v["hidden_size"], layers=v["num_hidden_layers"], heads=v["num_attention_heads"],
                            mlp_width=v["intermediate_size"], patch_size=v["patch_size"], image_size=v["image_size"],
                            embed_dim=raw.get("projection_dim", v.get("projection_dim", 512)), act=v.get("hidden_act", "quick_gelu"),
                            layer_norm_eps=v.get("layer_norm_eps", 1e-5))


def pil_pixel_values(image, config):
    """What the reference's processors do to a PIL image, on the host: RGB, PIL's own bicubic resize of the shortest edge, centre
    crop, `(q / 255 - mean) / std` -> [3, R, R] fp32."""
    import numpy as np
    from PIL import Image
    R = config.image_size
    image = image.convert("RGB")
    W, H = image.size
    ow, oh = (int(R * W / H), R) if H <= W else (R, int(R * H / W))
    image = image.resize((ow, oh), Image.BICUBIC)
    left, top = (ow - R) // 2, (oh - R) // 2
    a = torch.from_numpy(np.asarray(image.crop((left, top, left + R, top + R)), dtype=np.float32).copy()).permute(2, 0, 1)
    mean, std = (torch.tensor(v, dtype=F32).view(3, 1, 1) for v in (config.image_mean, config.image_std))
    return (a / 255.0 - mean) / std


class VitTrunk(EncoderHost):
    """The ViT both image encoders run (ClipVisionTower here, image_reward.BlipVisionEncoder): preprocessing, the padded patch
    weight, and patch GEMM (bias optional) -> `vit_embed` -> `ln_pre` if the network has one -> the pre-norm layers.  `P` is
    the internal layout of `param_shapes`; what follows the last layer is the subclass's."""
    label = "CLIP vision"

    def __init__(self, config, device="cuda"):
        self.config = config.check()
        super().__init__(device, self.config.width)

    def _load(self, t):
        """A converted dict onto the device (`_place`); the patch weight is flattened to [width, 3 p p] and zero-padded to the
        GEMM's K % 64 == 0."""
        c = self.config
        P = self._place({k: v for k, v in t.items() if k != "patch.weight"})
        w = torch.zeros(c.width, ops.clip_patch_cols(c.patch_size), dtype=BF16, device=self.device)
        w[:, :3 * c.patch_size ** 2] = t["patch.weight"].to(self.device).reshape(c.width, -1).to(BF16)
        P["patch.weight"] = w
        self.P = P
        return self

    def preprocess(self, images):
        """Decoded images ([3, H, W] device tensors in about [-1, 1], a list or a [B, 3, H, W] tensor; sizes may differ) -> patch
        rows [B (R / p)^2, Kp] bf16, a shared buffer.  PIL images are resized by PIL on the host, as the reference does."""
        c = self.config
        n = c.grid * c.grid
        images = list(images)
        out = self._plain("patches", len(images) * n, ops.clip_patch_cols(c.patch_size))
        for i, im in enumerate(images):
            if not torch.is_tensor(im):
                out[i * n:(i + 1) * n].copy_(self._patchify(pil_pixel_values(im, c)[None].to(self.device)))
                continue
            if im.dim() != 3 or im.shape[0] != 3:
                raise ValueError(f"an image is [3, H, W], not {tuple(im.shape)}")
            ops.clip_preprocess(im.to(self.device, BF16).contiguous(), c.image_size, c.patch_size, c.image_mean, c.image_std,
                                out[i * n:(i + 1) * n])
        return out

    def _patchify(self, pixel_values):
        """[B, 3, R, R] normalised pixels -> patch rows (the layout of mgx_clip_preprocess), a fresh tensor"""
        c = self.config
        B, g, p = pixel_values.shape[0], c.grid, c.patch_size
        if tuple(pixel_values.shape[1:]) != (3, c.image_size, c.image_size):
            raise ValueError(f"pixel_values must be [B, 3, {c.image_size}, {c.image_size}], not {tuple(pixel_values.shape)}")
        rows = pixel_values.to(self.device, BF16).view(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * p * p)
        out = torch.zeros(B * g * g, ops.clip_patch_cols(p), dtype=BF16, device=self.device)
        out[:, :3 * p * p] = rows
        return out

    def _trunk(self, images, pixel_values, act):
        """Decoded `images` (see `preprocess`) or `pixel_values` [B, 3, R, R] already resized and normalised -> (the residual
        stream after the last layer [B tokens, width] bf16, a shared buffer; B).  `act`: the MLP's activation (ops.ACT_*)."""
        if self.P is None:
            raise RuntimeError(f"{self.label} weights not loaded")
        if (images is None) == (pixel_values is None):
            raise ValueError("give images or pixel_values")
        c, P = self.config, self.P
        patches = self.preprocess(images) if pixel_values is None else self._patchify(pixel_values)
        w, S, H, d, mlp, eps = c.width, c.tokens, c.heads, c.head_dim, c.mlp_width, c.layer_norm_eps
        B = patches.shape[0] // (S - 1)
        M = B * S
        pe = self._plain("patch_out", B * (S - 1), w)
        self._linear(patches, "patch", pe)
        x = self._plain("x", M, w)
        ops.vit_embed(pe, P["cls"], P["pos"], x, B, S, w)
        if "ln_pre.weight" in P:
            self._layer_norm(x, "ln_pre", x, M, w, eps)
        n, qkv, o, h = self._plain("n", M, w), self._plain("qkv", M, 3 * w), self._plain("o", M, w), self._plain("h", M, mlp)

        def norm(src, name, dst):
            self._layer_norm(src, name, dst, M, w, eps)

        def attend(qkv, o):
            if not ops.vit_attn_fwd(qkv, 3 * w, o, w, B, H, S, d, d ** -0.5):
                raise RuntimeError(f"mgx_vit_attn_fwd refused {S} tokens")

        def activate(h):
            ops.act_rows(h, mlp, h, mlp, M, mlp, act)
            return h

        for i in range(c.layers):
            self._prenorm_layer(f"layers.{i}.", x, n, qkv, o, h, norm, attend, activate)
        return x, B


class ClipVisionTower(VitTrunk):
    def __init__(self, config: ClipVisionConfig = None, device="cuda"):
        super().__init__(config or VIT_H_14, device)
        self.logit_scale = None

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, path, device="cuda"):
        """A directory with `config.json` (see `config_from_json`), optionally `preprocessor_config.json` (image_mean / image_std)
        and one or more `*.safetensors` files in HF or open_clip key names."""
        raw, sd = read_checkpoint_dir(path)
        cfg = config_from_json(raw)
        pp = os.path.join(path, "preprocessor_config.json")
        if os.path.exists(pp):
            with open(pp) as f:
                raw = json.load(f)
            if "image_mean" in raw and "image_std" in raw:
                cfg = replace(cfg, image_mean=tuple(raw["image_mean"]), image_std=tuple(raw["image_std"]))
        return cls(cfg, device=device).load_state_dict(sd)

    def load_state_dict(self, sd):
        """HF or open_clip names (`convert_state_dict`).  Matrices and biases go to bf16 (the GEMM's operands), LayerNorm
        parameters, class token and position embeddings stay fp32; the patch weight is flattened and padded (`_load`)."""
        t, self.logit_scale = convert_state_dict(sd, self.config)
        return self._load(t)

    def init_synthetic(self, seed=0):
        """Random weights of the configured architecture drawn on the tower's device, every value a bf16 number (no checkpoint
        offline), HF key names."""
        return self.load_state_dict(synthetic_state_dict(self.config, seed, self.device))

    # ---------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def encode_image(self, images=None, pixel_values=None, normalize=True):
        """-> [B, embed_dim] fp32: the projected class token (bf16 values), L2-normalised if `normalize`.  Give decoded `images`
        (see `preprocess`) or `pixel_values` [B, 3, R, R] already resized and normalised."""
        c = self.config
        x, B = self._trunk(images, pixel_values, ACTS[c.act])
        w = c.width
        pooled = self._plain("pooled", B, w)
        self._layer_norm(x, "ln_post", pooled, B, w, c.layer_norm_eps, ldx=c.tokens * w)                  # the class rows
        feat = self._plain("feat", B, c.embed_dim)
        ops.skinny_linear(pooled, self.P["proj.weight"], None, feat, c.embed_dim, w)
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
