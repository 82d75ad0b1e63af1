"""CLIP ViT image tower on the HIP kernels: the network behind the reference's three usual rewards,
    HPSClipRewardModel (fastvideo/models/reward_model/hps_score.py: open_clip ViT-H/14, `self.reward_model(image, text)` :71),
    PickScoreRewardModel (pick_score.py: transformers CLIPModel, `get_image_features` :73) and
    CLIPScoreRewardModel (clip_score.py: open_clip, `encode_image` :63).
Only the image tower runs in the training loop; the text feature of a prompt is constant and cached (mixgrpo_amd/rewards.py).

Layout: all images of a call are one batch of M = B S token rows, bf16; every Linear is a launch of the persistent GEMM
(`ops.gemm`, without its stream-K workspace, so that an image's rows do not depend on how many images share the call), residual
sums ride the GEMM epilogue with a ones gate, as vae._attention does; csrc/clip.hip holds the rest: the preprocessing (PIL's
antialiased bicubic resize, crop, normalise, patch rows), the embedding, LayerNorm, the attention that reads the packed q | k | v
projection, the exact / quick GELU and the scores' tail.

Weights: HF `CLIPModel` / `CLIPVisionModelWithProjection` key names (pinned against transformers by tests/test_clip_refs.py) or
open_clip's `visual.*` names (recollected: the library is absent offline, PARITY UNPINNED), both converted to one internal
layout with the fused q | k | v weight [3 width, width] (`convert_state_dict`)."""
import json
import os
from dataclasses import dataclass, replace
from typing import Tuple

import torch

from . import ops
from .ops import BF16, F32, Rows, EPI_BIAS_GATE_RES

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
    hf = any(k.startswith("vision_model.") for k in sd)
    names = _hf_names(config) if hf else _open_clip_names(config)
    prefix = ("vision_model.", "visual_projection.") if hf else ("visual.",)
    out, missing, used = {}, [], set()
    for name, src in names.items():
        parts = src if isinstance(src, tuple) else (src,)
        miss = [p for p in parts if p not in sd]
        if miss:
            missing += miss
            continue
        used.update(parts)
        t = torch.cat([sd[p] for p in parts], 0) if len(parts) > 1 else sd[parts[0]]
        if name == "proj.weight" and not hf:
            t = t.t()
        out[name] = t
    unknown = sorted(k for k in sd if k.startswith(prefix) and k not in used and not k.endswith("position_ids"))
    if missing or unknown:
        raise ValueError(f"CLIP vision state dict: missing {sorted(missing)[:8]} ({len(missing)}), unknown {unknown[:8]} ({len(unknown)})")
    bad = [f"{k} {tuple(out[k].shape)} != {shp}" for k, shp in param_shapes(config).items() if tuple(out[k].shape) != tuple(shp)]
    if bad:
        raise ValueError(f"CLIP vision state dict: wrong shapes: {bad[:8]}")
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


class ClipVisionTower:
    def __init__(self, config: ClipVisionConfig = None, device="cuda"):
        self.config = (config or VIT_H_14).check()
        self.device = torch.device(device)
        self.P = None
        self.logit_scale = None
        self._buf = {}
        self._ones = torch.ones(max(self.config.width, 512), dtype=BF16, device=self.device)

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, path, device="cuda"):
        """A directory with `config.json` (see `config_from_json`), optionally `preprocessor_config.json` (image_mean / image_std)
        and one or more `*.safetensors` files in HF or open_clip key names."""
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = config_from_json(json.load(f))
        pp = os.path.join(path, "preprocessor_config.json")
        if os.path.exists(pp):
            with open(pp) as f:
                raw = json.load(f)
            if "image_mean" in raw and "image_std" in raw:
                cfg = replace(cfg, image_mean=tuple(raw["image_mean"]), image_std=tuple(raw["image_std"]))
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors file in {path}")
        sd = {}
        for f in files:
            sd.update(load_file(os.path.join(path, f)))
        return cls(cfg, device=device).load_state_dict(sd)

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def load_state_dict(self, sd):
        """HF or open_clip names (`convert_state_dict`).  Matrices and biases go to bf16 (the GEMM's operands), LayerNorm
        parameters, class token and position embeddings stay fp32; the patch weight is flattened to [width, 3 p p] and
        zero-padded to the GEMM's K % 64 == 0."""
        c, dev = self.config, self.device
        t, self.logit_scale = convert_state_dict(sd, c)
        P = {}
        Kp = ops.clip_patch_cols(c.patch_size)
        for k, v in t.items():
            v = v.to(dev)
            if k == "patch.weight":
                w = torch.zeros(c.width, Kp, dtype=BF16, device=dev)
                w[:, :3 * c.patch_size ** 2] = v.reshape(c.width, -1).to(BF16)
                P[k] = w
            elif k in ("cls", "pos") or ".ln_" in k or k.startswith("ln_"):
                P[k] = v.to(F32).contiguous()
            else:
                P[k] = v.to(BF16).contiguous()
        self.P = P
        return self

    def init_synthetic(self, seed=0):
        """Random weights of the configured architecture drawn on the tower's device, every value a bf16 number (no checkpoint
        offline), HF key names."""
        return self.load_state_dict(synthetic_state_dict(self.config, seed, self.device))

    # ---------------------------------------------------------------------------------------------- buffers
    def _plain(self, tag, M, C, dtype=BF16):
        key = (tag, M, C, dtype)
        t = self._buf.get(key)
        if t is None:
            t = self._buf[key] = torch.empty(M, C, dtype=dtype, device=self.device)
        return t

    # ---------------------------------------------------------------------------------------------- forward
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

    @torch.no_grad()
    def encode_image(self, images=None, pixel_values=None, normalize=True):
        """-> [B, embed_dim] fp32: the projected class token (bf16 values), L2-normalised if `normalize`.  Give decoded `images`
        (see `preprocess`) or `pixel_values` [B, 3, R, R] already resized and normalised."""
        if self.P is None:
            raise RuntimeError("CLIP vision weights not loaded")
        if (images is None) == (pixel_values is None):
            raise ValueError("give images or pixel_values")
        c, P = self.config, self.P
        patches = self.preprocess(images) if pixel_values is None else self._patchify(pixel_values)
        w, S, H, d, mlp, eps = c.width, c.tokens, c.heads, c.head_dim, c.mlp_width, c.layer_norm_eps
        B = patches.shape[0] // (S - 1)
        M = B * S
        gemm = lambda a, W, b, out, N, K, **kw: ops.gemm(Rows.of(a), W, b, Rows.of(out), N, K, stream_k=False, **kw)
        pe = self._plain("patch_out", B * (S - 1), w)
        gemm(patches, P["patch.weight"], None, pe, w, patches.shape[1])
        x = self._plain("x", M, w)
        ops.vit_embed(pe, P["cls"], P["pos"], x, B, S, w)
        ops.layer_norm_affine(x, w, P["ln_pre.weight"], P["ln_pre.bias"], x, w, M, w, eps)
        n, qkv, o, h = self._plain("n", M, w), self._plain("qkv", M, 3 * w), self._plain("o", M, w), self._plain("h", M, mlp)
        for i in range(c.layers):
            L = f"layers.{i}."
            ops.layer_norm_affine(x, w, P[L + "ln_1.weight"], P[L + "ln_1.bias"], n, w, M, w, eps)
            gemm(n, P[L + "qkv.weight"], P[L + "qkv.bias"], qkv, 3 * w, w)
            if not ops.vit_attn_fwd(qkv, 3 * w, o, w, B, H, S, d, d ** -0.5):
                raise RuntimeError(f"mgx_vit_attn_fwd refused {S} tokens")
            gemm(o, P[L + "out.weight"], P[L + "out.bias"], x, w, w, epi=EPI_BIAS_GATE_RES, gate=self._ones, gate_ld=0)
            ops.layer_norm_affine(x, w, P[L + "ln_2.weight"], P[L + "ln_2.bias"], n, w, M, w, eps)
            gemm(n, P[L + "fc1.weight"], P[L + "fc1.bias"], h, mlp, w)
            ops.act_rows(h, mlp, h, mlp, M, mlp, ACTS[c.act])
            gemm(h, P[L + "fc2.weight"], P[L + "fc2.bias"], x, w, mlp, epi=EPI_BIAS_GATE_RES, gate=self._ones, gate_ld=0)
        pooled = self._plain("pooled", B, w)
        ops.layer_norm_affine(x, S * w, P["ln_post.weight"], P["ln_post.bias"], pooled, w, B, w, eps)    # the class rows
        feat = self._plain("feat", B, c.embed_dim)
        ops.skinny_linear(pooled, P["proj.weight"], None, feat, c.embed_dim, w)
        if not normalize:
            return feat.float()
        out = torch.empty(B, c.embed_dim, dtype=F32, device=self.device)
        ops.l2_normalize_rows(feat, out)
        return out


def synthetic_state_dict(config, seed=0, device="cpu"):
    """A random HF-named state dict of `config`, drawn on `device`, every value a bf16 number held in fp32; logit_scale = ln 100."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda shp, std: (std * torch.randn(shp, generator=g, device=device)).to(BF16).float()
    sd = {}
    for name, src in _hf_names(config).items():
        shp = param_shapes(config)[name]
        for j, key in enumerate(src if isinstance(src, tuple) else (src,)):
            s = (shp[0] // 3,) + tuple(shp[1:]) if isinstance(src, tuple) else shp
            if name in ("cls", "pos"):
                sd[key] = r(s, 0.5)
            elif name.endswith("weight") and len(shp) == 1:
                sd[key] = (1.0 + 0.1 * torch.randn(s, generator=g, device=device)).to(BF16).float()
            elif name.endswith("bias"):
                sd[key] = r(s, 0.05)
            else:
                fan_in = 1
                for v in s[1:]:
                    fan_in *= v
                sd[key] = r(s, fan_in ** -0.5)
    sd["logit_scale"] = torch.tensor(4.605170185988092)
    return sd
