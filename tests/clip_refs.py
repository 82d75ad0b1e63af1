"""float64 restatement of the CLIP image tower and its preprocessing (mixgrpo_amd/clip_vision.py, csrc/clip.hip), plain torch,
device-agnostic.  tests/test_clip_refs.py holds it to transformers' CLIPModel, torch's antialiased bicubic and PIL on the CPU;
tests/test_hip_clip.py holds the kernels to it.

`tower(..., emulate_bf16=True)` is the second arm: the same float64 arithmetic with a bf16 rounding at exactly the points where
the HIP path stores bf16 -- the patch rows, every GEMM output, every LayerNorm output, the activation, the embedding sum, each
residual sum and the attention's O.  Its distance from the float64 arm is the error the number format alone causes; the HIP
result may be twice that (a different fp32 summation order inside GEMM and attention)."""
import math

import torch

from mixgrpo_amd.sample_flux import image_levels

F64 = torch.float64


def bf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------------------------------------------------- preprocess
def cubic(x, a=-0.5):
    x = x.abs()
    return torch.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, torch.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, torch.zeros_like(x)))


def resize_matrix(n_in, n_out):
    """[n_out, n_in] float64 weights of PIL's antialiased BICUBIC (ImagingResample's precompute_coeffs)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    Wm = torch.zeros(n_out, n_in, dtype=F64)
    for i in range(n_out):
        center = (i + 0.5) * scale
        k0 = max(0, int(center - support + 0.5))
        k1 = min(n_in, int(center + support + 0.5))
        k = torch.arange(k0, k1, dtype=F64)
        w = cubic((k - center + 0.5) / fs)
        Wm[i, k0:k1] = w / w.sum()
    return Wm


def resized_hw(H, W, R):
    return (R, R * W // H) if H <= W else (R * H // W, R)


def resize(levels, oh, ow):
    """levels [3, H, W] float64 -> [3, oh, ow], horizontal pass then vertical pass, nothing rounded"""
    _, H, W = levels.shape
    return resize_matrix(H, oh).to(levels.device) @ (levels @ resize_matrix(W, ow).to(levels.device).t())


def preprocess(image, R, patch, mean, std):
    """image [3, H, W] bf16 in about [-1, 1] -> dict: `pre` the resized, cropped image before rounding [3, R, R] float64,
    `levels` its rounding to 0..255, `pixels` (q / 255 - mean) / std float64, `patches` [(R / p)^2, 3 p p] float64."""
    lv = image_levels(image).to(F64)
    _, H, W = lv.shape
    oh, ow = resized_hw(H, W, R)
    top, left = (oh - R) // 2, (ow - R) // 2
    pre = resize(lv, oh, ow)[:, top:top + R, left:left + R]
    q = pre.round().clamp(0, 255)
    m, s = (torch.tensor(v, dtype=F64, device=q.device).view(3, 1, 1) for v in (mean, std))
    pix = (q / 255 - m) / s
    return {"pre": pre, "levels": q, "pixels": pix, "patches": patchify(pix[None], patch)}


def patchify(pixels, p):
    """[B, 3, R, R] -> [B (R / p)^2, 3 p p]: row py (R / p) + px, column c p p + dy p + dx"""
    B, _, R, _ = pixels.shape
    g = R // p
    return pixels.reshape(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * p * p)


RESIZES = [((1024, 1024), 224), ((720, 720), 224), ((64, 48), 28), ((100, 100), 224)]      # (H, W) -> R
TIE = 1e-3            # pixels whose pre-rounding value is this close to k + 1/2 may round either way in fp32
TIE_CAP = 0.005       # ... and may be at most this share of an image


def make_image(H, W, kind, seed=0):
    """[3, H, W] bf16 in [-1, 1]: noise, or a smooth pattern.  The noise is uniform in [-0.7, 0.7] (levels 38 .. 217): a bicubic
    filter overshoots its input's range by up to an eighth of it, and PIL's uint8 image between its two passes clamps what
    leaves 0 .. 255 there, which the fp32 intermediate image of this path, by design, does not."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return (0.7 * (torch.rand(3, H, W, generator=g) * 2 - 1)).bfloat16()
    y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    return torch.stack([torch.sin(7 * x + 3 * y), torch.cos(5 * y * x + 1), 2 * x * y - 1]).bfloat16()


def tie_distance(pre):
    """distance of each value from the nearest rounding tie k + 1/2"""
    f = pre - pre.floor()
    return (f - 0.5).abs()


# ------------------------------------------------------------------------------------------------------------------ tower
def layer_norm(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * g + b


def gelu(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


ACT = {"gelu": gelu, "quick_gelu": quick_gelu}


def tower(P, config, pixel_values, emulate_bf16=False):
    """P: the internal layout of clip_vision.convert_state_dict; pixel_values [B, 3, R, R] -> the projected class token
    [B, embed_dim] float64, not normalised."""
    c = config
    r = bf if emulate_bf16 else (lambda t: t)
    P = {k: v.to(F64).to(pixel_values.device) for k, v in P.items()}
    w, S, H, d = c.width, c.tokens, c.heads, c.head_dim
    B = pixel_values.shape[0]
    patches = r(patchify(pixel_values.to(F64), c.patch_size))
    pe = r(patches @ P["patch.weight"].reshape(w, -1).t()).view(B, S - 1, w)
    x = r(torch.cat([(P["cls"] + P["pos"][0]).expand(B, 1, w), pe + P["pos"][1:]], 1))
    x = r(layer_norm(x, P["ln_pre.weight"], P["ln_pre.bias"], c.layer_norm_eps))
    for i in range(c.layers):
        L = f"layers.{i}."
        n = r(layer_norm(x, P[L + "ln_1.weight"], P[L + "ln_1.bias"], c.layer_norm_eps))
        qkv = r(n @ P[L + "qkv.weight"].t() + P[L + "qkv.bias"])
        q, k, v = (t.view(B, S, H, d).transpose(1, 2) for t in qkv.split(w, -1))
        o = r(attention(q, k, v, d ** -0.5).transpose(1, 2).reshape(B, S, w))
        x = r(x + r(o @ P[L + "out.weight"].t() + P[L + "out.bias"]))
        n = r(layer_norm(x, P[L + "ln_2.weight"], P[L + "ln_2.bias"], c.layer_norm_eps))
        h = r(n @ P[L + "fc1.weight"].t() + P[L + "fc1.bias"])
        h = r(ACT[c.act](h))
        x = r(x + r(h @ P[L + "fc2.weight"].t() + P[L + "fc2.bias"]))
    pooled = r(layer_norm(x[:, 0], P["ln_post.weight"], P["ln_post.bias"], c.layer_norm_eps))
    return r(pooled @ P["proj.weight"].t())


def attention(q, k, v, scale):
    """[..., S, d] float64"""
    return torch.softmax((q.to(F64) @ k.to(F64).transpose(-1, -2)) * scale, -1) @ v.to(F64)


def attention_budget(q, k, v, scale):
    """Per-row budget of the bf16 attention output, as tests/attn_refs.py states it for O:
    u (|O_r| + sqrt(sum_d sum_j P_rj^2 V_jd^2)), u = 2^-9 -- the output rounding plus independent roundings of P_rj."""
    P = torch.softmax((q.to(F64) @ k.to(F64).transpose(-1, -2)) * scale, -1)
    O = P @ v.to(F64)
    return 2.0 ** -9 * (O.norm(dim=-1) + ((P ** 2) @ (v.to(F64) ** 2)).sum(-1).sqrt())


def score(feat, text, logit_scale=1.0, mean=0.0, std=1.0):
    f, t = feat.to(F64), text.to(F64)
    cos = (f * t).sum(-1) / (f.norm(dim=-1) * t.norm(dim=-1))
    return (logit_scale * cos - mean) / std


def rel_l2(a, b):
    return ((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm()).item()


def one_minus_cos(a, b):
    a, b = a.to(F64), b.to(F64)
    return (1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).abs().max().item()
