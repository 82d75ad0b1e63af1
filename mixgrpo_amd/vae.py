"""FLUX VAE on the HIP kernels: the `vae` object of the reference's rollout,
    vae = AutoencoderKL.from_pretrained(path, subfolder="vae", torch_dtype=torch.bfloat16)       (train_grpo_flux.py:697-701)
    vae.enable_tiling(); image = vae.decode(latents, return_dict=False)[0]                        (:279-289)
-- diffusers' AutoencoderKL.  Same constructor call, `.config`, `.enable_tiling()`, `.decode(z, return_dict=False)`; weights from
the published `vae/diffusion_pytorch_model.safetensors` (diffusers key names).  The trainer never encodes; the encoder half
(`.encode(x).latent_dist.sample()`, `.tiled_encode`) is here for image-to-image sampling, latent datasets and the
`encode(decode(z))` self-check of a set of weights: the same kernels in the opposite order, with a stride-2 convolution
(Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride=2) -- recollected from diffusers, parity unpinned) in place of
the upsampler and the DiagonalGaussianDistribution of fastvideo/models/hunyuan/vae/vae.py:321-353 behind conv_out.  Encode tiling
follows `spatial_tiled_encode` (autoencoder_kl_causal_3d.py:408-470): the MOMENTS of the tiles are blended, then one Gaussian.

Layout: one image at a time, activations NHWC bf16; every 3x3 convolution is an implicit GEMM on the MFMA GEMM kernels over a
zero-bordered copy written by the GroupNorm + SiLU (or upsample) pass in front of it, residual sums ride the GEMM epilogue, the
mid block's single-head attention (H W <= 16384 tokens of dim 512) is two GEMMs around an fp32 row softmax.  All arithmetic is in
csrc/ (gemm.hip, vae.hip); this file sequences it, walking the layer list of mixgrpo_amd/vae_arch.py, which also gives the
key inventory of both halves.  Tiling follows the reference lineage's `spatial_tiled_decode`
(fastvideo/models/hunyuan/vae/autoencoder_kl_causal_3d.py:472-525): a 1024^2 image (128^2 latent) is exactly one tile and is
decoded whole; larger images are decoded tile by tile and blended (in place on the later tile, :384-399).  That tiling is
pinned to the reference's vendored 3-D lineage; parity with diffusers' AutoencoderKL.tiled_decode is unpinned.
"""
import json
import os
from dataclasses import dataclass
from typing import Tuple

import torch

from . import ops
from .ops import BF16, F32, Rows, EPI_BIAS, EPI_BIAS_GATE_RES, EPI_F32_ACC
from .vae_arch import HALVES, layers, param_shapes


@dataclass
class VaeConfig:
    latent_channels: int = 16
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    sample_size: int = 1024
    scaling_factor: float = 0.3611
    shift_factor: float = 0.1159
    mid_block_add_attention: bool = True
    in_channels: int = 3                 # the encoder's three: other values are refused at `encode`
    use_quant_conv: bool = False         # (FLUX's VAE has no quant conv)
    double_z: bool = True


def _pad_ch(c):
    for p in (64, 128, 256, 512):
        if c <= p:
            return p
    raise ValueError(f"{c} channels: the convolution kernels take up to 512 per tap")


class AutoencoderKL:
    def __init__(self, config: VaeConfig = None, device="cuda"):
        self.config = config or VaeConfig()
        self.device = torch.device(device)
        self.use_tiling = False
        c = self.config
        self.tile_sample_min_size = c.sample_size
        self.tile_latent_min_size = int(c.sample_size / (2 ** (len(c.block_out_channels) - 1)))
        self.tile_overlap_factor = 0.25
        for ch in c.block_out_channels:
            if ch not in (64, 128, 256, 512):
                raise ValueError("block_out_channels must be 64, 128, 256 or 512 (channels per convolution tap)")
        self.P = None
        self.has_encoder = False
        self._buf = {}
        self._ones = torch.ones(512, dtype=BF16, device=self.device)

    # ---------------------------------------------------------------------------------------------- weights
    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None, device="cuda"):
        from safetensors.torch import load_file
        if subfolder and os.path.isdir(os.path.join(path, subfolder)):
            path = os.path.join(path, subfolder)
        with open(os.path.join(path, "config.json")) as f:
            raw = json.load(f)
        keys = set(VaeConfig.__dataclass_fields__)
        cfg = VaeConfig(**{k: (tuple(v) if k == "block_out_channels" else v) for k, v in raw.items()
                           if k in keys and v is not None})
        m = cls(cfg, device=device)
        m.load_state_dict(load_file(os.path.join(path, "diffusion_pytorch_model.safetensors")))
        return m

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def load_state_dict(self, sd):
        """diffusers keys.  `decoder.*` is required; `encoder.*` is loaded if and only if EVERY encoder tensor is there (a state
        dict with none or only some of them gives a decoder-only object: `has_encoder` False); quant-conv entries are ignored.
        Conv weights OIHW -> [O][kh][kw][I] bf16 with the input channels padded to the kernel's tap width and the output
        channels to a multiple of 4."""
        P = {}
        for half in HALVES:
            keys = list(param_shapes(self.config, half))
            missing = [k for k in keys if k not in sd]
            if missing and half == "decoder":
                raise KeyError(f"VAE state dict lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")
            if not missing:
                self._convert(sd, keys, half, P)
        self.has_encoder = any(k.startswith("encoder.") for k in P)
        self.P = P
        return self

    def _convert(self, sd, keys, half, P):
        dev = self.device
        for k in keys:
            t = sd[k].to(dev)
            if t.dim() == 4 and t.shape[-1] == 3:
                O, I = t.shape[0], t.shape[1]
                Ip, Op = _pad_ch(I), (O + 3) // 4 * 4
                w = torch.zeros(Op, 3, 3, Ip, dtype=BF16, device=dev)
                w[:O, :, :, :I] = t.permute(0, 2, 3, 1).to(BF16)
                P[k] = w.contiguous()
            elif t.dim() == 4:                                   # 1x1 shortcut
                P[k] = t[:, :, 0, 0].to(BF16).contiguous()
            elif k.endswith("conv_out.bias"):
                b = torch.zeros((t.shape[0] + 3) // 4 * 4 + 4, dtype=BF16, device=dev)   # 16-byte sized
                b[:t.shape[0]] = t.to(BF16)
                P[k] = b
            else:
                P[k] = t.to(BF16).contiguous()
        for a in (l.name for l in layers(self.config, half) if l.kind == "attention"):      # q | k | v as one GEMM operand
            P[a + ".qkv.weight"] = torch.cat([P[f"{a}.to_{n}.weight"] for n in "qkv"], 0).contiguous()
            P[a + ".qkv.bias"] = torch.cat([P[f"{a}.to_{n}.bias"] for n in "qkv"], 0).contiguous()

    def init_synthetic(self, seed=0):
        """Random bf16 weights of the configured architecture (no checkpoint offline); the decoder's from the same generator as
        oracle/vae.py, the encoder's from a second one (seed + 1) drawn after them, so the decoder's do not depend on it."""
        sd = {}
        for i, half in enumerate(HALVES):
            g = torch.Generator().manual_seed(seed + i)
            for k, shp in param_shapes(self.config, half).items():
                if k.endswith(".weight") and len(shp) == 1:
                    sd[k] = (1.0 + 0.1 * torch.randn(shp, generator=g)).to(BF16)
                elif k.endswith(".bias"):
                    sd[k] = (0.05 * torch.randn(shp, generator=g)).to(BF16)
                else:
                    fan_in = shp[1] * (shp[2] * shp[3] if len(shp) == 4 else 1)
                    sd[k] = (torch.randn(shp, generator=g) / fan_in ** 0.5).to(BF16)
        return self.load_state_dict(sd)

    # ---------------------------------------------------------------------------------------------- buffers
    def _plain(self, tag, M, C, dtype=BF16):
        key = (tag, M, C, dtype)
        t = self._buf.get(key)
        if t is None:
            t = self._buf[key] = torch.empty(M, C, dtype=dtype, device=self.device)
        return t

    def _padded(self, H, W, C, tag="pad"):
        key = (tag, H, W, C)
        t = self._buf.get(key)
        if t is None:                                           # zero border = the convolutions' padding; interiors only are written
            t = self._buf[key] = torch.zeros(H + 2, W + 2, C, dtype=BF16, device=self.device)
        return t

    # ---------------------------------------------------------------------------------------------- blocks
    def _resnet(self, name, x, H, W, Cin, Cout):
        P, G = self.P, self.config.norm_num_groups
        pad = self._padded(H, W, Cin)
        ops.group_norm(x, P[name + ".norm1.weight"], P[name + ".norm1.bias"], pad, H, W, Cin, G, True, True)
        h = self._plain("h", H * W, Cout)
        ops.conv3x3(pad, P[name + ".conv1.weight"], P[name + ".conv1.bias"], h, H, W, Cin, Cout)
        pad2 = self._padded(H, W, Cout)
        ops.group_norm(h, P[name + ".norm2.weight"], P[name + ".norm2.bias"], pad2, H, W, Cout, G, True, True)
        if Cin != Cout:                                          # 1x1 conv_shortcut: a plain GEMM over the pixels
            y = self._plain("x", H * W, Cout)                    # another buffer than x: keyed by the channel count
            ops.gemm(Rows.of(x), P[name + ".conv_shortcut.weight"], P[name + ".conv_shortcut.bias"], Rows.of(y), Cout, Cin)
            x = y
        ops.conv3x3(pad2, P[name + ".conv2.weight"], P[name + ".conv2.bias"], x, H, W, Cout, Cout, ones=self._ones)
        return x

    def _attention(self, name, x, H, W, C):
        """x [H W, C] plain bf16 -> x + to_out(softmax(q k^T / sqrt(C)) v) of GroupNorm(x), in place: single-head attention over
        the H W tokens, any H W up to 16384 (more is refused here, before anything is launched).  The GEMM writes S = q k^T with
        a column count that is a multiple of 4, so for H W % 4 != 0 S gets up to three spare columns, computed from zeroed
        spare k rows and never read by the softmax; the contraction of P v is zero-padded to a multiple of 64."""
        P, G = self.P, self.config.norm_num_groups
        M = H * W
        if M > 16384:
            raise ValueError("mid-block attention handles up to 16384 tokens (a 128 x 128 latent tile)")
        M4 = (M + 3) // 4 * 4
        n = self._plain("attn_n", M, C)
        ops.group_norm(x, P[name + ".group_norm.weight"], P[name + ".group_norm.bias"], n, H, W, C, G, False, False)
        qkv = self._plain("attn_qkv", M4, 3 * C)
        if M4 != M:
            qkv[M:].zero_()
        ops.gemm(Rows.of(n), P[name + ".qkv.weight"], P[name + ".qkv.bias"], Rows(qkv, M, 3 * C), 3 * C, C)
        S = self._plain("attn_s", M, M4, F32)
        ops.gemm(Rows(qkv, M, 3 * C), qkv[0, C:], None, Rows.of(S), M4, C, EPI_F32_ACC, beta=0.0, ldw=3 * C)    # q k^T, fp32
        Pm = self._plain("attn_p", M, M)
        ops.softmax_rows(S, Pm, M, M, float(C) ** -0.5)
        Mp = (M + 63) // 64 * 64
        vt = self._plain("attn_vt", C, Mp)
        if Mp != M:
            vt.zero_()
        ops.transpose(Rows(qkv[0, 2 * C:], M, 3 * C), C, vt, Mp)
        o = self._plain("attn_o", M, C)
        K = M if M % 64 == 0 else None
        if K is None:                                            # contraction length must be a multiple of 64: zero-padded P
            Pp = self._plain("attn_pp", M, Mp)
            Pp.zero_()
            Pp[:, :M].copy_(Pm)
            Pm, K = Pp, Mp
        ops.gemm(Rows.of(Pm), vt, None, Rows.of(o), C, K, ldw=Mp)
        ops.gemm(Rows.of(o), P[name + ".to_out.0.weight"], P[name + ".to_out.0.bias"], Rows.of(x), C, C, EPI_BIAS_GATE_RES,
                 gate=self._ones, gate_ld=0)
        return x

    def _walk(self, half, t):
        """One image through the layers of `half`: t [C, H, W] fp32 on the device -> the decoder's image [out_channels, H', W']
        bf16, or the encoder's moments (see `_encoder`).  Both results are fresh tensors, not shared buffers: a batch stacks
        them and the tiling keeps several."""
        P, G = self.P, self.config.norm_num_groups
        _, H, W = t.shape
        for kind, name, ci, co in layers(self.config, half):
            if kind == "conv_in":
                # its own buffer: only the first `ci` of its Cp channels are ever written, the rest must stay the zeros of the
                # allocation (conv_in's weight is zero there, but 0 * inf = NaN) -- the shared ("pad", H, W, 64) buffer of a
                # 64-channel layer at the same resolution would leave stale activations in them
                Cp = _pad_ch(ci)
                pad = self._padded(H, W, Cp, tag="pad_z" if half == "decoder" else "pad_x")
                ops.latents_to_pad(t.contiguous(), pad, ci, H, W, Cp)
                x = self._plain("x", H * W, co)
                ops.conv3x3(pad, P[name + ".weight"], P[name + ".bias"], x, H, W, Cp, co)
            elif kind == "resnet":
                x = self._resnet(name, x, H, W, ci, co)
            elif kind == "attention":
                x = self._attention(name, x, H, W, ci)
            elif kind == "upsample":
                pad = self._padded(2 * H, 2 * W, co)
                ops.upsample2x_pad(x, pad, H, W, co)
                H, W = 2 * H, 2 * W
                x = self._plain("x", H * W, co)
                ops.conv3x3(pad, P[name + ".weight"], P[name + ".bias"], x, H, W, co, co)
            elif kind == "downsample":                           # Downsample2D(padding=0): pad right / bottom, 3x3 stride 2
                pad = self._padded(H, W, co)
                ops.pad_nhwc(x, co, pad, H, W, co)
                y = self._plain("x", (H // 2) * (W // 2), co)
                ops.conv3x3s2(pad, P[name + ".weight"], P[name + ".bias"], y, H, W, co, co)
                H, W, x = H // 2, W // 2, y
            elif kind == "norm_out":
                pad = self._padded(H, W, ci)
                ops.group_norm(x, P[name + ".weight"], P[name + ".bias"], pad, H, W, ci, G, True, True)
            elif half == "decoder":                              # conv_out, to NHWC rows of 8 and from there to the image
                y = self._plain("img_nhwc", H * W, 8)
                ops.conv3x3(pad, P[name + ".weight"], P[name + ".bias"], y, H, W, ci, (co + 3) // 4 * 4, ld_out=8)
                out = torch.empty(co, H, W, dtype=BF16, device=self.device)
                ops.nhwc_to_image(y, 8, out, co, H, W)
            else:                                                # conv_out, onto the moments
                out = torch.empty(H * W, co, dtype=BF16, device=self.device)
                ops.conv3x3(pad, P[name + ".weight"], P[name + ".bias"], out, H, W, ci, co)
        return out

    def _decoder(self, z):
        """z [latent_channels, h, w] fp32 on the device -> image [out_channels, 8h, 8w] bf16"""
        if self.P is None:
            raise RuntimeError("VAE weights not loaded")
        return self._walk("decoder", z)

    def _encoder(self, x):
        """x [in_channels, H, W] fp32 on the device -> the moments, plain NHWC bf16 [(H / f)(W / f)][2 latent_channels] with
        f = 2^(len(block_out_channels) - 1): channels [0, latent_channels) the mean, the rest the logvar."""
        f = 2 ** (len(self.config.block_out_channels) - 1)
        _, H, W = x.shape
        if H % f or W % f or H <= 0 or W <= 0:
            raise ValueError(f"the encoder takes image sides that are multiples of {f}, not {H} x {W}")
        return self._walk("encoder", x)

    # ---------------------------------------------------------------------------------------------- public surface
    def enable_tiling(self, use_tiling=True):
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.use_tiling = False

    def _decode_batch(self, z):
        return torch.stack([self._decoder(z[b].float()) for b in range(z.shape[0])])

    def tiled_decode(self, z):
        """autoencoder_kl_causal_3d.py:472-525 in 2-D: latent tiles of `tile_latent_min_size`, their images blended and cropped."""
        tl, ts, ov = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        return _tiled(z, tl, int(tl * (1 - ov)), int(ts * ov), ts - int(ts * ov), -2, -1, self._decode_batch)

    @torch.no_grad()
    def decode(self, z, return_dict=True, generator=None):
        """z [B, latent_channels, h, w] (already un-scaled: `latents / scaling_factor + shift_factor`, :286) -> images
        [B, 3, 8h, 8w] bf16.  Tiled only when a latent side exceeds the tile (autoencoder_kl_causal_3d.py:338-342)."""
        z = z.to(self.device)
        tl = self.tile_latent_min_size
        if self.use_tiling and (z.shape[-1] > tl or z.shape[-2] > tl):
            img = self.tiled_decode(z)
        else:
            img = self._decode_batch(z)
        return {"sample": img} if return_dict else (img,)

    def _encode_batch(self, x):
        """x [B, 3, H, W] -> moments NHWC [B, H / f, W / f, 2 latent_channels] bf16"""
        f = 2 ** (len(self.config.block_out_channels) - 1)
        return torch.stack([self._encoder(x[b].float()).view(x.shape[-2] // f, x.shape[-1] // f, -1) for b in range(x.shape[0])])

    def _tiled_moments(self, x):
        """autoencoder_kl_causal_3d.py:408-462 in 2-D, on NHWC moments (rows are dim 1, columns dim 2): image tiles of
        `tile_sample_min_size`, their moments blended and cropped."""
        tl, ts, ov = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        return _tiled(x, ts, int(ts * (1 - ov)), int(tl * ov), tl - int(tl * ov), 1, 2, self._encode_batch)

    def _check_encode(self):
        c = self.config
        if c.in_channels != 3 or c.use_quant_conv or not c.double_z or c.latent_channels % 2:
            raise ValueError("encode handles in_channels = 3, use_quant_conv = False, double_z = True and an even number of "
                             "latent channels (the FLUX VAE)")
        if self.P is None:
            raise RuntimeError("VAE weights not loaded")
        if not self.has_encoder:
            raise RuntimeError("this VAE is decoder-only: its state dict did not hold every encoder.* tensor, so it has no encoder")

    def _posterior(self, mom, return_dict):
        dist = DiagonalGaussianDistribution(mom, self.config.latent_channels)
        return AutoencoderKLOutput(dist) if return_dict else (dist,)

    @torch.no_grad()
    def tiled_encode(self, x, return_dict=True, return_moments=False):
        """`spatial_tiled_encode` (autoencoder_kl_causal_3d.py:408-470): one Gaussian over the blended moments (:466), or --
        `return_moments` (:463-464) -- the moments themselves, [B, 2 latent_channels, h, w]."""
        self._check_encode()
        mom = self._tiled_moments(x.to(self.device))
        return mom.permute(0, 3, 1, 2) if return_moments else self._posterior(mom, return_dict)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        """x [B, 3, H, W] in [-1, 1] -> `.latent_dist`, the posterior over [B, latent_channels, H / 8, W / 8] latents (raw: the
        caller applies `(z - shift_factor) * scaling_factor`).  Tiled only when tiling is enabled and a side exceeds the tile
        (autoencoder_kl_causal_3d.py:307-310); a 1024^2 image is one tile."""
        self._check_encode()
        x = x.to(self.device)
        ts = self.tile_sample_min_size
        tiled = self.use_tiling and (x.shape[-1] > ts or x.shape[-2] > ts)
        return self._posterior(self._tiled_moments(x) if tiled else self._encode_batch(x), return_dict)


class AutoencoderKLOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class DiagonalGaussianDistribution:
    """fastvideo/models/hunyuan/vae/vae.py:321-353,384 on bf16 tensors, from NHWC moments [B, h, w, 2 Cz] (csrc/vae.hip:
    mgx_diag_gaussian_nhwc).  `.parameters`, `.mean`, `.logvar` (clamped), `.std`, `.var` are [B, Cz or 2 Cz, h, w] bf16."""

    def __init__(self, moments, Cz):
        self._moments, self._Cz = moments.contiguous(), Cz
        self.parameters = self._moments.permute(0, 3, 1, 2)
        self.mean, self.std, _ = self._run(None)
        self.logvar = torch.clamp(self.parameters[:, Cz:], -30.0, 20.0)
        self.var = torch.exp(self.logvar)

    def _run(self, noise):
        m = self._moments
        B, h, w, ld = m.shape
        mean, std, sample = (torch.empty(B, self._Cz, h, w, dtype=BF16, device=m.device) for _ in range(3))
        for b in range(B):
            ops.diag_gaussian(m[b], ld, None if noise is None else noise[b], mean[b], std[b], sample[b], self._Cz, h, w)
        return mean, std, sample

    def sample(self, generator=None):
        """mean + std * noise, the noise drawn as bf16 on the device (on the generator's device, if one is given)."""
        dev = self.mean.device
        noise = torch.randn(self.mean.shape, generator=generator, device=dev if generator is None else generator.device,
                            dtype=BF16).to(dev)
        return self._run(noise)[2]

    def mode(self):
        return self.mean


def _blend(a, b, blend_extent, dim):
    """blend_v (dim -2) / blend_h (dim -1) of the reference lineage, vectorised over the blended rows.  Per element, as torch
    evaluates `a[y] * (1 - y / e) + b[y] * (y / e)` on bf16 tensors with python-float weights: each product is formed in fp32 with
    the fp32 weight and rounded to bf16, then the two bf16 products are added and rounded once more.  In place on b."""
    e = min(a.shape[dim], b.shape[dim], blend_extent)
    if e <= 0:
        return b
    shape = [1] * b.dim()
    shape[dim] = e
    wb = torch.tensor([y / e for y in range(e)], dtype=torch.float64)
    wa = (1.0 - wb).to(F32).to(b.device).view(shape)           # python computes 1 - y / e in double, torch takes it as fp32
    wb = wb.to(F32).to(b.device).view(shape)
    src = a.narrow(dim, a.shape[dim] - e, e)
    dst = b.narrow(dim, 0, e)
    dst.copy_((src.float() * wa).to(BF16) + (dst.float() * wb).to(BF16))
    return b


def _tiled(t, tile, stride, blend_extent, limit, rows_dim, cols_dim, run):
    """The tile walk of `spatial_tiled_decode` / `spatial_tiled_encode` (autoencoder_kl_causal_3d.py:472-525, 408-462) in 2-D:
    `run` on the tiles of side `tile`, `stride` apart, of t [B, C, H, W]; each result blended over `blend_extent` rows /
    columns (its dims `rows_dim` / `cols_dim`) with the one above and the one to its left -- bf16 tensor arithmetic IN PLACE
    on the later tile exactly as :384-399, the earlier tile having been blended itself -- and cropped to `limit`."""
    rows = [[run(t[:, :, i:i + tile, j:j + tile]) for j in range(0, t.shape[-1], stride)] for i in range(0, t.shape[-2], stride)]
    crop = [slice(None)] * rows[0][0].dim()
    crop[rows_dim] = crop[cols_dim] = slice(limit)
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, out in enumerate(row):
            if i > 0:
                out = _blend(rows[i - 1][j], out, blend_extent, rows_dim)
            if j > 0:
                out = _blend(row[j - 1], out, blend_extent, cols_dim)
            result_row.append(out[tuple(crop)])
        result_rows.append(torch.cat(result_row, dim=cols_dim))
    return torch.cat(result_rows, dim=rows_dim)
