"""CPU restatement of the FLUX VAE ENCODER -- test helper (imported by tests/test_vae_encoder_host.py and
tests/test_hip_vae_encoder.py, never by the product path), on the decoder oracle's building blocks and rounding points
(oracle/vae.py: `_conv`, `_gn`, `_resnet`, `_attention`, `rb`).

What it restates: `vae.encode(x).latent_dist` of diffusers' AutoencoderKL under bf16 autocast with bf16 weights.  PARITY UNPINNED,
like the decoder oracle: diffusers is not importable here.  The block order follows the reference lineage's 3-D encoder
(fastvideo/models/hunyuan/vae/vae.py Encoder.forward: conv_in, down blocks, mid block, GroupNorm, SiLU, conv_out; down block =
resnets then downsamplers, unet_causal_3d_blocks.py); the 2-D downsampler is diffusers' Downsample2D(padding=0), recollected:
`F.pad(x, (0, 1, 0, 1))` then `Conv2d(3, stride=2)` (the lineage's DownsampleCausal3D, :208, pads differently).  The Gaussian is
DiagonalGaussianDistribution (vae.py:321-353,384) as torch evaluates it on bf16 tensors; the tiling is `spatial_tiled_encode`
(autoencoder_kl_causal_3d.py:408-470) in 2-D on the decoder oracle's tile walk and `blend_v` / `blend_h` (pinned to the
reference's vendored 3-D lineage).
"""
import torch
import torch.nn.functional as F

from oracle import vae as OV

IN_CHANNELS = 3
BF16 = torch.bfloat16


def param_shapes(cfg):
    """diffusers key -> shape for the encoder half; block i in the forward order of `block_out_channels`."""
    ch = list(cfg.block_out_channels)
    out = {}
    OV.shape_conv(out, "encoder.conv_in", ch[0], IN_CHANNELS, 3)
    prev = ch[0]
    for i, co in enumerate(ch):
        for j in range(cfg.layers_per_block):
            OV.shape_resnet(out, f"encoder.down_blocks.{i}.resnets.{j}", prev if j == 0 else co, co)
        if i != len(ch) - 1:
            OV.shape_conv(out, f"encoder.down_blocks.{i}.downsamplers.0.conv", co, co, 3)
        prev = co
    OV.shape_mid_block(out, "encoder.mid_block", prev, cfg.mid_block_add_attention)
    OV.shape_norm(out, "encoder.conv_norm_out", prev)
    OV.shape_conv(out, "encoder.conv_out", 2 * cfg.latent_channels, prev, 3)
    return out


def init_params(cfg, seed=0):
    """Random bf16-valued parameters (fp32 tensors), the decoder oracle's scales."""
    return OV.draw_params(param_shapes(cfg), seed)


def downsample(P, name, x):
    x = F.pad(OV.rb(x), (0, 1, 0, 1))
    return OV.rb(F.conv2d(x, P[name + ".weight"], P[name + ".bias"], stride=2))


def encoder(P, cfg, x):
    """x [B, 3, H, W] fp32 -> moments [B, 2 latent_channels, H / f, W / f] (bf16 values in fp32)"""
    G = cfg.norm_num_groups
    n = len(cfg.block_out_channels)
    x = OV._conv(P, "encoder.conv_in", x, 1)
    for i in range(n):
        for j in range(cfg.layers_per_block):
            x = OV._resnet(P, f"encoder.down_blocks.{i}.resnets.{j}", x, G)
        if i != n - 1:
            x = downsample(P, f"encoder.down_blocks.{i}.downsamplers.0.conv", x)
    x = OV._resnet(P, "encoder.mid_block.resnets.0", x, G)
    if cfg.mid_block_add_attention:
        x = OV._attention(P, "encoder.mid_block.attentions.0", x, G)
    x = OV._resnet(P, "encoder.mid_block.resnets.1", x, G)
    x = F.silu(OV._gn(P, "encoder.conv_norm_out", x, G))
    return OV._conv(P, "encoder.conv_out", x, 1)


def gaussian(moments, noise=None):
    """bf16 moments [..., 2 Cz, h, w] -> (mean, std, sample) as torch gives them on bf16 tensors: every op rounds to bf16.
    std = bf16(exp(bf16(0.5 * clamp(logvar, -30, 20)))), sample = bf16(mean + bf16(std * noise)); no noise: the mode."""
    m = moments.to(BF16)
    mean, logvar = torch.chunk(m, 2, dim=-3)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    half = (0.5 * logvar.float()).to(BF16)
    std = torch.exp(half.float()).to(BF16)
    if noise is None:
        return mean, std, mean
    prod = (std.float() * noise.to(BF16).float()).to(BF16)
    return mean, std, (mean.float() + prod.float()).to(BF16)


def tiled_moments(P, cfg, x, encode_tile=None):
    """autoencoder_kl_causal_3d.py:408-462 in 2-D: image tiles, their bf16 moments blended in place on the later tile."""
    ts, tl, ov = OV.tile_sizes(cfg)
    blend_extent = int(tl * ov)
    return OV.tile_walk(x, ts, int(ts * (1 - ov)), blend_extent, tl - blend_extent, encode_tile or (lambda t: encoder(P, cfg, t)))


def encode_moments(P, cfg, x, use_tiling=False):
    ts = OV.tile_sizes(cfg)[0]
    if use_tiling and (x.shape[-1] > ts or x.shape[-2] > ts):
        return tiled_moments(P, cfg, x)
    return encoder(P, cfg, x).to(BF16)


def pack(z):
    """[B, C, h, w] -> [B, (h/2)(w/2), 4C] (train_grpo_flux.py:94-99)"""
    B, C, h, w = z.shape
    return z.view(B, C, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (h // 2) * (w // 2), C * 4)
