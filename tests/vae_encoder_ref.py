"""CPU restatement of the FLUX VAE ENCODER -- test helper (imported by tests/test_vae_encoder_host.py and
tests/test_hip_vae_encoder.py, never by the product path), on the decoder oracle's building blocks and rounding points
(oracle/vae.py: `_conv`, `_gn`, `_resnet`, `_attention`, `rb`).

What it restates: `vae.encode(x).latent_dist` of diffusers' AutoencoderKL under bf16 autocast with bf16 weights.  PARITY UNPINNED,
like the decoder oracle: diffusers is not importable here.  The block order follows the reference lineage's 3-D encoder
(fastvideo/models/hunyuan/vae/vae.py Encoder.forward: conv_in, down blocks, mid block, GroupNorm, SiLU, conv_out; down block =
resnets then downsamplers, unet_causal_3d_blocks.py); the 2-D downsampler is diffusers' Downsample2D(padding=0), recollected:
`F.pad(x, (0, 1, 0, 1))` then `Conv2d(3, stride=2)` (the lineage's DownsampleCausal3D, :208, pads differently).  The Gaussian is
DiagonalGaussianDistribution (vae.py:321-353,384) as torch evaluates it on bf16 tensors; the tiling is `spatial_tiled_encode`
(autoencoder_kl_causal_3d.py:408-470) in 2-D with the decoder oracle's `blend_v` / `blend_h` (pinned to the reference).
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

    def conv(name, co, ci, k):
        out[name + ".weight"] = (co, ci, k, k)
        out[name + ".bias"] = (co,)

    def norm(name, c):
        out[name + ".weight"] = (c,)
        out[name + ".bias"] = (c,)

    def resnet(name, ci, co):
        norm(name + ".norm1", ci)
        conv(name + ".conv1", co, ci, 3)
        norm(name + ".norm2", co)
        conv(name + ".conv2", co, co, 3)
        if ci != co:
            conv(name + ".conv_shortcut", co, ci, 1)

    conv("encoder.conv_in", ch[0], IN_CHANNELS, 3)
    prev = ch[0]
    for i, co in enumerate(ch):
        for j in range(cfg.layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", prev if j == 0 else co, co)
        if i != len(ch) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", co, co, 3)
        prev = co
    resnet("encoder.mid_block.resnets.0", prev, prev)
    if cfg.mid_block_add_attention:
        a = "encoder.mid_block.attentions.0"
        norm(a + ".group_norm", prev)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            out[f"{a}.{n}.weight"] = (prev, prev)
            out[f"{a}.{n}.bias"] = (prev,)
    resnet("encoder.mid_block.resnets.1", prev, prev)
    norm("encoder.conv_norm_out", prev)
    conv("encoder.conv_out", 2 * cfg.latent_channels, prev, 3)
    return out


def init_params(cfg, seed=0):
    """Random bf16-valued parameters (fp32 tensors), the decoder oracle's scales."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in param_shapes(cfg).items():
        if k.endswith(".weight") and len(shp) == 1:
            P[k] = OV.rb(1.0 + 0.1 * torch.randn(shp, generator=g))
        elif k.endswith(".bias"):
            P[k] = OV.rb(0.05 * torch.randn(shp, generator=g))
        else:
            fan_in = shp[1] * (shp[2] * shp[3] if len(shp) == 4 else 1)
            P[k] = OV.rb(torch.randn(shp, generator=g) / fan_in ** 0.5)
    return P


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
    """autoencoder_kl_causal_3d.py:408-462 in 2-D: tiles are bf16 tensors, blended in place on the later tile."""
    ts, tl, ov = OV.tile_sizes(cfg)
    overlap_size = int(ts * (1 - ov))
    blend_extent = int(tl * ov)
    row_limit = tl - blend_extent
    enc = encode_tile or (lambda t: encoder(P, cfg, t))
    rows = []
    for i in range(0, x.shape[-2], overlap_size):
        row = []
        for j in range(0, x.shape[-1], overlap_size):
            row.append(enc(x[:, :, i:i + ts, j:j + ts]).to(BF16))
        rows.append(row)
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = OV.blend_v(rows[i - 1][j], tile, blend_extent)
            if j > 0:
                tile = OV.blend_h(row[j - 1], tile, blend_extent)
            result_row.append(tile[..., :row_limit, :row_limit])
        result_rows.append(torch.cat(result_row, dim=-1))
    return torch.cat(result_rows, dim=-2)


def encode_moments(P, cfg, x, use_tiling=False):
    ts = OV.tile_sizes(cfg)[0]
    if use_tiling and (x.shape[-1] > ts or x.shape[-2] > ts):
        return tiled_moments(P, cfg, x)
    return encoder(P, cfg, x).to(BF16)


def pack(z):
    """[B, C, h, w] -> [B, (h/2)(w/2), 4C] (train_grpo_flux.py:94-99)"""
    B, C, h, w = z.shape
    return z.view(B, C, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (h // 2) * (w // 2), C * 4)
