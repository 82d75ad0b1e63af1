"""The two halves of the VAE described once, as plain data: `layers(cfg, half)` is the ordered list of an AutoencoderKL
decoder's or encoder's layers -- kind, diffusers name, channels in and out -- and the one place that spells the diffusers
parameter names and knows how channels run through the blocks.  The key -> shape inventory (`param_shapes`: what a state dict
must hold, and the order `init_synthetic` draws in) and the launch walk of mixgrpo_amd/vae.py both read it.  No torch:
importable without a GPU, like mixgrpo_amd/arch.py.
"""
from collections import namedtuple

HALVES = ("decoder", "encoder")
ATTENTION_LINEARS = ("to_q", "to_k", "to_v", "to_out.0")

# kind: conv_in | resnet | attention | upsample | downsample | norm_out | conv_out; name: the diffusers prefix of its tensors
Layer = namedtuple("Layer", "kind name cin cout")


def layers(cfg, half):
    """The layers of `half` in forward order.  Decoder: conv_in, mid block, up blocks over the reversed `block_out_channels`
    (layers_per_block + 1 resnets each, an upsampler behind all but the last), norm, conv_out; encoder: conv_in, down blocks
    (layers_per_block resnets, a downsampler behind all but the last), mid block, norm, conv_out onto the moments."""
    dec = half == "decoder"
    ch = list(cfg.block_out_channels)[::-1 if dec else 1]
    blocks, resampler, kind = ("up_blocks", "upsamplers", "upsample") if dec else ("down_blocks", "downsamplers", "downsample")
    c_in, c_out = (cfg.latent_channels, cfg.out_channels) if dec else \
        (cfg.in_channels, (2 if cfg.double_z else 1) * cfg.latent_channels)

    def mid(c):
        m = half + ".mid_block"
        attention = [Layer("attention", m + ".attentions.0", c, c)] if cfg.mid_block_add_attention else []
        return [Layer("resnet", m + ".resnets.0", c, c)] + attention + [Layer("resnet", m + ".resnets.1", c, c)]

    body, prev = [], ch[0]
    for i, co in enumerate(ch):
        for j in range(cfg.layers_per_block + (1 if dec else 0)):
            body.append(Layer("resnet", f"{half}.{blocks}.{i}.resnets.{j}", prev if j == 0 else co, co))
        if i != len(ch) - 1:
            body.append(Layer(kind, f"{half}.{blocks}.{i}.{resampler}.0.conv", co, co))
        prev = co
    body = mid(ch[0]) + body if dec else body + mid(ch[-1])
    return [Layer("conv_in", half + ".conv_in", c_in, ch[0])] + body + \
        [Layer("norm_out", half + ".conv_norm_out", ch[-1], ch[-1]), Layer("conv_out", half + ".conv_out", ch[-1], c_out)]


def _wb(name, *w):
    return [(name + ".weight", w), (name + ".bias", w[:1])]


def _conv(name, ci, co, k=3):
    return _wb(name, co, ci, k, k)


# kind -> (name, cin, cout) -> its tensors as (key, shape), in state-dict order
_TENSORS = {
    "resnet": lambda n, ci, co: _wb(n + ".norm1", ci) + _conv(n + ".conv1", ci, co) + _wb(n + ".norm2", co) +
    _conv(n + ".conv2", co, co) + (_conv(n + ".conv_shortcut", ci, co, 1) if ci != co else []),
    "attention": lambda n, ci, co: _wb(n + ".group_norm", ci) + [t for m in ATTENTION_LINEARS for t in _wb(f"{n}.{m}", co, ci)],
    "norm_out": lambda n, ci, co: _wb(n, ci),
    **{kind: _conv for kind in ("conv_in", "upsample", "downsample", "conv_out")},
}


def param_shapes(cfg, half):
    """diffusers key -> shape of every tensor of `half`, in forward order of the layers"""
    return {k: s for l in layers(cfg, half) for k, s in _TENSORS[l.kind](l.name, l.cin, l.cout)}
