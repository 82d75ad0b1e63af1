"""What the inference-only transformer encoders share on the host: clip_vision.py, clip_text.py, t5.py and image_reward.py.
Each of those keeps what is its own -- the configuration, the `param_shapes` / `*_names` tables, its entry points -- and takes
from here
    read_checkpoint_dir   `config.json` + every `*.safetensors` file of a directory
    convert_names         a checkpoint's state dict -> the internal layout, by a module's name table; one error report
    draw_state_dict       the loop behind every `synthetic_state_dict`; the module gives the distribution of a tensor
    EncoderHost           device, weights `P`, the buffer cache, placement (fp32 / bf16), the GEMM call of every Linear and
                          the pre-norm layer (norm, q | k | v, attention, out + residual, norm, fc1, activation, fc2 + residual).

Layout of every encoder: all samples of a call are one batch of M = B S token rows, bf16; every Linear is a launch of the
persistent GEMM (`ops.gemm`), residual sums ride the GEMM epilogue with a ones gate, as vae._attention does."""
import json
import os

import torch

from . import ops
from .ops import BF16, F32, Rows, EPI_BIAS_GATE_RES


def read_checkpoint_dir(path):
    """-> (`config.json` as a dict, the state dict of all `*.safetensors` files of the directory)"""
    from safetensors.torch import load_file
    with open(os.path.join(path, "config.json")) as f:
        raw = json.load(f)
    files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if not files:
        raise FileNotFoundError(f"no *.safetensors file in {path}")
    sd = {}
    for f in files:
        sd.update(load_file(os.path.join(path, f)))
    return raw, sd


def convert_names(sd, names, shapes, own, label, optional=(), fixups=None):
    """The internal dict of `names`: internal name -> the checkpoint's name, a tuple of names to concatenate along dim 0
    (q | k | v), or a list of alternatives of which the first present one is taken (T5's tied table).  Tensors keep their dtype;
    `fixups[name]` is applied to the (concatenated) tensor.  One ValueError, headed by `label`, names the tensors that are
    missing (unless `optional`), those under the prefixes `own` that the table does not know (`position_ids` buffers are
    ignored) and then those whose shape is not `shapes[name]`; keys outside `own` are ignored."""
    out, missing, used = {}, [], set()
    for name, src in names.items():
        if isinstance(src, list):
            have = [p for p in src if p in sd]
            used.update(have)
            parts, miss = tuple(have[:1]), ([] if have else src[:1])
        else:
            parts = src if isinstance(src, tuple) else (src,)
            miss = [p for p in parts if p not in sd]
        if miss:
            if name not in optional:
                missing += miss
            continue
        used.update(parts)
        t = torch.cat([sd[p] for p in parts], 0) if len(parts) > 1 else sd[parts[0]]
        out[name] = fixups[name](t) if fixups and name in fixups else t
    unknown = sorted(k for k in sd if k.startswith(tuple(own)) and k not in used and not k.endswith("position_ids"))
    if missing or unknown:
        raise ValueError(f"{label} state dict: missing {sorted(missing)[:8]} ({len(missing)}), unknown {unknown[:8]} ({len(unknown)})")
    source = lambda s: s if isinstance(s, str) else s[0] + " ..."
    bad = [f"{source(names[k])} -> {k} {tuple(out[k].shape)} != {shp}" for k, shp in shapes.items()
           if k in out and tuple(out[k].shape) != tuple(shp)]
    if bad:
        raise ValueError(f"{label} state dict: wrong shapes: {bad[:8]}")
    return out


def fan_in(shape):
    n = 1
    for v in shape[1:]:
        n *= v
    return n


def layer_norm_net_std(name, key, s):
    """The rule of the LayerNorm encoders for `draw_state_dict`: class token, positions and token tables 0.5; LayerNorm weights
    are gain vectors; biases 0.05; matrices by fan-in."""
    if name.rsplit(".", 1)[-1] in ("cls", "pos", "tok"):
        return 0.5
    if name.endswith("weight") and len(s) == 1:
        return None
    return 0.05 if name.endswith("bias") else fan_in(s) ** -0.5


def draw_state_dict(names, shapes, std, seed, device):
    """A random state dict in the checkpoint's names, drawn on `device` from one generator in the order of `names`, every value
    a bf16 number held in fp32.  `std(name, key, shape)` is the module's rule: the standard deviation of the normal draw, or
    None for a gain vector 1 + 0.1 N.  The parts of a tuple each get their share of dim 0; a list of alternatives is one tensor
    under every one of its names."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, src in names.items():
        shp = tuple(shapes[name])
        keys = src if isinstance(src, (tuple, list)) else (src,)
        s = (shp[0] // len(keys),) + shp[1:] if isinstance(src, tuple) else shp
        for key in keys:
            if isinstance(src, list) and keys[0] in sd:
                sd[key] = sd[keys[0]]
                continue
            sigma = std(name, key, s)
            n = torch.randn(s, generator=g, device=device)
            sd[key] = ((1.0 + 0.1 * n) if sigma is None else sigma * n).to(BF16).float()
    return sd


PRENORM_LINEARS = ("qkv", "out", "fc1", "fc2")


class EncoderHost:
    """The host side of one inference-only encoder: `P` (internal name -> tensor on the device), a cache of work buffers, and
    the launches every encoder makes the same way."""

    def __init__(self, device, width=None):
        self.device = torch.device(device)
        self.P = None
        self._buf = {}
        self._ones = None if width is None else torch.ones(max(width, 512), dtype=BF16, device=self.device)

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def _place(self, t):
        """A converted dict onto the device: LayerNorm parameters, class token and position embeddings stay fp32, everything
        else (matrices, biases, token tables: the GEMM's operands, the gather's rows) goes to bf16."""
        fp32 = lambda k: k in ("cls", "pos") or ".ln_" in k or k.startswith("ln_")
        return {k: v.to(self.device).to(F32 if fp32(k) else BF16).contiguous() for k, v in t.items()}

    def _plain(self, tag, M, C, dtype=BF16):
        key = (tag, M, C, dtype)
        t = self._buf.get(key)
        if t is None:
            t = self._buf[key] = torch.empty(M, C, dtype=dtype, device=self.device)
        return t

    def _layer_norm(self, x, name, y, M, D, eps, ldx=None):
        """nn.LayerNorm with P[name.weight], P[name.bias] over M rows of D, `ldx` (D if not given) elements apart in x"""
        ops.layer_norm_affine(x, ldx or D, self.P[name + ".weight"], self.P[name + ".bias"], y, D, M, D, eps)

    def _linear(self, a, name, out, residual=False):
        """out = a W^T + bias, or out += ... with `residual` (the sum rides the epilogue, with a ones gate); W = P[name.weight]
        is [N, K], a Linear without a `.bias` entry has none.  Without the GEMM's stream-K workspace, so that a sample's rows
        do not depend on how many samples share the call."""
        W = self.P[name + ".weight"]
        kw = dict(epi=EPI_BIAS_GATE_RES, gate=self._ones, gate_ld=0) if residual else {}
        ops.gemm(Rows.of(a), W, self.P.get(name + ".bias"), Rows.of(out), W.shape[0], W.shape[1], stream_k=False, **kw)

    def _prenorm_layer(self, L, x, n, qkv, o, h, norm, attend, act, linears=PRENORM_LINEARS):
        """One pre-norm transformer layer on the residual stream x, in place; n, qkv, o, h: work buffers.  `norm(src, name, dst)`
        is the layer's normalisation, `attend(qkv, o)` its attention (raises when the kernel refuses), `act(h)` applies the
        activation and returns the buffer that holds the result; `linears` names the four Linears under the prefix L."""
        q, out, fc1, fc2 = linears
        norm(x, L + "ln_1", n)
        self._linear(n, L + q, qkv)
        attend(qkv, o)
        self._linear(o, L + out, x, residual=True)
        norm(x, L + "ln_2", n)
        self._linear(n, L + fc1, h)
        self._linear(act(h), L + fc2, x, residual=True)
