"""The FLUX MMDiT described once, as plain data: every Linear with its shape and its place in the flat parameter buffers.

`describe(cfg)` is the one place that spells the diffusers parameter names.  The flat layout (`flux.param_layout`: names,
shapes, order -- checkpoints, optimizer state and the DP buckets depend on it), the forward, the backward and the LoRA store
all read it.  It holds element offsets, not tensors (`ParamStore.weight / bias(buf, lin)` make the views): importable without
a GPU, and nothing to invalidate when a gradient buffer comes or goes.
"""
import math
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, NamedTuple, Tuple

ALIGN = 64          # every tensor starts at a multiple of this many elements


@dataclass(frozen=True)
class Linear:
    """y = x W^T + b, W [N, K] at element `w_off` and b [N] at `b_off` of the flat buffers.  `module`: the diffusers name of
    its first member; `members`: (module, first output row, rows) of each diffusers Linear it spans -- one for a plain
    Linear, several for a fused projection, whose members' weights (and biases) are adjacent in the buffers."""
    module: str
    N: int
    K: int
    w_off: int
    b_off: int
    members: Tuple[Tuple[str, int, int], ...]

    def rows(self, lo, hi):
        """The Linear of output rows [lo, hi), which must fall on member boundaries."""
        inside = tuple((m, r0 - lo, n) for m, r0, n in self.members if lo <= r0 < hi)
        if not inside or inside[0][1] != 0 or inside[-1][1] + inside[-1][2] != hi - lo:
            raise ValueError(f"{self.module}: rows [{lo}, {hi}) are not on member boundaries {self.members}")
        return Linear(inside[0][0], hi - lo, self.K, self.w_off + lo * self.K, self.b_off + lo, inside)


Vec = namedtuple("Vec", "name off n")          # a parameter vector (an RMSNorm weight): name, element offset, length


class Stream(NamedTuple):
    """One stream ("txt" / "img") of a double block: AdaLN modulation, fused q | k | v, QK-norm weights, attention output, FF."""
    name: str
    norm: Linear
    qkv: Linear
    norm_q: Vec
    norm_k: Vec
    out: Linear
    ff0: Linear
    ff2: Linear


# streams: (txt, img) -- text first, as its rows come first in the joint residual and in the scratch buffers
DoubleBlock = namedtuple("DoubleBlock", "prefix streams")


class SingleBlock(NamedTuple):
    """`qkv_mlp`: to_q | to_k | to_v | proj_mlp as the one [7d, d] operand of the backward GEMMs; `qkv` and `proj_mlp` are its
    row ranges."""
    prefix: str
    norm: Linear
    qkv_mlp: Linear
    qkv: Linear
    proj_mlp: Linear
    proj_out: Linear
    norm_q: Vec
    norm_k: Vec


class Arch(NamedTuple):
    index: Dict[str, Tuple[int, Tuple[int, ...]]]       # name -> (element offset, shape), in flat order
    numel: int
    x_embedder: Linear
    context_embedder: Linear
    embedders: Tuple[Tuple[str, Linear, Linear], ...]   # (name, linear_1, linear_2) of timestep, (guidance,) text: temb is their sum
    double: Tuple[DoubleBlock, ...]
    single: Tuple[SingleBlock, ...]
    norm_out: Linear
    proj_out: Linear


def describe(cfg) -> Arch:
    d, hd = cfg.dim, cfg.attention_head_dim
    index, end = {}, 0

    def put(name, *shape):
        nonlocal end
        index[name] = (end, shape)
        end += (math.prod(shape) + ALIGN - 1) // ALIGN * ALIGN
        return index[name][0]

    def fused(members, K):
        """Weights of all members, then their biases: one Linear.  Adjacent means no alignment gap between members."""
        w = [put(f"{m}.weight", n, K) for m, n in members]
        b = [put(f"{m}.bias", n) for m, n in members]
        rows, r0 = [], 0
        for i, (m, n) in enumerate(members):
            assert w[i] == w[0] + r0 * K and b[i] == b[0] + r0, f"{m}: not contiguous with the members fused before it"
            rows.append((m, r0, n))
            r0 += n
        return Linear(members[0][0], r0, K, w[0], b[0], tuple(rows))

    def lin(module, N, K):
        return Linear(module, N, K, put(f"{module}.weight", N, K), put(f"{module}.bias", N), ((module, 0, N),))

    def vec(name, n):
        return Vec(name, put(name, n), n)

    x_embedder = lin("x_embedder", d, cfg.in_channels)
    context_embedder = lin("context_embedder", d, cfg.joint_attention_dim)
    names = ["timestep_embedder"] + (["guidance_embedder"] if cfg.guidance_embeds else []) + ["text_embedder"]
    embedders = tuple((e, lin(f"time_text_embed.{e}.linear_1", d, cfg.pooled_projection_dim if e == "text_embedder" else 256),
                       lin(f"time_text_embed.{e}.linear_2", d, d)) for e in names)
    double = []
    for i in range(cfg.num_layers):
        p = f"transformer_blocks.{i}"
        norm = [lin(f"{p}.{n}.linear", 6 * d, d) for n in ("norm1", "norm1_context")]
        qkv = [fused([(f"{p}.attn.{n}", d) for n in ns], d) for ns in (("to_q", "to_k", "to_v"), ("add_q_proj", "add_k_proj", "add_v_proj"))]
        out = [lin(f"{p}.attn.{n}", d, d) for n in ("to_out.0", "to_add_out")]
        nqk = [vec(f"{p}.attn.{n}.weight", hd) for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k")]
        ff = [(lin(f"{p}.{n}.net.0.proj", 4 * d, d), lin(f"{p}.{n}.net.2", d, 4 * d)) for n in ("ff", "ff_context")]
        img, txt = (Stream(s, norm[j], qkv[j], nqk[2 * j], nqk[2 * j + 1], out[j], *ff[j]) for j, s in enumerate(("img", "txt")))
        double.append(DoubleBlock(p, (txt, img)))
    single = []
    for i in range(cfg.num_single_layers):
        p = f"single_transformer_blocks.{i}"
        norm = lin(f"{p}.norm.linear", 3 * d, d)
        qkv_mlp = fused([(f"{p}.attn.to_q", d), (f"{p}.attn.to_k", d), (f"{p}.attn.to_v", d), (f"{p}.proj_mlp", 4 * d)], d)
        proj_out = lin(f"{p}.proj_out", d, 5 * d)
        single.append(SingleBlock(p, norm, qkv_mlp, qkv_mlp.rows(0, 3 * d), qkv_mlp.rows(3 * d, 7 * d), proj_out,
                                  vec(f"{p}.attn.norm_q.weight", hd), vec(f"{p}.attn.norm_k.weight", hd)))
    norm_out = lin("norm_out.linear", 2 * d, d)
    proj_out = lin("proj_out", cfg.patch_size * cfg.patch_size * cfg.in_channels, d)
    return Arch(index, end, x_embedder, context_embedder, embedders, tuple(double), tuple(single), norm_out, proj_out)

