"""Low-rank adapters (LoRA) on the flat parameter store: frozen fp32 base, trainable rank-r pairs, adapter files.

For a target Linear `y = x W0^T + b` the adapted layer is `y = x (W0 + s B A)^T + b`, A [r, K], B [N, r], s = alpha / r.
MERGED form: the forward, the recompute pass and the input gradient keep reading the bf16 compute copy `store.w16`, which
`LoraStore.merge` refreshes as bf16(W0 + s B A) from the fp32 masters -- ONE rounding of their sum (formed in fp64), as the full
fine-tune refreshes `w16` from `w32` with one rounding -- after attaching, loading and every optimizer step; `store.w32` stays the frozen base.  The
backward of a target forms only the rank-r gradients (flux_backward._lora_wgrad, csrc/lora.hip); the full dW, the fp32
gradient buffer of the base and every bias / norm / modulation gradient are never computed.

B is held transposed (`lora_Bt` [r, N]) so that both halves are "r rows x wide" and each kernel serves both.  `LoraStore` is
duck-typed like `flux.ParamStore` (w32 / w16 / g32 / numel / index / view / ensure_grad / block_ranges), so `FusedAdamW` and
`dist_utils.GradReducer` run on it unchanged in kind.
"""
import json
import math
import os
from typing import Dict, List, Tuple

import torch

from . import ops
from .ops import BF16, F32

# diffusers module names (suffixes) an adapter can sit on.  Not supported: `ff.net.2` / `ff_context.net.2` and the single
# blocks' `proj_out` (their inputs are not materialised in the lean replay of the backward), and the embedder / modulation /
# time-text linears (skinny: a handful of rows, nothing to gain from a low-rank path).
SUPPORTED_TARGETS = ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out",
                     "ff.net.0.proj", "ff_context.net.0.proj", "proj_mlp")
DEFAULT_TARGETS = ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out")
WEIGHTS_NAME = "pytorch_lora_weights.safetensors"
CONFIG_NAME = "lora_config.json"
KEY_PREFIX = "transformer."


def parse_target_modules(spec):
    """A comma list ("to_q,to_k") or a sequence of names -> tuple of names; None / "" -> the default (the eight attention
    projections).  Any name outside `SUPPORTED_TARGETS` raises a ValueError naming it.  Needs no model."""
    if spec is None or spec == "" or spec == ():
        return DEFAULT_TARGETS
    names = [s.strip() for s in spec.split(",")] if isinstance(spec, str) else list(spec)
    names = [n for n in names if n]
    for n in names:
        if n not in SUPPORTED_TARGETS:
            raise ValueError(f"LoRA target module {n!r} is not supported; choose from {', '.join(SUPPORTED_TARGETS)}")
    if not names:
        return DEFAULT_TARGETS
    return tuple(dict.fromkeys(names))


def resolve_targets(layout, target_modules) -> List[Tuple[str, int, int]]:
    """[(module, N, K)] of the Linears in `layout` (flux.param_layout: [(name, shape)]) that `target_modules` selects, in layout
    order.  A module matches a target when its diffusers name is the target or ends with "." + target (peft's rule): `to_q`
    selects the double blocks' and the single blocks' query projections alike."""
    targets = parse_target_modules(target_modules)
    out = []
    for name, shape in layout:
        if not name.endswith(".weight") or len(shape) != 2:
            continue
        module = name[:-len(".weight")]
        if any(module == t or module.endswith("." + t) for t in targets):
            out.append((module, shape[0], shape[1]))
    return out


def check_rank(rank):
    if rank not in ops.LORA_RANKS:
        raise ValueError(f"LoRA rank {rank} is not supported; choose from {ops.LORA_RANKS}")


class LoraStore:
    """Flat fp32 master of every adapter (+ bf16 mirror, fp32 gradient on demand), addressed as `<module>.lora_A` [r, K] and
    `<module>.lora_Bt` [r, N]."""

    ALIGN = 64

    def __init__(self, cfg, device, rank, alpha, target_modules=None, layout=None, allocate=True):
        from .flux import param_layout
        check_rank(rank)
        self.cfg = cfg
        self.device = torch.device(device)
        self.rank, self.alpha = int(rank), float(alpha)
        self.scale = self.alpha / self.rank
        self.target_modules = parse_target_modules(target_modules)
        self.layout = param_layout(cfg) if layout is None else layout
        self.targets = resolve_targets(self.layout, self.target_modules)
        if not self.targets:
            raise ValueError(f"LoRA target modules {self.target_modules} select no Linear of this model")
        for module, N, K in self.targets:
            if K % 64 or N % 64:
                raise ValueError(f"LoRA target {module}: [{N}, {K}] is not a multiple of 64 in both dimensions")
        self.index: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.by_module = {m: (N, K) for m, N, K in self.targets}
        off = 0
        for module, N, K in self.targets:
            for key, width in ((f"{module}.lora_A", K), (f"{module}.lora_Bt", N)):
                self.index[key] = (off, (self.rank, width))
                off += (self.rank * width + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = off
        self.g32 = None
        if allocate:
            self.w32 = torch.zeros(off, dtype=F32, device=self.device)
            self.w16 = torch.zeros(off, dtype=BF16, device=self.device)

    # -- ParamStore's surface -----------------------------------------------------------------------------------------
    def view(self, buf, name):
        off, shape = self.index[name]
        return buf[off:off + shape[0] * shape[1]].view(shape)

    def sync_bf16(self):
        self.w16.copy_(self.w32)

    def ensure_grad(self):
        if self.g32 is None:
            self.g32 = torch.zeros(self.numel, dtype=F32, device=self.device)
        return self.g32

    def block_ranges(self):
        """{block prefix: (lo, hi)} element ranges like `ParamStore.block_ranges`: one contiguous range per transformer block
        (empty for a block without targets, and for "head" / "tail": no adapter sits outside the blocks)."""
        cfg = self.cfg
        prefixes = [f"transformer_blocks.{i}" for i in range(cfg.num_layers)] + \
                   [f"single_transformer_blocks.{i}" for i in range(cfg.num_single_layers)]
        out, pos = {"head": (0, 0)}, 0
        keys = list(self.index)
        k = 0
        for p in prefixes:
            lo = pos
            while k < len(keys) and keys[k].startswith(p + "."):
                k += 1
                pos = self.index[keys[k]][0] if k < len(keys) else self.numel
            out[p] = (lo, pos)
        out["tail"] = (self.numel, self.numel)
        return out

    # -- adapters -----------------------------------------------------------------------------------------------------
    def init_adapters(self, seed=0):
        """peft's initialisation: A kaiming-uniform(a = sqrt 5), i.e. U(-1 / sqrt K, 1 / sqrt K); B zero.  Drawn on the device."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        self.w32.zero_()
        for module, N, K in self.targets:
            bound = math.sqrt(6.0 / ((1.0 + 5.0) * K))
            self.view(self.w32, f"{module}.lora_A").uniform_(-bound, bound, generator=g)
        self.sync_bf16()

    def members(self, lin):
        """The targets among the members of the `arch.Linear` a `_wgrad` call covers: [(module, first output column, N)]."""
        return [mem for mem in lin.members if mem[0] in self.by_module]

    def merge(self, store):
        """store.w16[target] = bf16(store.w32[target] + s Bt^T A) for every target (from the fp32 masters, summed in fp64, one rounding)."""
        for module, N, K in self.targets:
            ops.lora_merge(store.view(store.w32, f"{module}.weight"), self.view(self.w32, f"{module}.lora_Bt"),
                           self.view(self.w32, f"{module}.lora_A"), store.view(store.w16, f"{module}.weight"), N, K, self.rank,
                           self.scale)

    def unmerge(self, store):
        """store.w16[target] = bf16(store.w32[target]): the adapter-free compute copy, bit for bit."""
        for module, N, K in self.targets:
            store.view(store.w16, f"{module}.weight").copy_(store.view(store.w32, f"{module}.weight"))

    # -- adapter files ------------------------------------------------------------------------------------------------
    def key_shapes(self):
        """{state-dict key: shape}: `transformer.<module>.lora_A.weight` [r, K] and `.lora_B.weight` [N, r]."""
        out = {}
        for module, N, K in self.targets:
            out[f"{KEY_PREFIX}{module}.lora_A.weight"] = (self.rank, K)
            out[f"{KEY_PREFIX}{module}.lora_B.weight"] = (N, self.rank)
        return out

    def state_dict(self):
        out = {}
        for module, N, K in self.targets:
            out[f"{KEY_PREFIX}{module}.lora_A.weight"] = self.view(self.w32, f"{module}.lora_A")
            out[f"{KEY_PREFIX}{module}.lora_B.weight"] = self.view(self.w32, f"{module}.lora_Bt").t()
        return out

    def load_state_dict(self, sd):
        want = self.key_shapes()
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"LoRA state dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        for module, N, K in self.targets:
            a, b = sd[f"{KEY_PREFIX}{module}.lora_A.weight"], sd[f"{KEY_PREFIX}{module}.lora_B.weight"]
            if tuple(a.shape) != (self.rank, K) or tuple(b.shape) != (N, self.rank):
                raise RuntimeError(f"LoRA state dict: {module} has A {tuple(a.shape)} B {tuple(b.shape)}, expected "
                                   f"{(self.rank, K)} and {(N, self.rank)}")
            self.view(self.w32, f"{module}.lora_A").copy_(a.to(device=self.device, dtype=F32))
            self.view(self.w32, f"{module}.lora_Bt").copy_(b.to(device=self.device, dtype=F32).t())
        self.sync_bf16()

    def config(self, step=0):
        return lora_config(self.rank, self.alpha, self.target_modules, step)


def lora_config(rank, alpha, target_modules, step=0):
    """The dict `lora_config.json` holds (the reference's fastvideo/utils/checkpoint.py:287-297)."""
    return {"step": int(step), "lora_params": {"lora_rank": int(rank), "lora_alpha": float(alpha),
                                               "target_modules": list(parse_target_modules(target_modules))}}


def write_lora_config(save_dir, config):
    os.makedirs(save_dir, exist_ok=True)
    tmp = os.path.join(save_dir, CONFIG_NAME + ".tmp")
    with open(tmp, "w") as f:
        json.dump(config, f, indent=4)
    os.replace(tmp, os.path.join(save_dir, CONFIG_NAME))


def read_lora_config(save_dir):
    """(rank, alpha, target_modules, step) of an adapter directory."""
    with open(os.path.join(save_dir, CONFIG_NAME)) as f:
        c = json.load(f)
    p = c["lora_params"]
    check_rank(int(p["lora_rank"]))
    return int(p["lora_rank"]), float(p["lora_alpha"]), parse_target_modules(p["target_modules"]), int(c.get("step", 0))


def is_lora_dir(path):
    return bool(path) and os.path.exists(os.path.join(path, CONFIG_NAME)) and os.path.exists(os.path.join(path, WEIGHTS_NAME))
