"""FLUX MMDiT on MI355X: drop-in for `diffusers.FluxTransformer2DModel` as the reference calls it
(fastvideo/utils/sampling_utils.py:68-82, fastvideo/train_grpo_flux.py:134-144,606,677-679).

Same call signature (kwargs), `.train()/.eval()/.parameters()/.state_dict()/.load_state_dict()/.config/
.clip_grad_norm_()`, diffusers state-dict key names.  All arithmetic runs in the hand-written HIP kernels of
csrc/ through the C ABI; this file is host orchestration: the flat parameter store, workspace reuse, the block
schedule and (for training) block-level activation recompute in the backward pass.

Precision policy = the reference's autocast(bf16) over fp32 master weights: bf16 compute copy of the weights,
fp32 MFMA accumulation, bf16 residual stream, fp32 norm statistics, fp32 gradients for weights.

Memory layout: ONE joint residual buffer X[B, S, d] (text rows first, S = L + N); the text / image streams of
the double blocks are row-batched views of it (no concat/split copies).  Parameters live in one flat fp32
buffer (+ a bf16 mirror with the identical element order) in which to_q|to_k|to_v are adjacent, so the fused
QKV projection is a view.
"""
import contextlib
import json
import math
import os
from dataclasses import asdict, dataclass
from typing import Dict, List, Tuple

import torch

from . import ops
from ._lib import MgxError
from .arch import describe
from .ops import BF16, F32, Rows, EPI_BIAS_GELU, EPI_BIAS_GATE_RES


@dataclass
class FluxConfig:
    patch_size: int = 1
    in_channels: int = 64
    num_layers: int = 19
    num_single_layers: int = 38
    attention_head_dim: int = 128
    num_attention_heads: int = 24
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 768
    guidance_embeds: bool = True
    axes_dims_rope: Tuple[int, int, int] = (16, 56, 56)

    @property
    def dim(self):
        return self.attention_head_dim * self.num_attention_heads

    def to_dict(self):
        d = asdict(self)
        d["axes_dims_rope"] = list(self.axes_dims_rope)
        d["_class_name"] = "FluxTransformer2DModel"
        return d


def param_layout(cfg: FluxConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """Flat order of the parameters (diffusers names), as `arch.describe` lays them out."""
    return [(name, shape) for name, (_, shape) in describe(cfg).index.items()]


class ParamStore:
    """Flat fp32 master + bf16 mirror (+ fp32 grad / Adam moments on demand), addressed by diffusers names."""

    def __init__(self, cfg: FluxConfig, device):
        self.cfg = cfg
        self.device = torch.device(device)
        self.arch = describe(cfg)
        self.index, self.numel = self.arch.index, self.arch.numel       # {name: (element offset, shape)} in flat order
        self.w32 = torch.zeros(self.numel, dtype=F32, device=self.device)
        self.w16 = torch.zeros(self.numel, dtype=BF16, device=self.device)
        self.g32 = None

    def view(self, buf, name):
        off, shape = self.index[name]
        return buf[off:off + math.prod(shape)].view(shape)

    def weight(self, buf, lin):
        """The [N, K] weight of an `arch.Linear` (a fused one: its members' rows, adjacent in the buffer) in flat buffer `buf`."""
        return buf[lin.w_off:lin.w_off + lin.N * lin.K].view(lin.N, lin.K)

    def bias(self, buf, lin):
        return buf[lin.b_off:lin.b_off + lin.N]

    def block_ranges(self):
        """{block prefix: (lo, hi)} element ranges of the flat buffers, in layout order (transformer blocks; everything
        before / after them under "head" / "tail").  Contiguous and 64-aligned: the buckets of the DP gradient reduction."""
        a = self.arch       # (a block's first tensor is its AdaLN modulation; the double blocks' image stream's comes first)
        starts = [("head", 0)] + [(b.prefix, b.streams[1].norm.w_off) for b in a.double] + \
                 [(b.prefix, b.norm.w_off) for b in a.single] + [("tail", a.norm_out.w_off), (None, self.numel)]
        return {k: (lo, hi) for (k, lo), (_, hi) in zip(starts, starts[1:])}

    def sync_bf16(self):
        self.w16.copy_(self.w32)

    def ensure_grad(self):
        if self.g32 is None:
            self.g32 = torch.zeros(self.numel, dtype=F32, device=self.device)
        return self.g32

    def init_synthetic(self, seed=0, std=0.02, bias_std=0.0):
        """Random-init weights of the right architecture (no checkpoints offline): N(0, std^2) matrices, zero (or
        N(0, bias_std^2)) biases, RMSNorm weights 1.  Generated on the device, tensor by tensor."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        for name, (off, shape) in self.index.items():
            v = self.view(self.w32, name)
            if name.endswith(".bias"):
                if bias_std > 0:
                    v.normal_(0.0, bias_std, generator=g)
                else:
                    v.zero_()
            elif len(shape) == 1:
                v.fill_(1.0)
                if bias_std > 0:
                    v.add_(torch.randn(shape, generator=g, device=self.device) * bias_std)
            else:
                v.normal_(0.0, std, generator=g)
        self.sync_bf16()


def rope_tables(ids, axes_dims, theta=10000.0):
    """FluxPosEmbed tables [S, head_dim] fp32 (angles in fp64), computed once per id set on the device."""
    cos, sin = [], []
    pos = ids.float()
    for a, dim in enumerate(axes_dims):
        fr = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64, device=ids.device) / dim))
        ang = torch.outer(pos[:, a].double(), fr)
        cos.append(ang.cos().repeat_interleave(2, dim=1).float())
        sin.append(ang.sin().repeat_interleave(2, dim=1).float())
    return torch.cat(cos, -1).contiguous(), torch.cat(sin, -1).contiguous()


class _Work:
    """Activation workspace for one (L, N) problem shape at a batch CAPACITY B; calls with a smaller batch use leading
    slices of it (`view`), so the rollout (B = G), the shared first step (B = 1) and the replay micro-batches share one
    allocation instead of one per batch size."""

    kv_len = None     # a padded call (ops.ATTN_PAD_KV) works on a `_WorkView` that carries its kv_len: rows >= kv_len of S are padding

    def __init__(self, cfg, B, L, N, device):
        d, H, hd = cfg.dim, cfg.num_attention_heads, cfg.attention_head_dim
        S = L + N
        self.B, self.L, self.N, self.S = B, L, N, S
        self.Sp = (S + 63) // 64 * 64
        e = lambda *shape, dtype=BF16: torch.empty(*shape, dtype=dtype, device=device)
        self.X = e(B, S, d)
        self.nrm = e(B * S, d)
        self.qkv = e(B * S, 3 * d)
        self.Q = e(B, H, S, hd)
        self.K = e(B, H, S, hd)
        self.Vt = torch.zeros(B, H, hd, self.Sp, dtype=BF16, device=device)   # padding must stay finite
        self.O = e(B, S, d)
        self.hid = e(B * S, 4 * d)
        self.cat = e(B, S, 5 * d)
        self.in16 = e(B * N, cfg.in_channels)
        self.out = e(B, N, cfg.patch_size * cfg.patch_size * cfg.in_channels)
        self.lse = e(B, H, S, dtype=F32)
        self.train = None                         # flux_backward._Train, at its own batch capacity
        self._f8 = None                           # (Q8, K8, V8t, amax): allocated when attention_dtype == "fp8"
        self._f8_bwd = None                       # (workspace, amax) of the e4m3 attention backward (ops.ATTN_FP8_BWD)
        self._dims = (H, hd)

    def fp8_bwd_workspace(self):
        """Byte workspace and [4][B*H] amax table of `ops.attn_bwd_fp8`, once, at batch capacity (a smaller batch lays its
        sections out inside the same bytes)."""
        if self._f8_bwd is None:
            H, _ = self._dims
            dev = self.X.device
            self._f8_bwd = (torch.empty(ops.attn_bwd_fp8_workspace(self.B, H, self.S, self.Sp), dtype=torch.uint8, device=dev),
                            torch.empty(4 * self.B * H, dtype=F32, device=dev))
        return self._f8_bwd

    def fp8_operands(self):
        """e4m3 copies of Q, K and the key-permuted V^T plus the per-(batch, head) amax table, at batch capacity."""
        if self._f8 is None:
            H, hd = self._dims
            u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=self.X.device)
            self._f8 = (u8(self.B, H, self.S, hd), u8(self.B, H, self.S, hd), u8(self.B, H, hd, self.Sp),
                        torch.empty(3 * self.B * H, dtype=F32, device=self.X.device))
        return self._f8

    def view(self, B, kv_len=None):
        return self if B == self.B and kv_len is None else _WorkView(self, B, kv_len)


class _WorkView:
    """The first B batches of a `_Work` (all buffers are batch-major and contiguous, so these are plain prefixes), for one
    call: `kv_len` is that call's valid sequence length when it runs padded, and stays with the view (a training forward's
    view serves its backward)."""

    def __init__(self, base, B, kv_len=None):
        assert B <= base.B
        self.base, self.B, self.L, self.N, self.S, self.Sp, self.kv_len = base, B, base.L, base.N, base.S, base.Sp, kv_len
        M = B * base.S
        self.X, self.Q, self.K, self.Vt, self.O, self.cat = (t[:B] for t in (base.X, base.Q, base.K, base.Vt, base.O, base.cat))
        self.nrm, self.qkv, self.hid = base.nrm[:M], base.qkv[:M], base.hid[:M]
        self.in16, self.out, self.lse = base.in16[:B * base.N], base.out[:B], base.lse[:B]

    def fp8_operands(self):
        q8, k8, v8t, amax = self.base.fp8_operands()
        return q8[:self.B], k8[:self.B], v8t[:self.B], amax      # amax is laid out [3][B*H] for the CURRENT batch

    def fp8_bwd_workspace(self):
        return self.base.fp8_bwd_workspace()

    @property
    def train(self):
        return self.base.train

    @train.setter
    def train(self, v):
        self.base.train = v


class FluxTransformer2DModel(torch.nn.Module):
    """MI355X-native FLUX MMDiT.  `hipflux = FluxTransformer2DModel(FluxConfig(), device="cuda")`."""

    def __init__(self, config: FluxConfig = None, device="cuda", attention_dtype="bf16", **cfg_kwargs):
        super().__init__()
        if attention_dtype not in ("bf16", "fp8"):
            raise ValueError(f"attention_dtype {attention_dtype!r} is not supported (bf16 | fp8)")
        self.attention_dtype = attention_dtype    # "fp8": e4m3 MFMA attention forward (BASELINE.json configs[4])
        self.cfg = config or FluxConfig(**cfg_kwargs)
        self.config = self.cfg.to_dict()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise MgxError("FluxTransformer2DModel (mixgrpo_amd) runs on an MI355X only; there is no CPU path")
        self.store = ParamStore(self.cfg, dev)
        self.arch = self.store.arch               # arch.describe(cfg): every Linear's shape and place in the flat buffers
        # one flat fp32 parameter (what optimizers / clip_grad_norm_ see); named views via state_dict()
        self.flat_param = torch.nn.Parameter(self.store.w32, requires_grad=True)
        self._work: Dict[Tuple[int, int], _Work] = {}
        self._rope_cache = {}
        self.recompute = True
        self.last_route = None                    # of the last no-grad forward: "plain" | "padded_kv" (ops.ATTN_PAD_KV)
        self.padded_kv_calls = 0
        self.last_train_route = None              # of the last training forward (FluxFunction): "plain" | "padded_kv"
        self.padded_kv_train_calls = 0
        self.lora = None                          # lora.LoraStore once adapters are attached (add_lora / load_lora)
        self._reference_active = False            # inside `reference_policy()`
        self._reference_saved = None              # its side buffer: the merged targets while the base's are in `store.w16`
        self.last_ref_kl = None                   # the last train step's mean KL to the base policy (--kl_ref_coeff), else None

    # ------------------------------------------------------------------ low-rank adapters (lora.py)
    @property
    def trainable_store(self):
        """The store the optimizer, the gradient clipping and the DP reduction work on: the adapters' when attached, else
        the model's own."""
        return self.store if self.lora is None else self.lora

    @property
    def trainable_param(self):
        return self.flat_param if self.lora is None else self.lora_param

    def add_lora(self, rank=16, alpha=None, target_modules=None, seed=0):
        """Attach rank-`rank` adapters (scale alpha / rank; alpha defaults to rank) to the Linears `target_modules` selects
        (lora.SUPPORTED_TARGETS; default: the eight attention projections) and freeze everything else: the base weights
        `store.w32` stay as they are, only the adapters receive gradients and optimizer steps, and the base's fp32 gradient
        buffer is dropped.  A kaiming-uniform, B zero: every output bit is unchanged until the first step."""
        from .lora import LoraStore
        if self.lora is not None:
            raise MgxError("add_lora: adapters are already attached (unload_lora() first)")
        lo = LoraStore(self.cfg, self.store.device, rank, rank if alpha is None else alpha, target_modules)
        lo.init_adapters(seed)
        self._attach_lora(lo)
        return self

    def _attach_lora(self, lo):
        self.lora = lo
        self.lora_param = torch.nn.Parameter(lo.w32, requires_grad=True)
        self.flat_param.requires_grad_(False)
        self.flat_param.grad = None
        self.store.g32 = None
        self.config.update(lora_rank=lo.rank, lora_alpha=lo.alpha, lora_target_modules=list(lo.target_modules))
        lo.merge(self.store)

    def merge_lora(self):
        """Refresh the targets' bf16 compute copy from the frozen base and the current adapters (after every optimizer step)."""
        self.lora.merge(self.store)

    def unload_lora(self):
        """Detach the adapters: the targets' compute copy is the base's again (bit for bit) and the base trains as before."""
        if self.lora is None:
            return self
        self.lora.unmerge(self.store)
        self.lora = None
        self._reference_saved = None
        del self.lora_param
        for k in ("lora_rank", "lora_alpha", "lora_target_modules"):
            self.config.pop(k, None)
        self.flat_param.requires_grad_(True)
        return self

    @contextlib.contextmanager
    def reference_policy(self):
        """Inside: every forward is the adapter-free base policy's -- the targets' compute copy is bf16(W0), bit for bit what
        `unload_lora()` leaves -- and builds no graph.  It takes the route the policy's own forward would take: the training
        route's kernels (flux_backward.train_forward; the two routes do not agree in bits) when the model is in training
        mode with gradients enabled, else the no-grad route, so with B = 0 its output is the policy's bit for bit.
        Outside: `store.w16` is bit for bit what it was.

        How: the merged targets are saved into a side buffer (2 bytes per target weight, allocated on first use and kept:
        `reference_policy_bytes`), `LoraStore.unmerge` writes bf16(W0) over them, and the exit copies them back -- a copy,
        not a second `merge` ("LoRA path").  A training-route pass overwrites the saved activations
        of a pending backward of the same shape: run it BEFORE the policy's grad-enabled forward."""
        if self.lora is None:
            raise MgxError("reference_policy: no adapters attached (the model is its own reference)")
        if self._reference_active:
            raise MgxError("reference_policy: already inside one")
        lo, st = self.lora, self.store
        views = [st.view(st.w16, f"{module}.weight") for module, _, _ in lo.targets]
        total = sum(v.numel() for v in views)
        if self._reference_saved is None or self._reference_saved.numel() != total:
            self._reference_saved = torch.empty(total, dtype=BF16, device=st.device)
        saved = torch.split(self._reference_saved, [v.numel() for v in views])
        flat = [v.view(-1) for v in views]
        torch._foreach_copy_(list(saved), flat)                   # (one launch per group of tensors, not one per target)
        lo.unmerge(st)
        self._reference_active = True
        try:
            yield self
        finally:
            self._reference_active = False
            torch._foreach_copy_(flat, list(saved))

    @property
    def reference_policy_bytes(self):
        """Device bytes `reference_policy` holds for the saved merged targets (0 before its first use)."""
        return 0 if self._reference_saved is None else self._reference_saved.numel() * 2

    def lora_state_dict(self):
        """{`transformer.<module>.lora_A.weight` [r, K], `transformer.<module>.lora_B.weight` [N, r]}: fp32, the adapter
        naming of peft / diffusers' `save_lora_weights`.  Neither library is available to test against here: the key format
        is UNPINNED."""
        if self.lora is None:
            raise MgxError("lora_state_dict: no adapters attached")
        return self.lora.state_dict()

    def save_lora(self, save_dir, step=0):
        """`pytorch_lora_weights.safetensors` + `lora_config.json` (rank, alpha, target modules, step) into `save_dir`."""
        from safetensors.torch import save_file

        from .lora import WEIGHTS_NAME, write_lora_config
        os.makedirs(save_dir, exist_ok=True)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.lora_state_dict().items()}
        tmp = os.path.join(save_dir, WEIGHTS_NAME + ".tmp")
        save_file(sd, tmp)
        os.replace(tmp, os.path.join(save_dir, WEIGHTS_NAME))
        write_lora_config(save_dir, self.lora.config(step))

    def load_lora(self, load_dir):
        """Attach the adapters of a directory `save_lora` / `checkpoint.save_lora_checkpoint` wrote (replacing attached ones)
        and merge them into the compute copy."""
        from safetensors.torch import load_file

        from .lora import WEIGHTS_NAME, LoraStore, read_lora_config
        rank, alpha, targets, _ = read_lora_config(load_dir)
        self.unload_lora()
        lo = LoraStore(self.cfg, self.store.device, rank, alpha, targets)
        lo.load_state_dict(load_file(os.path.join(load_dir, WEIGHTS_NAME)))
        self._attach_lora(lo)
        return self

    # ------------------------------------------------------------------ parameters / checkpoints
    def state_dict(self, *args, **kwargs):
        return {k: self.store.view(self.store.w32, k) for k in self.store.index}

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self.store.index if k not in sd]
        unexpected = [k for k in sd if k not in self.store.index]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        with torch.no_grad():
            for k, v in sd.items():
                if k in self.store.index:
                    self.store.view(self.store.w32, k).copy_(v.to(F32))
        self.store.sync_bf16()
        if self.lora is not None:
            self.lora.merge(self.store)
        return missing, unexpected

    def init_synthetic(self, seed=0, std=0.02, bias_std=0.0):
        self.store.init_synthetic(seed, std, bias_std)
        return self

    def W(self, name):
        return self.store.view(self.store.w16, name)

    def W32(self, name):
        return self.store.view(self.store.w32, name)

    def Wb(self, lin):
        """(weight, bias) of an `arch.Linear` in the bf16 compute copy."""
        return self.store.weight(self.store.w16, lin), self.store.bias(self.store.w16, lin)

    def _linear(self, A, lin, C, epi=ops.EPI_BIAS, **kw):
        """C = epi(A @ W^T + b) of the `arch.Linear` `lin` (A, C: `Rows`)."""
        ops.gemm(A, *self.Wb(lin), C, lin.N, lin.K, epi, **kw)

    def clip_grad_norm_(self, max_norm):
        """Global L2 norm of the fp32 gradients, scaled in place like torch's clip_grad_norm_ (reference :606)."""
        g = self.trainable_store.ensure_grad()
        nsq = torch.zeros(1, dtype=F32, device=g.device)
        ops.sqnorm(g, nsq)
        total = nsq.sqrt()
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        g.mul_(coef)
        return total.squeeze(0)

    def grow_ff_keep(self, reserve_gib=None):
        """Spend the device memory that is still free (beyond a reserve) on kept FF pre-activations and QKV outputs, so that
        the training pass's recompute skips those blocks' d -> 4d / d -> 3d GEMMs (flux_backward.KEEP_FF / KEEP_QKV =
        "auto").  Called by `train_one_step` at the start of its second step, when the first has shown the step's real peak.
        Returns the number of blocks whose FF pre-activation is kept."""
        from . import flux_backward as FB
        if not FB.KEEP_ACTS or (FB.KEEP_FF != "auto" and FB.KEEP_QKV != "auto"):
            return self.ff_blocks_kept()
        reserve = (FB.KEEP_FF_RESERVE_GIB if reserve_gib is None else reserve_gib) * 2.0 ** 30
        for base in self._work.values():
            tr = base.train
            if tr is None or tr.keep is None:
                continue
            free, _total = torch.cuda.mem_get_info(self.store.device)
            tr.grow_auto(int(free - reserve))
        return self.ff_blocks_kept()

    def ff_blocks_kept(self):
        return sum(b.train.ff_kept() for b in self._work.values() if b.train is not None and b.train.keep is not None)

    def qkv_blocks_kept(self):
        return sum(b.train.qkv_kept() for b in self._work.values() if b.train is not None and b.train.keep is not None)

    # ------------------------------------------------------------------ forward
    def _workspace(self, B, L, N, kv_len=None):
        """Workspace view for batch B of the (L, N) shape; the base grows to the largest batch seen.  `kv_len`: the call runs
        padded (ops.ATTN_PAD_KV) and its view says so to `_attn` / `_attn_bwd`; the base never does."""
        key = (L, N)
        base = self._work.get(key)
        if base is None or base.B < B:
            if base is not None:
                self._work.pop(key)
                del base
            elif len(self._work) >= 2:   # keep at most two sequence shapes resident
                self._work.pop(next(iter(self._work)))
            torch.cuda.empty_cache()     # hand the outgrown buffers back before allocating the larger ones
            base = _Work(self.cfg, B, L, N, self.store.device)
            self._work[key] = base
        return base.view(B, kv_len)

    def _attn(self, w, O, lse, ldo, o_bstride):
        """Joint attention of the current Q / K / Vt workspace into O (+ LSE).  `attention_dtype == "fp8"` (BASELINE.json
        configs[4]) quantises the operands per (batch, head) to e4m3 and runs both contractions on fp8 MFMA; every
        forward of the model (rollout, training forward) then uses it, the backward stays bf16."""
        H = self.cfg.num_attention_heads
        scale = self.attn_scale()
        if self.attention_dtype == "fp8":
            q8, k8, v8t, amax = w.fp8_operands()
            ops.attn_fp8_quantize(w.Q, w.K, w.Vt, q8, k8, v8t, amax, w.B, H, w.S, w.Sp)
            ops.attn_fwd_fp8(q8, k8, v8t, amax, O, lse, w.B, H, w.S, w.Sp, ldo, o_bstride, scale)
        elif ops.Q_PRESCALE and w.kv_len is not None:
            # padded forward (no-grad, training, recompute): every buffer is allocated at w.S (% 256 == 0), the image rows
            # >= kv_len are padding
            if not ops.attn_fwd_log2_kv(w.Q, w.K, w.Vt, O, lse, w.B, H, w.S, w.kv_len, ldo, o_bstride):
                raise MgxError(f"mgx_attn_fwd_log2_kv refused B {w.B} H {H} Sa {w.S} kv_len {w.kv_len} after its path query took it")
        elif ops.Q_PRESCALE:
            ops.attn_fwd_log2(w.Q, w.K, w.Vt, O, lse, w.B, H, w.S, w.Sp, ldo, o_bstride)
        else:
            ops.attn_fwd(w.Q, w.K, w.Vt, O, lse, w.B, H, w.S, w.Sp, ldo, o_bstride, scale)

    def _qkv_nograd(self, nrm, lin, qkv, w, rows, s0, wq, wk, cos, sin):
        """Fused q | k | v projection of one stream ([tokens, d] -> `qkv` [tokens, 3d]) + QK-norm / RoPE / head split for a
        forward that keeps nothing (the rollout).  When the persistent GEMM takes the shapes: the value projection is issued
        with the operand roles swapped and lands transposed in `w.Vt` [B, H, 128, Sp] at sequence offset `s0`
        (`mgx_linear_bf16_t`), and the q | k projection normalises, rotates and head-splits its tile in the epilogue
        (`mgx_linear_qk_norm_rope`: `qkv` is not touched at all).  Otherwise the plain projection(s) and the norm pass."""
        d, H = self.cfg.dim, self.cfg.num_attention_heads
        qk, v = lin.rows(0, 2 * d), lin.rows(2 * d, 3 * d)
        tokens = nrm.numel() // d
        B = tokens // rows
        vt = ops.LINEAR_VT and ops.linear_t(nrm, *self.Wb(v), w.Vt.view(-1)[s0:], tokens, d, d, w.Sp, rows, d * w.Sp)
        if vt and ops.LINEAR_QKNORM and H * 128 == d and ops.linear_qk_norm_rope(
                nrm, *self.Wb(qk), wq, wk, cos, sin, w.Q, w.K, B, H, w.S, rows, s0, d, q_scale=self.q_scale(),
                pairs=self._rope_pairs(cos, sin)):
            return
        if vt:
            self._linear(Rows.of(nrm), qk, Rows(qkv, tokens, 3 * d))
        else:
            self._linear(Rows.of(nrm), lin, Rows.of(qkv))
        ops.qk_norm_rope(qkv, wq, wk, cos, sin, w.Q, w.K, None if vt else w.Vt, B, H, w.S, w.Sp, rows, s0, q_scale=self.q_scale())

    def q_scale(self):
        """What `mgx_qk_norm_rope_fwd_qs` multiplies q by before its one bf16 rounding: softmax scale * log2(e) (the scores
        are exponents of two: mgx_attn_fwd_log2), or 1 under MGX_ATTN_Q_PRESCALE=0."""
        return ops.LOG2E / math.sqrt(self.cfg.attention_head_dim) if ops.Q_PRESCALE else 1.0

    def attn_scale(self):
        """The `scale` every other consumer of that Q takes (mgx_attn_bwd, mgx_attn_fwd_fp8): ln 2 for the prescaled Q."""
        return ops.LN2 if ops.Q_PRESCALE else 1.0 / math.sqrt(self.cfg.attention_head_dim)

    def _rope(self, txt_ids, img_ids):
        key = (id(txt_ids), txt_ids._version, tuple(txt_ids.shape), id(img_ids), img_ids._version, tuple(img_ids.shape))
        hit = self._rope_cache.get("k")
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        ids = torch.cat([txt_ids.float(), img_ids.float()], dim=0)
        cos, sin = rope_tables(ids, self.cfg.axes_dims_rope)
        self._rope_cache["k"] = (key, cos, sin, txt_ids, img_ids)   # keep the id tensors alive with the key
        return cos, sin

    def _rope_pairs(self, cos, sin):
        """[S, 64, 2] (cos, sin) per rotation pair for `mgx_linear_qk_norm_rope` when the tables repeat every pair's entry
        (FluxPosEmbed's do), else None; cached with the tables (MGX_ROPE_PAIR_TABLE=0: never)."""
        if not ops.ROPE_PAIR_TABLE:
            return None
        hit = self._rope_cache.get("pairs")
        if hit is None or hit[0] is not cos:
            hit = (cos, ops.rope_pair_table(cos, sin))
            self._rope_cache["pairs"] = hit
        return hit[1]

    def _temb(self, B, timestep, guidance, pooled, keep=None):
        """temb = t_emb + g_emb + text_emb (bf16 after every op), st = silu(temb)."""
        d = self.cfg.dim
        dev = self.store.device
        t = (timestep.to(BF16) * 1000).float().contiguous()          # `.to(hidden.dtype) * 1000` under autocast
        gd = guidance.to(dev)
        gd = (gd.to(BF16) * 1000).float()
        gd = gd.expand(B).contiguous() if gd.numel() == 1 else gd.contiguous()

        emb = {name: (l1, l2) for name, l1, l2 in self.arch.embedders}

        def mlp(name, x):
            l1, l2 = emb[name]
            h1 = torch.empty(B, d, dtype=BF16, device=dev)
            ops.skinny_linear(x, *self.Wb(l1), h1, d, l1.K)
            a1 = torch.empty_like(h1)
            ops.ew(h1, None, a1, 0)
            h2 = torch.empty_like(h1)
            ops.skinny_linear(a1, *self.Wb(l2), h2, d, d)
            if keep is not None:
                keep[name] = (x, h1, a1)
            return h2

        te = torch.empty(B, 256, dtype=BF16, device=dev)
        ops.sincos_embed(t, te)
        temb = mlp("timestep_embedder", te)
        if self.cfg.guidance_embeds:
            ge = torch.empty(B, 256, dtype=BF16, device=dev)
            ops.sincos_embed(gd, ge)
            gemb = mlp("guidance_embedder", ge)
            t2 = torch.empty_like(temb)
            ops.ew(temb, gemb, t2, 2)
            temb = t2
        pe = mlp("text_embedder", pooled.to(BF16).contiguous())
        t3 = torch.empty_like(temb)
        ops.ew(temb, pe, t3, 2)
        st = torch.empty_like(t3)
        ops.ew(t3, None, st, 0)
        return t3, st

    def _stream_rows(self, t, w, which, width):
        """Row-batched view of the text ('txt') or image ('img') rows of a joint [B, S, width] buffer."""
        if which == "txt":
            return Rows(t, w.B * w.L, width, w.L, w.S * width)
        return Rows(t[0, w.L:], w.B * w.N, width, w.N, w.S * width)

    def _stream_spans(self, w):
        """What the workspace view decides about the streams of a double block (`arch.Stream`), by stream name: its rows of the
        stacked scratch buffers (nrm / qkv / hid / kept activations; text first), its rows per batch, its first sequence row."""
        return ({"txt": slice(0, w.B * w.L), "img": slice(w.B * w.L, w.B * w.S)}, {"txt": w.L, "img": w.N}, {"txt": 0, "img": w.L})

    def _double_block(self, i, w, st, cos, sin, pl, mods_in=None):
        """One pass through double block `i` as its plan `pl` lays it out (flux_backward._BlockPlan: the buffer of every role
        and which steps run).  `mods_in`: the forward's modulations, for a recompute pass."""
        d, H = self.cfg.dim, self.cfg.num_attention_heads
        B, mods = w.B, {}
        streams = self.arch.double[i].streams
        sl, rows, s0 = self._stream_spans(w)
        Wb, W32, srows = self.Wb, self.W32, self._stream_rows
        if pl.restore is not None:
            w.X.copy_(pl.restore)                               # full recompute rewrites the residual stream
        for s in streams:
            if mods_in is not None:
                m = mods_in[s.name]
            else:
                m = torch.empty(B, 6 * d, dtype=BF16, device=self.store.device)
                ops.skinny_linear(st, *Wb(s.norm), m, 6 * d, d)
            mods[s.name] = m
            ops.ln_modulate(srows(pl.x_in, w, s.name, d), m[:, 0:d], m[:, d:2 * d], 6 * d, pl.nrm1[sl[s.name]], d)
        if pl.fused_qkv:
            # no-grad forward (the rollout): V^T straight from the value projection, QK-norm / RoPE in the q | k projection's epilogue
            for s in streams:
                self._qkv_nograd(pl.nrm1[sl[s.name]], s.qkv, pl.qkv[sl[s.name]], w, rows[s.name], s0[s.name],
                                 W32(s.norm_q.name), W32(s.norm_k.name), cos, sin)
        else:
            for s in (streams if pl.run_qkv else ()):        # the fused QKV projections
                self._linear(Rows.of(pl.nrm1[sl[s.name]]), s.qkv, Rows.of(pl.qkv[sl[s.name]]))
            for s in streams:
                ops.qk_norm_rope(pl.qkv[sl[s.name]], W32(s.norm_q.name), W32(s.norm_k.name), cos, sin, w.Q, w.K, w.Vt, B, H, w.S,
                                 w.Sp, rows[s.name], s0[s.name], V=pl.V, Qt=pl.Qt, Kt=pl.Kt, q_scale=self.q_scale())
        if pl.run_attn:
            self._attn(w, pl.O, pl.lse, d, w.S * d)
        part = lambda t, name: None if t is None else t[sl[name]]
        if pl.run_out:
            # attention output projections, both streams: x += gate_msa * (O @ W^T + b)
            for s in streams:
                self._linear(srows(pl.O, w, s.name, d), s.out, srows(w.X, w, s.name, d), EPI_BIAS_GATE_RES,
                             gate=mods[s.name][:, 2 * d:3 * d], gate_ld=6 * d, aux=part(pl.y_attn, s.name))
            if pl.x_mid is not None:
                pl.x_mid.copy_(w.X)
        x_mid = w.X if pl.run_out else pl.x_mid                  # replay: kept, the residual stream is not written
        for s in streams:
            m = mods[s.name]
            ops.ln_modulate(srows(x_mid, w, s.name, d), m[:, 3 * d:4 * d], m[:, 4 * d:5 * d], 6 * d, pl.nrm2[sl[s.name]], d)
        # (pre-activation kept: no GEMM in the replay, and no activation either -- its only reader in the backward, the weight
        # gradient of ff.net.2, applies GELU inside its operand transpose: flux_backward._wgrad)
        for s in (streams if pl.run_ff else ()):
            self._linear(Rows.of(pl.nrm2[sl[s.name]]), s.ff0, Rows.of(w.hid[sl[s.name]]), EPI_BIAS_GELU, aux=part(pl.hid_pre, s.name))
        for s in (streams if pl.run_out else ()):
            self._linear(Rows.of(w.hid[sl[s.name]]), s.ff2, srows(w.X, w, s.name, d), EPI_BIAS_GATE_RES,
                         gate=mods[s.name][:, 5 * d:6 * d], gate_ld=6 * d, aux=part(pl.y_ff, s.name))
        return mods

    def _single_block(self, i, w, st, cos, sin, pl, mod_in=None):
        """As `_double_block`.  [O | mlp] lives in `w.cat` at row stride 5d, except in a lean replay (`pl.lean`), which builds
        no such operand."""
        d, H = self.cfg.dim, self.cfg.num_attention_heads
        blk, Wb = self.arch.single[i], self.Wb
        B, S, M = w.B, w.S, w.B * w.S
        if pl.restore is not None:
            w.X.copy_(pl.restore)
        if mod_in is not None:
            m = mod_in
        else:
            m = torch.empty(B, 3 * d, dtype=BF16, device=self.store.device)
            ops.skinny_linear(st, *Wb(blk.norm), m, 3 * d, d)
        Xa = Rows(pl.x_in, M, d, S, S * d)
        ops.ln_modulate(Xa, m[:, 0:d], m[:, d:2 * d], 3 * d, pl.nrm1, d)
        wq, wk = self.W32(blk.norm_q.name), self.W32(blk.norm_k.name)
        if pl.fused_qkv:
            self._qkv_nograd(pl.nrm1, blk.qkv, pl.qkv, w, S, 0, wq, wk, cos, sin)
        elif pl.run_qkv:
            self._linear(Rows.of(pl.nrm1), blk.qkv, Rows.of(pl.qkv))
        cat2 = w.cat.view(M, 5 * d)
        if pl.run_ff:
            self._linear(Rows.of(pl.nrm1), blk.proj_mlp, Rows(cat2[0, d:], M, 5 * d), EPI_BIAS_GELU, aux=pl.hid_pre)
        if not pl.fused_qkv:
            ops.qk_norm_rope(pl.qkv, wq, wk, cos, sin, w.Q, w.K, w.Vt, B, H, S, w.Sp, S, 0, V=pl.V, Qt=pl.Qt, Kt=pl.Kt,
                             q_scale=self.q_scale())
        if pl.run_attn:
            self._attn(w, pl.O, pl.lse, pl.ldo, S * pl.ldo)
            if pl.O_keep is not None:
                pl.O_keep.copy_(w.cat[:, :, :d])
        elif not pl.lean:
            w.cat[:, :, :d].copy_(pl.O_keep)         # (the wgrad of proj_out then reads [O | mlp] as one [M, 5d] operand)
        if pl.run_out:
            self._linear(Rows.of(cat2), blk.proj_out, Xa, EPI_BIAS_GATE_RES, gate=m[:, 2 * d:3 * d], gate_ld=3 * d, aux=pl.y_attn)
        return m

    def _embed(self, w, hidden_states, encoder_hidden_states):
        d = self.cfg.dim
        B, N, L = w.B, w.N, w.L
        hs = hidden_states.detach()
        if hs.dtype == BF16:
            w.in16.copy_(hs.reshape(B * N, -1))
        else:
            ops.cast_bf16(hs.to(F32).contiguous().view(-1), w.in16.view(-1))
        self._linear(Rows.of(w.in16), self.arch.x_embedder, self._stream_rows(w.X, w, "img", d))
        ehs = encoder_hidden_states.detach().to(BF16).contiguous()
        self._linear(Rows.of(ehs.view(B * L, -1)), self.arch.context_embedder, self._stream_rows(w.X, w, "txt", d))
        return ehs

    def _head(self, w, st):
        d = self.cfg.dim
        B, N = w.B, w.N
        e = torch.empty(B, 2 * d, dtype=BF16, device=self.store.device)
        ops.skinny_linear(st, *self.Wb(self.arch.norm_out), e, 2 * d, d)
        nrm = w.nrm[:B * N]
        ops.ln_modulate(self._stream_rows(w.X, w, "img", d), e[:, d:2 * d], e[:, 0:d], 2 * d, nrm, d)   # scale first
        cout = self.arch.proj_out.N
        out = torch.empty(B, N, cout, dtype=BF16, device=self.store.device)
        self._linear(Rows.of(nrm), self.arch.proj_out, Rows.of(out.view(B * N, cout)))
        return out, e

    def forward(self, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections, img_ids,
                joint_attention_kwargs=None, return_dict=False):
        if self._reference_active and torch.is_grad_enabled() and self.training:
            from .flux_backward import train_forward
            with torch.no_grad():                  # the training route's kernels, nothing kept for a backward
                out = train_forward(self, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections,
                                    img_ids)[0]
            return (out,)
        if torch.is_grad_enabled() and self.training and self.trainable_param.requires_grad and not self._reference_active:
            from .flux_backward import FluxFunction
            out = FluxFunction.apply(self.trainable_param, self, hidden_states, encoder_hidden_states, timestep, guidance,
                                     txt_ids, pooled_projections, img_ids)
            return (out,)
        with torch.no_grad():
            out = self._forward_nograd(hidden_states, encoder_hidden_states, timestep, guidance, txt_ids,
                                       pooled_projections, img_ids)
        return (out,)

    def _pad_kv_rows(self, B, L, N):
        """Image rows of the padded no-grad forward (ops.ATTN_PAD_KV), or None for the plain one: a sequence off 256 is run
        at the next multiple of 256 with the added keys masked (`mgx_attn_fwd_log2_kv`), so that the 64-query attention
        forward and the fused q | k / V^T projections take it (720 x 720: 512 + 2025 = 2537 -> 2560, image rows 2048).
        The training path asks `_pad_kv_rows_train`, which also needs the masked backward to take the shape."""
        S = L + N
        if not ops.ATTN_PAD_KV or S % 256 == 0 or not ops.Q_PRESCALE or self.attention_dtype != "bf16":
            return None
        d, H = self.cfg.dim, self.cfg.num_attention_heads
        Sa = (S + 255) // 256 * 256
        # (ldo, batch stride) of the double blocks' O and of the single blocks' [O | mlp] operand
        if not all(ops.attn_fwd_kv_path(B, H, Sa, S, ld, Sa * ld) == 1 for ld in (d, 5 * d)):
            return None
        return Sa - L

    def _pad_kv_rows_train(self, B, L, N):
        """Image rows of the padded TRAINING forward / recompute / backward (flux_backward.FluxFunction), or None for the plain
        one: `_pad_kv_rows` and the masked attention backward (`mgx_attn_bwd_kv`) both take the shape.  The rollout and the
        replay of a sample then run the same kernels on the same padded shape."""
        N_pad = self._pad_kv_rows(B, L, N)
        if N_pad is None:
            return None
        d, H = self.cfg.dim, self.cfg.num_attention_heads
        Sa = L + N_pad
        # (ldo, batch stride) of dO / O: the double blocks and lean single blocks, the single blocks' d(cat)
        if not all(ops.attn_bwd_kv_path(B, H, Sa, L + N, ld, Sa * ld) == 1 for ld in (d, 5 * d)):
            return None
        return N_pad

    def _padded_inputs(self, hidden_states, img_ids, N_pad):
        """hidden_states [B, N, C] / img_ids [N, 3] with zero rows appended up to N_pad.  The padded ids are cached with the
        tensor they were made from, so that the RoPE tables (cached on their ids' identity) are not rebuilt every call."""
        B, N, C = hidden_states.shape
        hs = hidden_states.new_zeros(B, N_pad, C)
        hs[:, :N] = hidden_states
        key = (id(img_ids), img_ids._version, tuple(img_ids.shape), N_pad)
        hit = self._rope_cache.get("pad_ids")
        if hit is None or hit[0] != key:
            ids = torch.cat([img_ids, img_ids.new_zeros(N_pad - N, img_ids.shape[1])], dim=0)
            hit = (key, ids, img_ids)
            self._rope_cache["pad_ids"] = hit
        return hs, hit[1]

    def _forward_nograd(self, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections,
                        img_ids, collect=None):
        B, N, _ = hidden_states.shape
        L = encoder_hidden_states.shape[1]
        N_pad = self._pad_kv_rows(B, L, N) if collect is None else None
        if N_pad is not None:
            hs, ids = self._padded_inputs(hidden_states, img_ids, N_pad)
            out = self._forward_nograd_on(self._workspace(B, L, N_pad, kv_len=L + N), hs, encoder_hidden_states, timestep, guidance,
                                          txt_ids, pooled_projections, ids, None)
            self.last_route = "padded_kv"
            self.padded_kv_calls += 1
            return out[:, :N].contiguous()
        self.last_route = "plain"
        return self._forward_nograd_on(self._workspace(B, L, N), hidden_states, encoder_hidden_states, timestep, guidance, txt_ids,
                                       pooled_projections, img_ids, collect)

    def _forward_nograd_on(self, w, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections,
                           img_ids, collect):
        from .flux_backward import _BlockPlan
        B, L = w.B, w.L
        double, single = _BlockPlan(w, True), _BlockPlan(w, False)      # nothing is kept: one plan per block type
        self._embed(w, hidden_states, encoder_hidden_states)
        temb, st = self._temb(B, timestep.to(self.store.device), guidance, pooled_projections)
        cos, sin = self._rope(txt_ids, img_ids)
        if collect is not None:
            collect.update(temb=temb.clone(), x_embed=w.X[:, L:].clone(), ctx_embed=w.X[:, :L].clone())
        for i in range(self.cfg.num_layers):
            self._double_block(i, w, st, cos, sin, double)
            if collect is not None:
                collect[f"double{i}_h"] = w.X[:, L:].clone()
                collect[f"double{i}_c"] = w.X[:, :L].clone()
        for i in range(self.cfg.num_single_layers):
            self._single_block(i, w, st, cos, sin, single)
            if collect is not None:
                collect[f"single{i}_x"] = w.X.clone()
        out, _ = self._head(w, st)
        return out

    # ------------------------------------------------------------------ checkpoint format (reference checkpoint.py:65-88)
    def save_pretrained(self, save_dir):
        from safetensors.torch import save_file
        os.makedirs(save_dir, exist_ok=True)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        save_file(sd, os.path.join(save_dir, "diffusion_pytorch_model.safetensors"))
        cfg = dict(self.config)
        cfg.pop("dtype", None)
        with open(os.path.join(save_dir, "config.json"), "w") as f:
            json.dump(cfg, f, indent=4)

    @classmethod
    def from_pretrained(cls, path, device="cuda", subfolder=None, torch_dtype=None):
        """`FluxTransformer2DModel.from_pretrained(model_path, subfolder="transformer", torch_dtype=torch.float32)` as the
        reference calls it (train_grpo_flux.py:677-679): config.json + diffusers-named safetensors, single file or the
        sharded layout of the published FLUX.1-dev checkpoint (`...safetensors.index.json`).  Master weights are always
        fp32 (`torch_dtype` is accepted for the call signature)."""
        from safetensors.torch import load_file
        if subfolder and os.path.isdir(os.path.join(path, subfolder)):
            path = os.path.join(path, subfolder)
        with open(os.path.join(path, "config.json")) as f:
            raw = json.load(f)
        keys = {f.name for f in FluxConfig.__dataclass_fields__.values()}
        cfg = FluxConfig(**{k: (tuple(v) if k == "axes_dims_rope" else v) for k, v in raw.items() if k in keys})
        m = cls(cfg, device=device)
        index = os.path.join(path, "diffusion_pytorch_model.safetensors.index.json")
        if os.path.exists(index):
            with open(index) as f:
                shards = sorted(set(json.load(f)["weight_map"].values()))
            sd = {}
            for shard in shards:
                sd.update(load_file(os.path.join(path, shard)))
        else:
            sd = load_file(os.path.join(path, "diffusion_pytorch_model.safetensors"))
        m.load_state_dict(sd)
        return m
