"""Backward pass of the HIP FLUX MMDiT with block-level activation recompute.

Replaces `loss.backward()` through diffusers' FluxTransformer2DModel under FSDP + full activation
checkpointing (reference fastvideo/train_grpo_flux.py:585, fastvideo/utils/fsdp_util.py:26-53): the forward
keeps only each block's input (bf16 [B, S, d]); the backward re-runs one block at a time with its
intermediates kept, then walks it in reverse.  Weight gradients accumulate in fp32 into the flat gradient
buffer (MGX_EPI_F32_ACC, beta = 1); activation gradients are bf16 like autograd's.

All arithmetic is in csrc/ kernels; this file only sequences them.
"""
import math
import os

import torch

from . import ops
from ._lib import MgxError
from .ops import BF16, F32, Rows, EPI_BIAS, EPI_DGELU, EPI_F32_ACC

KEEP_ACTS = os.environ.get("MGX_KEEP_ACTS", "1") != "0"
# How many blocks ALSO keep their FF / proj_mlp pre-activation ([M, 4d] bf16 per block: 0.79 GB at micro-batch 7), so that the
# recompute pass re-creates the activation with an elementwise GELU instead of re-running the d -> 4d GEMM (1/3 of a block's
# linear FLOPs).  An integer = that many leading blocks from the start; "auto" (default) = none until the trainer, at the
# start of its SECOND train step (the first one has shown the step's real peak), hands out what the device still has free
# beyond `KEEP_FF_RESERVE_GIB` (`FluxTransformer2DModel.grow_ff_keep`).  Values kept are the very values a recompute produces.
KEEP_FF = os.environ.get("MGX_KEEP_FF_BLOCKS", "auto")
KEEP_FF_RESERVE_GIB = float(os.environ.get("MGX_KEEP_FF_RESERVE_GIB", "12"))
# Likewise the fused QKV projection's output ([M, 3d] bf16 per block: 0.085 GB per sample): the recompute pass then skips the
# d -> 3d GEMM as well (1/4 of a block's linear FLOPs) and only re-runs the elementwise QK-RMSNorm + RoPE on the kept rows.
# "auto": handed out together with the FF pre-activations, block by block (FF first), from the memory that is still free.
# With both kept for every block the recompute pass runs NO GEMM at all (micro-batch 4 at FLUX.1-dev 1024^2 on 288 GB).
KEEP_QKV = os.environ.get("MGX_KEEP_QKV_BLOCKS", "auto")


def _pad64(n):
    return (n + 63) // 64 * 64


class _Train:
    """Extra buffers of the training pass for one (L, N) shape at a batch CAPACITY B (smaller micro-batches use
    leading slices: `view`)."""

    def __init__(self, cfg, w, device):
        d, H, hd = cfg.dim, cfg.num_attention_heads, cfg.attention_head_dim
        B, S, Sp = w.B, w.S, w.Sp
        self.B, self.S = B, S
        M = B * S
        e = lambda *shape, dtype=BF16: torch.empty(*shape, dtype=dtype, device=device)
        z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype, device=device)
        nblk = cfg.num_layers + cfg.num_single_layers
        self.block_in = e(nblk, B, S, d)          # block inputs: the recompute pass starts from these
        self.x_final = e(B, S, d)
        # Selective activation saving (288 GB HBM: no parameter sharding, so there is room): the attention output + LSE
        # and the pre-gate outputs of the projections that END a residual branch are kept per block (4 x 28 MB per
        # sample and double block, 2 x per single block), so the recompute pass skips attention and those GEMMs:
        # 5/12 of a block's linear FLOPs and all of its attention FLOPs.  MGX_KEEP_ACTS=0 restores full recompute.
        self.keep = None
        if KEEP_ACTS:
            self.keep = []
            for b in range(nblk):
                k = dict(O=e(B, S, d), lse=e(B, H, S, dtype=F32), y_attn=e(M, d))
                if b < cfg.num_layers:
                    k.update(y_ff=e(M, d), x_mid=e(B, S, d))
                self.keep.append(k)
            self._grow_shape, self._device = {"hid_pre": (M, 4 * d), "qkv": (M, 3 * d)}, device
            if KEEP_FF != "auto":
                self.grow_ff(int(KEEP_FF))
            if KEEP_QKV != "auto":
                self.grow_qkv(int(KEEP_QKV))
        self.save = dict(nrm1=e(M, d), nrm2=e(M, d), y_attn=e(M, d), y_ff=e(M, d), hid_pre=e(M, 4 * d),
                         x_mid=e(B, S, d), V=e(B, H, S, hd), Qt=z(B, H, hd, Sp), Kt=z(B, H, hd, Sp))
        self.dX = e(B, S, d)
        self.dO = e(B, S, 5 * d)                  # dO [B,S,d] view for double blocks, d(cat) [B,S,5d] for single
        self.dQ, self.dK, self.dV = e(B, H, S, hd), e(B, H, S, hd), e(B, H, S, hd)
        self.dOt = z(B, H, hd, Sp)
        self.delta = e(B, H, S, dtype=F32)
        self.dy = e(M, d)
        self.dbig = e(M, 7 * d)                   # [dqkv | dmlp_pre] (single) / dqkv, dhid_pre (double)
        self.dnrm = e(M, d)
        Mp = _pad64(M)
        self.dCt = e(7 * d * Mp)                  # transposed output-gradient operand for wgrad
        self.At = e(5 * d * Mp)                   # transposed activation operand for wgrad
        self.Wt = e(7 * d * max(d, 64) + 5 * d * d)
        self.ones = torch.ones(1, 5 * d, dtype=BF16, device=device)

    def view(self, B):
        return self if B == self.B else _TrainView(self, B)

    def ff_kept(self):
        return sum(1 for k in (self.keep or []) if "hid_pre" in k)

    def qkv_kept(self):
        return sum(1 for k in (self.keep or []) if "qkv" in k)

    def _grow(self, blocks, names, budget_bytes=math.inf):
        """Allocate the keep buffers `names` ("hid_pre": the FF pre-activation, "qkv": the QKV projection's output) that
        `blocks` lack, block by block, while `budget_bytes` covers the next one.  Returns the bytes left."""
        for k in blocks:
            for name in (n for n in names if n not in k):
                size = math.prod(self._grow_shape[name]) * 2
                if budget_bytes < size:
                    return budget_bytes
                k[name] = torch.empty(*self._grow_shape[name], dtype=BF16, device=self._device)
                budget_bytes -= size
        return budget_bytes

    def grow_ff(self, n_total):
        """Keep the FF pre-activation of the first `n_total` blocks (allocates the missing buffers)."""
        self._grow((self.keep or [])[:max(0, n_total)], ("hid_pre",))
        return self.ff_kept()

    def grow_qkv(self, n_total):
        """Keep the QKV projection's output of the first `n_total` blocks (allocates the missing buffers)."""
        self._grow((self.keep or [])[:max(0, n_total)], ("qkv",))
        return self.qkv_kept()

    def grow_auto(self, budget_bytes):
        """Spend `budget_bytes` block by block, FF pre-activation before QKV output, on whatever is still recomputed and
        set to "auto".  Returns the bytes left."""
        auto = tuple(n for n, mode in (("hid_pre", KEEP_FF), ("qkv", KEEP_QKV)) if mode == "auto")
        return self._grow(self.keep or [], auto, budget_bytes)


class _TrainView:
    """The first B batches of a `_Train` (batch-major contiguous buffers: plain prefixes; flat operand buffers shared)."""

    def __init__(self, base, B):
        assert B <= base.B
        M = B * base.S
        self.B, self.S = B, base.S
        self.block_in = [base.block_in[i, :B] for i in range(base.block_in.shape[0])]
        self.x_final = base.x_final[:B]
        rows = ("nrm1", "nrm2", "y_attn", "y_ff", "hid_pre")
        self.save = {k: (v[:M] if k in rows else v[:B]) for k, v in base.save.items()}
        self.keep = None
        if base.keep is not None:
            self.keep = [{k: (v[:M] if k in ("y_attn", "y_ff", "hid_pre", "qkv") else v[:B]) for k, v in kb.items()}
                         for kb in base.keep]
        self.dX, self.dO, self.dQ, self.dK, self.dV, self.dOt, self.delta = (
            t[:B] for t in (base.dX, base.dO, base.dQ, base.dK, base.dV, base.dOt, base.delta))
        self.dy, self.dbig, self.dnrm = base.dy[:M], base.dbig[:M], base.dnrm[:M]
        self.dCt, self.At, self.Wt, self.ones = base.dCt, base.At, base.Wt, base.ones


class _BlockPlan:
    """One pass through one block: the tensor every role uses and which steps run.  Built here and nowhere else; the block
    functions (`flux._double_block` / `_single_block`) and `_backward` read it and choose no buffer themselves.

    The passes:  `_BlockPlan(w, double)` -- no-grad: nothing is kept, every step runs, scratch buffers of the workspace `w`;
    `tr` (a `_Train` / `_TrainView`) and `blk` -- the training forward into the block's keep buffers `tr.keep[blk]` (without
    keep buffers, MGX_KEEP_ACTS=0, it IS the no-grad pass); `recompute=True` -- the backward's recompute pass into `tr.save`:
    in full from the saved block input, or, with keep buffers, a replay that reads them back and skips what made them.

    Steps: `fused_qkv` (the no-grad projection with QK-norm / RoPE / V^T in its epilogue; otherwise `run_qkv` says whether
    the GEMM in front of `qk_norm_rope` runs), `run_attn`, `run_out` (the projections that END a residual branch: to_out and
    ff.net.2, proj_out), `run_ff` (ff.net.0 / proj_mlp).  `lean`: a single block's replay with the pre-activation kept builds
    no [O | mlp] operand -- the backward reads O from its keep buffer at row stride d and forms gelu(hid_pre) in a transpose.

    Roles: `restore` (block input to copy into the residual stream first, or None), `x_in` (input of the first LayerNorm),
    `nrm1` / `nrm2`, `qkv`, `V` / `Qt` / `Kt` (extra outputs of `qk_norm_rope` for the attention backward, or None), `O` and
    its row stride `ldo`, `lse`, `y_attn` and `hid_pre` (aux outputs of their GEMMs in the pass that runs them, what the
    backward reads after a recompute), for double blocks `y_ff` and `x_mid`, for single blocks `O_keep` (the keep buffer that
    `w.cat[:, :, :d]` is copied to by the forward and, unless lean, back from by the replay)."""

    def __init__(self, w, double, tr=None, blk=None, recompute=False):
        k = tr.keep[blk] if tr is not None and tr.keep else None
        s = tr.save if recompute else {}
        replay = recompute and k is not None
        has = lambda name: k is not None and name in k
        # a role's buffer: the block's keep buffer, else the recompute pass's save buffer, else the workspace's scratch (or none)
        pick = lambda name, scratch=None: k[name] if has(name) else s.get(name, scratch)
        d = w.X.shape[-1]
        self.fused_qkv = k is None and not recompute
        self.run_qkv = not (replay and has("qkv"))
        self.run_attn = self.run_out = not replay
        self.run_ff = not (replay and has("hid_pre"))
        self.lean = not double and not self.run_ff
        self.restore = tr.block_in[blk] if recompute and not replay else None
        self.x_in = tr.block_in[blk] if replay else w.X
        self.nrm1, self.nrm2 = s.get("nrm1", w.nrm), s.get("nrm2", w.nrm)
        self.qkv = pick("qkv", w.qkv)
        self.V, self.Qt, self.Kt = s.get("V"), s.get("Qt"), s.get("Kt")
        self.lse = pick("lse", w.lse if recompute else None)
        self.y_attn, self.hid_pre = pick("y_attn"), pick("hid_pre")
        if double:
            self.O, self.ldo = pick("O", w.O), d
            self.y_ff, self.x_mid = pick("y_ff"), pick("x_mid")
        else:
            self.O_keep = pick("O")
            self.O, self.ldo = (self.O_keep, d) if self.lean else (w.cat, 5 * d)


def _train_buffers(cfg, w, device):
    """`_Train` view for the workspace view `w`; the base grows to the largest training batch seen."""
    base = w.train
    if base is None or base.B < w.B:
        w.train = None
        del base
        torch.cuda.empty_cache()
        base = _Train(cfg, w, device)
        w.train = base
    return base.view(w.B)


def train_forward(model, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections, img_ids):
    """The training route's forward pass: every block into its keep buffers.  Returns (out, w, tr, saved, generation): the
    output and what a backward needs.  `FluxFunction.forward` is this plus the autograd context; a caller that wants the
    training route's kernels and no backward (`FluxTransformer2DModel.reference_policy`) drops everything but `out`."""
    cfg = model.cfg
    B, N, _ = hidden_states.shape
    L = encoder_hidden_states.shape[1]
    # ops.ATTN_PAD_KV: a sequence off 256 runs on the workspace of the next multiple, zero image rows appended, the rows
    # >= kv_len masked in the attention forward (model._attn) and backward (_attn_bwd); the workspace view of this call
    # carries kv_len, and serves the backward
    N_pad = model._pad_kv_rows_train(B, L, N)
    kv_len = None
    if N_pad is not None:
        hidden_states, img_ids = model._padded_inputs(hidden_states, img_ids, N_pad)
        kv_len = L + N
    w = model._workspace(B, L, N if N_pad is None else N_pad, kv_len=kv_len)
    tr = _train_buffers(cfg, w, model.store.device)
    ehs = model._embed(w, hidden_states, encoder_hidden_states)
    keep = {}
    temb, st = model._temb(B, timestep.to(model.store.device), guidance, pooled_projections, keep=keep)
    cos, sin = model._rope(txt_ids, img_ids)
    mods = []
    for blk in range(cfg.num_layers + cfg.num_single_layers):
        tr.block_in[blk].copy_(w.X)
        if blk < cfg.num_layers:
            mods.append(model._double_block(blk, w, st, cos, sin, _BlockPlan(w, True, tr, blk)))
        else:
            mods.append(model._single_block(blk - cfg.num_layers, w, st, cos, sin, _BlockPlan(w, False, tr, blk)))
    tr.x_final.copy_(w.X)
    out, e = model._head(w, st)
    model.last_train_route = "plain" if kv_len is None else "padded_kv"
    model.padded_kv_train_calls += int(kv_len is not None)
    # the saved activations live in the model's shared per-shape workspace: ONE pending backward per model at a time
    # (INTEGRATION.md).  A second grad-enabled forward before this one's backward would overwrite them: stamped here,
    # checked in backward.
    w.train.generation = getattr(w.train, "generation", 0) + 1
    saved = dict(ehs=ehs, in16=w.in16.clone(), temb=temb, st=st, keep=keep, cos=cos, sin=sin, mods=mods, e=e)
    return (out if kv_len is None else out[:, :N].contiguous()), w, tr, saved, w.train.generation


class FluxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat_param, model, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids,
                pooled_projections, img_ids):
        out, w, tr, saved, generation = train_forward(model, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids,
                                                      pooled_projections, img_ids)
        ctx.generation = generation
        ctx.model, ctx.w, ctx.tr = model, w, tr
        ctx.rows = hidden_states.shape[1]
        ctx.saved = saved
        return out

    @staticmethod
    def backward(ctx, dout):
        if getattr(ctx.w.train, "generation", None) != ctx.generation:
            raise MgxError("FluxTransformer2DModel: the activations of this forward pass were overwritten by a later "
                           "grad-enabled forward of the same model (one pending backward per model; call backward() "
                           "before the next training forward)")
        dout = dout.contiguous().to(BF16)
        if ctx.w.kv_len is not None:
            # padded: the padding tokens' rows of dout are zero, and stay zero in every gradient behind them
            dout, valid = dout.new_zeros(dout.shape[0], ctx.w.N, dout.shape[2]), dout
            dout[:, :ctx.rows] = valid
        _backward(ctx.model, ctx.w, ctx.tr, ctx.saved, dout)
        return (None,) * 9


# ------------------------------------------------------------------------------------------------ helpers
def _wgrad(model, tr, lin, A, dC: Rows):
    """g32[W] += dC^T A ; g32[b] += colsum(dC) for the `arch.Linear` `lin` (a fused one: all its members' rows at once).
    `A`: the [M, K] activation as `Rows`, or a list of column blocks `(Rows, width, gelu)` that make it up side by side --
    `gelu`: that block is gelu_tanh of the given (kept) pre-activation, applied on the way into the transposed operand.
    With adapters attached (model.lora): the rank-r gradients of the targets among `lin`'s members, nothing for frozen tensors."""
    if model.lora is not None:
        return _lora_wgrad(model, lin, A, dC)
    st, N, K = model.store, lin.N, lin.K
    g = st.ensure_grad()
    parts = A if isinstance(A, list) else [(A, K, False)]
    Mp = _pad64(parts[0][0].M)
    dCt = tr.dCt[:N * Mp].view(N, Mp)
    At = tr.At[:K * Mp].view(K, Mp)
    ops.transpose(dC, N, dCt, Mp, colsum_out=st.bias(g, lin), colsum_beta=1.0)
    k0 = 0
    for a_rows, width, gelu in parts:
        ops.transpose(a_rows, width, At[k0:k0 + width], Mp, gelu=gelu)
        k0 += width
    assert k0 == K
    ops.gemm(Rows.of(dCt), At, None, Rows(st.weight(g, lin), N, K), K, Mp, EPI_F32_ACC, beta=1.0, ldw=Mp)


def _lora_wgrad(model, lin, X, dC: Rows):
    """The low-rank branch of `_wgrad`: for every adapter target among `lin`'s members (the members of a fused projection
    are column slices of dC), with s = alpha / r:
        T = bf16(s X A^T) [M, r];  dT = bf16(s dC B) [M, r];  g[Bt] += T^T dC;  g[A] += dT^T X      (fp32 accumulation)
    The full dW is never formed; bias gradients are not computed (frozen)."""
    lo = model.lora
    members = lo.members(lin)
    if not members:
        return
    assert isinstance(X, Rows), "adapter targets take their input as one row-batched matrix"
    g = lo.ensure_grad()
    r, M, K = lo.rank, dC.M, lin.K
    T = ops.scratch("lora_T", M * r, BF16, lo.device)
    dT = ops.scratch("lora_dT", M * r, BF16, lo.device)
    flat = dC.t.reshape(-1)
    for module, col, n in members:
        A16, Bt16 = lo.view(lo.w16, f"{module}.lora_A"), lo.view(lo.w16, f"{module}.lora_Bt")
        dCm = Rows(flat[col:], M, dC.ld, dC.rpb, dC.bstride)
        ops.lora_proj(X, A16, T, K, r, lo.scale)
        ops.lora_proj(dCm, Bt16, dT, n, r, lo.scale)
        ops.lora_wgrad(T, dCm, lo.view(g, f"{module}.lora_Bt"), n, r, beta=1.0)
        ops.lora_wgrad(dT, X, lo.view(g, f"{module}.lora_A"), K, r, beta=1.0)


def _weight_t(model, tr, lin):
    """W^T [K, N] of `lin`'s bf16 weight, written into tr.Wt: the K-contiguous operand of the input-gradient GEMMs."""
    Wt = tr.Wt[:lin.K * lin.N].view(lin.K, lin.N)
    ops.transpose(Rows.of(model.store.weight(model.store.w16, lin)), lin.K, Wt, lin.N)
    return Wt


def _dgrad(model, tr, lin, dC: Rows, out: Rows, epi=EPI_BIAS, aux=None, ldaux=None, gate=None):
    """out[M, K] = epi(dC[M, N] @ W[N, K])."""
    ops.gemm(dC, _weight_t(model, tr, lin), None, out, lin.K, lin.N, epi, aux=aux, ldaux=ldaux, gate=gate, gate_ld=0)


def _attn_bwd(model, w, Q, K, V, Qt, Kt, O, dO, lse, tr, B, H, S, Sp, ldo, o_bstride, scale):
    """The attention backward of one block into tr.dQ / dK / dV.  On a padded workspace (w.kv_len set; every buffer allocated
    at S % 256 == 0) the masked-tail pair: rows >= kv_len contribute nothing and their dQ / dK / dV rows come back zero.
    With e4m3 attention and ops.ATTN_FP8_BWD the e4m3 backward (never padded: `_pad_kv_rows` keeps fp8 on the plain route)."""
    if ops.ATTN_FP8_BWD and model.attention_dtype == "fp8":
        ws, amax = w.fp8_bwd_workspace()
        ops.attn_bwd_fp8(Q, K, V, Qt, Kt, O, dO, lse, tr.delta, tr.dOt, tr.dQ, tr.dK, tr.dV, ws, amax, B, H, S, Sp, ldo, o_bstride,
                         scale)
        return
    if w.kv_len is None:
        ops.attn_bwd(Q, K, V, Qt, Kt, O, dO, lse, tr.delta, tr.dOt, tr.dQ, tr.dK, tr.dV, B, H, S, Sp, ldo, o_bstride, scale)
    elif not ops.attn_bwd_kv(Q, K, V, Qt, Kt, O, dO, lse, tr.delta, tr.dOt, tr.dQ, tr.dK, tr.dV, B, H, S, w.kv_len, ldo, o_bstride,
                             scale):
        raise MgxError(f"mgx_attn_bwd_kv refused B {B} H {H} Sa {S} kv_len {w.kv_len} after its path query took it")


def _skinny_bwd(model, tr, lin, dmod, x, dx_acc):
    """Modulation / embedder linear backward: g32[W] += dmod^T x, g32[b] += sum_b dmod, dx_acc += dmod @ W.  With adapters
    attached these weights are frozen: only the input-gradient half runs."""
    st = model.store
    if model.lora is None:
        g = st.ensure_grad()
        ops.skinny_wgrad(dmod, x, st.weight(g, lin), st.bias(g, lin), lin.N, lin.K)
    if dx_acc is not None:
        ops.skinny_dgrad(dmod, st.weight(st.w16, lin), dx_acc, lin.N, lin.K)      # straight from the row-major weight


def _backward(model, w, tr, sv, dout):
    cfg, arch = model.cfg, model.arch
    d, H = cfg.dim, cfg.num_attention_heads
    B, L, N, S, Sp = w.B, w.L, w.N, w.S, w.Sp
    M = B * S
    dev, store = model.store.device, model.store
    st_, cos, sin = sv["st"], sv["cos"], sv["sin"]
    scale, q_scale = model.attn_scale(), model.q_scale()   # (ln 2, scale * log2 e) for the prescaled Q of mgx_attn_fwd_log2
    if model.lora is None:
        g32 = store.ensure_grad()
        gnorm = lambda vec: store.view(g32, vec.name)
    else:
        # the RMSNorm weights are frozen; mgx_qk_norm_rope_bwd_qs still accumulates their gradients somewhere: a sink
        sink = torch.zeros(cfg.attention_head_dim, dtype=F32, device=dev)
        gnorm = lambda vec: sink
    dst = torch.zeros(B, d, dtype=BF16, device=dev)        # grad wrt st = silu(temb), summed over all users

    srows = lambda t, which, width: model._stream_rows(t, w, which, width)

    # ---------------- head: out = proj_out( LN(x_img) * (1+scale) + shift )
    e = sv["e"]
    nrm = tr.save["nrm1"][:B * N]
    ops.ln_modulate(srows(tr.x_final, "img", d), e[:, d:2 * d], e[:, 0:d], 2 * d, nrm, d)
    dC = Rows.of(dout.view(B * N, arch.proj_out.N))
    _wgrad(model, tr, arch.proj_out, Rows.of(nrm), dC)
    dn = tr.dnrm[:B * N]
    _dgrad(model, tr, arch.proj_out, dC, Rows.of(dn))
    tr.dX.zero_()
    de = torch.zeros(B, 2 * d, dtype=BF16, device=dev)
    ops.ln_modulate_bwd(dn, srows(tr.x_final, "img", d), e[:, 0:d], 2 * d, srows(tr.dX, "img", d), False,
                        de[:, d:2 * d], de[:, 0:d], d)
    _skinny_bwd(model, tr, arch.norm_out, de, st_, dst)

    # data-parallel overlap (dist_utils.GradReducer): set by the trainer for the LAST micro-batch before an optimizer step;
    # called with a block's prefix once every gradient of that block is final
    grad_ready = getattr(model, "_grad_ready", None) or (lambda prefix: None)
    grad_ready("tail")
    # ---------------- single blocks (reverse)
    for i in reversed(range(cfg.num_single_layers)):
        blk, sb = cfg.num_layers + i, arch.single[i]
        m = sv["mods"][blk]
        pl = _BlockPlan(w, False, tr, blk, recompute=True)
        model._single_block(i, w, st_, cos, sin, pl, mod_in=m)
        dmod = torch.empty(B, 3 * d, dtype=BF16, device=dev)
        x_in = Rows(tr.block_in[blk], M, d, S, S * d)
        dXr = Rows(tr.dX, M, d, S, S * d)
        # out = x + gate * y ; y = proj_out(cat)
        ops.gate_bwd(dXr, pl.y_attn, m[:, 2 * d:3 * d], 3 * d, tr.dy, dmod[:, 2 * d:3 * d], B, S, d)
        dyr = Rows.of(tr.dy)
        # lean (attention output AND the FF pre-activation kept): the recompute pass built no [O | mlp] operand -- the weight
        # gradient of proj_out takes O from its keep buffer and gelu(hid_pre) formed inside the transpose, and the attention
        # backward reads O / writes dO at row stride d instead of 5d
        a_op = [(Rows.of(pl.O.view(M, d)), d, False), (Rows.of(pl.hid_pre), 4 * d, True)] if pl.lean else Rows.of(pl.O.view(M, 5 * d))
        _wgrad(model, tr, sb.proj_out, a_op, dyr)
        dO = tr.dO.view(-1)[:M * pl.ldo].view(B, S, pl.ldo)    # d(cat) [B, S, 5d]; lean: dO alone, [B, S, d]
        dbig = tr.dbig                                         # [M, 7d] = [dq | dk | dv | dmlp_pre]
        # one transpose of proj_out, two GEMMs: d(cat)[:, :d] = dO (attention output grad) ; d(cat)[:, d:] -> through GELU -> dbig[:, 3d:]
        Wt = _weight_t(model, tr, sb.proj_out)
        ops.gemm(dyr, Wt[0:d], None, Rows.of(dO.view(M, pl.ldo)), d, d, EPI_BIAS)
        ops.gemm(dyr, Wt[d:5 * d], None, Rows(dbig[0, 3 * d:], M, 7 * d), 4 * d, d, EPI_DGELU, aux=pl.hid_pre, ldaux=4 * d)
        _attn_bwd(model, w, w.Q, w.K, pl.V, pl.Qt, pl.Kt, pl.O, dO, pl.lse, tr, B, H, S, Sp, pl.ldo, S * pl.ldo, scale)
        # qk norm / rope backward writes [dq|dk|dv] straight into columns 0..3d of the [M, 7d] staging matrix
        ops.qk_norm_rope_bwd(pl.qkv, model.W32(sb.norm_q.name), model.W32(sb.norm_k.name), cos, sin, tr.dQ, tr.dK, tr.dV, dbig,
                             gnorm(sb.norm_q), gnorm(sb.norm_k), B, H, S, Sp, S, 0, ld_dqkv=7 * d, q_scale=q_scale)
        dbr = Rows.of(dbig)
        _wgrad(model, tr, sb.qkv_mlp, Rows.of(pl.nrm1), dbr)
        _dgrad(model, tr, sb.qkv_mlp, dbr, Rows.of(tr.dnrm))
        ops.ln_modulate_bwd(tr.dnrm, x_in, m[:, d:2 * d], 3 * d, dXr, True, dmod[:, 0:d], dmod[:, d:2 * d], d)
        _skinny_bwd(model, tr, sb.norm, dmod, st_, dst)
        grad_ready(sb.prefix)

    # ---------------- double blocks (reverse)
    sl, rows, s0 = model._stream_spans(w)
    dO3 = tr.dO.view(-1)[:B * S * d].view(B, S, d)
    dh_all = tr.dbig.view(-1)[:M * 4 * d].view(M, 4 * d)
    dqkv_all = tr.dbig.view(-1)[:M * 3 * d].view(M, 3 * d)
    for i in reversed(range(cfg.num_layers)):
        streams = arch.double[i].streams
        mods = sv["mods"][i]
        pl = _BlockPlan(w, True, tr, i, recompute=True)
        model._double_block(i, w, st_, cos, sin, pl, mods_in=mods)
        dmods = {k: torch.empty(B, 6 * d, dtype=BF16, device=dev) for k in ("img", "txt")}
        dy = {s.name: Rows.of(tr.dy[sl[s.name]]) for s in streams}
        # ---- FF branch: out = x_mid + gate_mlp * ff2(gelu(ff1(LNmod(x_mid))))
        for s in streams:
            m, dm, rs = mods[s.name], dmods[s.name], sl[s.name]
            ops.gate_bwd(srows(tr.dX, s.name, d), pl.y_ff[rs], m[:, 5 * d:6 * d], 6 * d, tr.dy[rs], dm[:, 5 * d:6 * d], B,
                         rows[s.name], d)
            # (ff.net.0 not run again: the recompute pass formed no activation; gelu(hid_pre) is applied inside the transpose)
            a_op = Rows.of(w.hid[rs]) if pl.run_ff else [(Rows.of(pl.hid_pre[rs]), 4 * d, True)]
            _wgrad(model, tr, s.ff2, a_op, dy[s.name])
        for s in streams:
            _dgrad(model, tr, s.ff2, dy[s.name], Rows.of(dh_all[sl[s.name]]), epi=EPI_DGELU, aux=pl.hid_pre[sl[s.name]], ldaux=4 * d)
        for s in streams:
            _wgrad(model, tr, s.ff0, Rows.of(pl.nrm2[sl[s.name]]), Rows.of(dh_all[sl[s.name]]))
        for s in streams:
            _dgrad(model, tr, s.ff0, Rows.of(dh_all[sl[s.name]]), Rows.of(tr.dnrm[sl[s.name]]))
        for s in streams:
            m, dm, rs = mods[s.name], dmods[s.name], sl[s.name]
            dXs = srows(tr.dX, s.name, d)
            ops.ln_modulate_bwd(tr.dnrm[rs], srows(pl.x_mid, s.name, d), m[:, 4 * d:5 * d], 6 * d, dXs, True,
                                dm[:, 3 * d:4 * d], dm[:, 4 * d:5 * d], d)
            # ---- attention branch: x_mid = x_in + gate_msa * to_out(O)
            ops.gate_bwd(dXs, pl.y_attn[rs], m[:, 2 * d:3 * d], 6 * d, tr.dy[rs], dm[:, 2 * d:3 * d], B, rows[s.name], d)
            _wgrad(model, tr, s.out, srows(pl.O, s.name, d), dy[s.name])
        for s in streams:
            _dgrad(model, tr, s.out, dy[s.name], srows(dO3, s.name, d))
        _attn_bwd(model, w, w.Q, w.K, pl.V, pl.Qt, pl.Kt, pl.O, dO3, pl.lse, tr, B, H, S, Sp, d, S * d, scale)
        for s in streams:
            ops.qk_norm_rope_bwd(pl.qkv[sl[s.name]], model.W32(s.norm_q.name), model.W32(s.norm_k.name), cos, sin, tr.dQ, tr.dK,
                                 tr.dV, dqkv_all[sl[s.name]], gnorm(s.norm_q), gnorm(s.norm_k), B, H, S, Sp, rows[s.name],
                                 s0[s.name], q_scale=q_scale)
            _wgrad(model, tr, s.qkv, Rows.of(pl.nrm1[sl[s.name]]), Rows.of(dqkv_all[sl[s.name]]))
        for s in streams:
            _dgrad(model, tr, s.qkv, Rows.of(dqkv_all[sl[s.name]]), Rows.of(tr.dnrm[sl[s.name]]))
        for s in streams:
            m, dm = mods[s.name], dmods[s.name]
            ops.ln_modulate_bwd(tr.dnrm[sl[s.name]], srows(tr.block_in[i], s.name, d), m[:, d:2 * d], 6 * d,
                                srows(tr.dX, s.name, d), True, dm[:, 0:d], dm[:, d:2 * d], d)
            _skinny_bwd(model, tr, s.norm, dm, st_, dst)
        grad_ready(arch.double[i].prefix)

    # ---------------- embedders (inputs need no gradient)
    _wgrad(model, tr, arch.x_embedder, Rows.of(sv["in16"]), srows(tr.dX, "img", d))
    _wgrad(model, tr, arch.context_embedder, Rows.of(sv["ehs"].view(B * L, -1)), srows(tr.dX, "txt", d))

    # ---------------- temb path: st = silu(temb); temb = sum of three MLP outputs
    dtemb = torch.empty(B, d, dtype=BF16, device=dev)
    ops.ew(sv["temb"], dst, dtemb, 1)
    for name, linear_1, linear_2 in arch.embedders:
        x, h1, a1 = sv["keep"][name]
        da1 = torch.zeros(B, d, dtype=BF16, device=dev)
        _skinny_bwd(model, tr, linear_2, dtemb, a1, da1)
        dh1 = torch.empty(B, d, dtype=BF16, device=dev)
        ops.ew(h1, da1, dh1, 1)
        _skinny_bwd(model, tr, linear_1, dh1, x, None)
    if model.trainable_param.grad is None:
        model.trainable_param.grad = model.trainable_store.ensure_grad()
