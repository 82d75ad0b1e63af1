"""Thin Python wrappers over the C-ABI MMDiT kernels (device tensors in, device tensors out, current stream).
Only plumbing lives here: shape bookkeeping and pointer passing.  See include/mixgrpo_hip.h for semantics."""
import os
from dataclasses import dataclass

import torch

from ._lib import check, lib, ptr, stream

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GATE_RES, EPI_F32_ACC, EPI_DGELU = 0, 1, 2, 3, 4
BF16 = torch.bfloat16
F32 = torch.float32


@dataclass
class Rows:
    """A row-batched bf16/fp32 matrix view: row m at data_ptr + (m // rpb) * bstride + (m % rpb) * ld elements."""
    t: torch.Tensor      # tensor whose data_ptr() is the first element
    M: int               # number of rows
    ld: int
    rpb: int = 1 << 40
    bstride: int = 0

    @staticmethod
    def of(t):
        """Plain 2-D view of a contiguous tensor [..., cols]."""
        cols = t.shape[-1]
        return Rows(t, t.numel() // cols, cols)


def gemm(A: Rows, W, bias, C: Rows, N, K, epi=EPI_BIAS, gate=None, gate_ld=0, aux=None, beta=0.0, ldw=None, ldaux=None,
         stream_k=None):
    """C = epi(A @ W[N,K]^T + bias).  `aux`: plain [M, ldaux] matrix (ldaux defaults to N); pass a tensor whose
    data_ptr() is its first element.  `stream_k`: None = the module's GEMM_STREAM_K; False = no stream-K workspace, every tile
    computed whole, so a row's result does not depend on how many rows the call has."""
    assert A.M == C.M
    _profiled(_gemm_launch, (A, W, bias, C, N, K, epi, gate, gate_ld, aux, beta, ldw, ldaux, stream_k), 2.0 * A.M * N * K,
              (A.M, N, K, epi))


GEMM_PROFILE = None


def _profiled(launch, args, flops, shape):
    """`launch(*args)`, and while bench.py holds a list in GEMM_PROFILE: HIP events around it on the launch stream, appended as
    (e0, e1, flops, (M, N, K, epi)).  A refused launch (`_try` said False) appends nothing."""
    if GEMM_PROFILE is None:
        return launch(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    took = launch(*args)
    if took is not False:
        e1.record()
        GEMM_PROFILE.append((e0, e1, flops, shape))
    return took


def _try(entry, *args):
    """Call an entry point that may refuse its problem: False for rc 1 (refused, nothing launched), True after a launch; any
    other code raises."""
    rc = entry(*args)
    if rc == 1:
        return False
    check(rc)
    return True

# MGX_LINEAR_VT=0: the value projection always leaves row-major and mgx_qk_norm_rope_fwd transposes it (the training passes
# do that anyway: their backward needs V row-major as well)
LINEAR_VT = os.environ.get("MGX_LINEAR_VT", "1") != "0"
# MGX_LINEAR_QKNORM=0: the q | k projection always writes its [tokens, 2d] output and mgx_qk_norm_rope_fwd_qs makes Q, K of it
LINEAR_QKNORM = os.environ.get("MGX_LINEAR_QKNORM", "1") != "0"
ROPE_PAIR_TABLE = os.environ.get("MGX_ROPE_PAIR_TABLE", "1") != "0"   # that epilogue reads (cos, sin) per pair when the tables allow


def linear_t(X, W, bias, Ct, tokens, F, K, ld_ct, tok_rpb, ct_bstride):
    """Ct[b][f][t] = bf16(X[b * tok_rpb + t] . W[f] + bias[f]) (`mgx_linear_bf16_t`: a Linear whose output leaves transposed,
    token-contiguous).  X plain [tokens, K], W [F, K]; Ct: a tensor whose data_ptr() is the element of (b 0, f 0, t 0).
    False -- nothing launched -- when the persistent kernel cannot take the shape."""
    ws = _sk_workspace(X.device) if GEMM_STREAM_K else None
    return _profiled(_try, (lib().mgx_linear_bf16_t, ptr(X), ptr(W), ptr(bias), Ct.data_ptr(), tokens, F, K, K, K, ld_ct, tok_rpb,
                            ct_bstride, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), stream()),
                     2.0 * tokens * F * K, (F, tokens, K, EPI_BIAS))


def _gemm_launch(A, W, bias, C, N, K, epi, gate, gate_ld, aux, beta, ldw, ldaux, stream_k=None):
    ws = _sk_workspace(C.t.device) if (GEMM_STREAM_K if stream_k is None else stream_k) else None
    check(lib().mgx_gemm_bf16_sk(ptr(A.t), ptr(W), ptr(bias), ptr(C.t), None if gate is None else gate.data_ptr(),
                                 None if aux is None else aux.data_ptr(), (N if ldaux is None else ldaux), A.M, N, K, A.ld,
                                 A.rpb, A.bstride, K if ldw is None else ldw, C.ld, C.rpb, C.bstride, gate_ld, epi, beta,
                                 None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), stream()))


# The text- and the image-stream Linear of a double block go out as two launches.  One launch for both (a pair entry point
# that walked the two problems as one tile grid, `MGX_GEMM_PAIR=1`) was built, measured neutral and removed on that evidence:
# same box, round 4, 18.418 s per step paired vs 18.397 s unpaired, 9745 vs 12861 launches, GEMM family 1374.5 vs 1372.7
# TFLOP/s (profiles/r04_bench_c_pair{1,0}.json.log).  The text launches' low rates (440-1240 TFLOP/s) are the idle capacity of
# a partial round, and the merged launch ends in the same partial round: the rollout's N = 3072 pair is 192 + 1536 tiles =
# 0.75 + 6 rounds apart and 6.75 -> 7 rounds together.


# Stream-K tail of the persistent GEMM (csrc/gemm.hip): on by default; MGX_GEMM_STREAM_K=0 calls the kernel without a
# workspace (every tile computed whole: results independent of the batch size).
GEMM_STREAM_K = os.environ.get("MGX_GEMM_STREAM_K", "1") != "0"
_sk_ws = {}


def _sk_workspace(device):
    """The caller-owned fp32 workspace of mgx_gemm_bf16_sk: one per (device, stream) that launches GEMMs."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    w = _sk_ws.get(key)
    if w is None:
        w = torch.empty(lib().mgx_gemm_sk_workspace_elems(), dtype=F32, device=device)
        _sk_ws[key] = w
    return w


_scratch = {}


def scratch(name, numel, dtype, device):
    """Grow-only named scratch buffers (caller-owned workspace for the C ABI)."""
    key = (name, dtype, device)
    t = _scratch.get(key)
    if t is None or t.numel() < numel:
        t = torch.empty(int(numel), dtype=dtype, device=device)
        _scratch[key] = t
    return t[:numel]


def transpose(inp: Rows, N, out, ld_out, colsum_out=None, colsum_beta=1.0, gelu=False):
    """out[N, ld_out] = inp[M, N]^T (zero padded); optional colsum_out[n] = beta*colsum_out[n] + sum_m inp[m,n].
    `gelu`: out = gelu_tanh(inp)^T (plain matrix, no column sums): the activation of a kept FF pre-activation."""
    if gelu:
        assert colsum_out is None and inp.rpb >= inp.M
        check(lib().mgx_transpose_gelu_bf16(ptr(inp.t), ptr(out), inp.M, N, inp.ld, ld_out, stream()))
        return
    part = None
    if colsum_out is not None:
        part = scratch("colsum_partial", lib().mgx_transpose_partial_elems(inp.M, N), F32, out.device)
    check(lib().mgx_transpose_bf16(ptr(inp.t), ptr(out), ptr(part), ptr(colsum_out), colsum_beta, inp.M, N, inp.ld,
                                   inp.rpb, inp.bstride, ld_out, stream()))


def ln_modulate(x: Rows, shift, scale, mod_ld, y, D, stats=None):
    """y[M, D] = bf16(LN(x) * bf16(1+scale[b]) + shift[b]); shift/scale are views at their chunk of mod [B, mod_ld]."""
    check(lib().mgx_ln_modulate_fwd(ptr(x.t), x.ld, x.rpb, x.bstride, shift.data_ptr(), scale.data_ptr(), mod_ld, ptr(y),
                                    D, ptr(stats), x.M, D, stream()))


def ln_modulate_bwd(dy, x: Rows, scale, mod_ld, dx: Rows, accumulate, dshift, dscale, D):
    ws = scratch("ln_bwd", lib().mgx_ln_modulate_bwd_workspace(x.M, min(x.rpb, x.M), D), F32, dy.device)
    check(lib().mgx_ln_modulate_bwd(ptr(dy), D, ptr(x.t), x.ld, min(x.rpb, x.M), x.bstride, scale.data_ptr(), mod_ld,
                                    ptr(dx.t), dx.ld, min(dx.rpb, dx.M), dx.bstride, int(accumulate), dshift.data_ptr(),
                                    dscale.data_ptr(), ptr(ws), x.M, D, stream()))


LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
# Q leaves mgx_qk_norm_rope_fwd_qs multiplied by softmax scale * log2(e) (scores = exponents of two: mgx_attn_fwd_log2's
# accumulator-initialised softmax); every other consumer of that Q takes scale = ln 2.  MGX_ATTN_Q_PRESCALE=0: plain Q.
Q_PRESCALE = os.environ.get("MGX_ATTN_Q_PRESCALE", "1") != "0"


def qk_norm_rope(qkv, wq, wk, cos, sin, Q, K, Vt, B, H, S, Sp, rows_per_batch, s0, V=None, Qt=None, Kt=None, q_scale=1.0):
    check(lib().mgx_qk_norm_rope_fwd_qs(ptr(qkv), qkv.shape[-1], ptr(wq), ptr(wk), ptr(cos), ptr(sin), ptr(Q), ptr(K),
                                        ptr(Vt), ptr(V), ptr(Qt), ptr(Kt), B, H, S, Sp, rows_per_batch, s0, float(q_scale),
                                        stream()))


def qk_norm_rope_bwd(qkv, wq, wk, cos, sin, dQ, dK, dV, dqkv, gwq, gwk, B, H, S, Sp, rows_per_batch, s0, ld_dqkv=None,
                     q_scale=1.0):
    """`dqkv`: a tensor whose data_ptr() is the first element of the [rows, >= 3d] output; `ld_dqkv` its row stride in
    elements (default: 3d, a plain matrix).  `q_scale`: the forward's (dQ is the gradient of the scaled Q)."""
    ws = scratch("qk_bwd", lib().mgx_qk_norm_rope_bwd_workspace(B, H, rows_per_batch), F32, qkv.device)
    check(lib().mgx_qk_norm_rope_bwd_qs(ptr(qkv), qkv.shape[-1], ptr(wq), ptr(wk), ptr(cos), ptr(sin), ptr(dQ), ptr(dK),
                                        ptr(dV), dqkv.data_ptr(), qkv.shape[-1] if ld_dqkv is None else ld_dqkv, ptr(gwq),
                                        ptr(gwk), ptr(ws), B, H, S, Sp, rows_per_batch, s0, float(q_scale), stream()))


def linear_qk_norm_rope(X, Wqk, bias, wq, wk, cos, sin, Q, K, B, H, S, rows_per_batch, s0, Kdim, q_scale=1.0, pairs=None):
    """Q, K [B, H, S, 128] <- qk_norm_rope(X @ Wqk^T + bias) in ONE launch (`mgx_linear_qk_norm_rope`: the norm / RoPE / head
    split run in the GEMM's epilogue).  X plain [B * rows_per_batch, Kdim], Wqk [2 * H * 128, Kdim].  False -- nothing launched --
    when the persistent kernel cannot take the problem: the caller keeps `gemm` + `qk_norm_rope`.  `pairs`: [S, 64, 2] (cos, sin)
    per rotation pair when both entries of every pair of `cos` / `sin` are equal (`rope_pair_table`): half the table bytes."""
    return _profiled(_try, (lib().mgx_linear_qk_norm_rope, ptr(X), ptr(Wqk), ptr(bias), ptr(wq), ptr(wk), ptr(cos), ptr(sin), ptr(pairs),
                            ptr(Q), ptr(K), B, H, S, rows_per_batch, s0, Kdim, Kdim, Kdim, float(q_scale), stream()),
                     2.0 * B * rows_per_batch * 2 * H * 128 * Kdim, (B * rows_per_batch, 2 * H * 128, Kdim, 5))


def rope_pair_table(cos, sin):
    """[S, 64, 2] (cos, sin) per rotation pair if the two entries of every pair are equal in both tables, else None."""
    if not (torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])):
        return None
    return torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1).contiguous()


def attn_fwd(Q, K, Vt, O_ptr_tensor, lse, B, H, S, Sp, ldo, o_bstride, scale):
    check(lib().mgx_attn_fwd(ptr(Q), ptr(K), ptr(Vt), O_ptr_tensor.data_ptr(), ptr(lse), B, H, S, Sp, ldo, o_bstride,
                             scale, stream()))


def attn_fwd_log2(Q2, K, Vt, O_ptr_tensor, lse, B, H, S, Sp, ldo, o_bstride):
    """Q2 = Q * scale * log2(e), from qk_norm_rope(..., q_scale=scale * LOG2E)."""
    check(lib().mgx_attn_fwd_log2(ptr(Q2), ptr(K), ptr(Vt), O_ptr_tensor.data_ptr(), ptr(lse), B, H, S, Sp, ldo, o_bstride,
                                  stream()))


def attn_fwd_path(B, H, S, Sp, ldo, o_bstride):
    """The kernel attn_fwd / attn_fwd_log2 launch for this problem: 0 = 8-wave, 1 = the generated 64-query one."""
    r = lib().mgx_attn_fwd_path(B, H, S, Sp, ldo, o_bstride)
    check(min(r, 0))
    return r


# A sequence that is off 256 is padded to the next multiple with the padding masked (attn_fwd_log2_kv, attn_bwd_kv), so that the
# 64-wide attention kernels and the fused projections apply: the no-grad forward (flux.py, _forward_nograd) and the training
# forward / recompute / backward (FluxFunction) alike, so rollout and replay of a sample run the same kernels on the same
# padded shape.  Off by default.
ATTN_PAD_KV = os.environ.get("MGX_ATTN_PAD_KV", "0") != "0"


def attn_fwd_log2_kv(Q2, K, Vt, O_ptr_tensor, lse, B, H, Sa, kv_len, ldo, o_bstride):
    """attn_fwd_log2 on operands allocated at Sa (% 256 == 0) with the keys >= kv_len masked (`mgx_attn_fwd_log2_kv`).  False --
    nothing launched -- when the 64-query kernel cannot take the problem (attn_fwd_kv_path): the caller keeps the unpadded path."""
    return _try(lib().mgx_attn_fwd_log2_kv, ptr(Q2), ptr(K), ptr(Vt), O_ptr_tensor.data_ptr(), ptr(lse), B, H, Sa, kv_len, ldo, o_bstride,
                stream())


def attn_fwd_kv_path(B, H, Sa, kv_len, ldo, o_bstride):
    """1 when attn_fwd_log2_kv takes this problem, 0 when it refuses it.  Launches nothing."""
    return lib().mgx_attn_fwd_kv_path(B, H, Sa, kv_len, ldo, o_bstride)


def attn_bwd_path(B, H, S, Sp, ldo, o_bstride):
    """The kernels attn_bwd launches for this problem: 0 = 8-wave dkv / dq, 1 = the generated 64-wide pair."""
    r = lib().mgx_attn_bwd_path(B, H, S, Sp, ldo, o_bstride)
    check(min(r, 0))
    return r


def attn_fp8_quantize(Q, K, Vt, Q8, K8, V8t, amax, B, H, S, Sp):
    """Per-(batch, head) e4m3 quantisation of the attention operands (csrc/attention_fp8.hip)."""
    check(lib().mgx_attn_fp8_quantize(ptr(Q), ptr(K), ptr(Vt), ptr(Q8), ptr(K8), ptr(V8t), ptr(amax), B, H, S, Sp,
                                      stream()))


def attn_fwd_fp8(Q8, K8, V8t, amax, O_ptr_tensor, lse, B, H, S, Sp, ldo, o_bstride, scale):
    check(lib().mgx_attn_fwd_fp8(ptr(Q8), ptr(K8), ptr(V8t), ptr(amax), O_ptr_tensor.data_ptr(), ptr(lse), B, H, S, Sp,
                                 ldo, o_bstride, scale, stream()))


# The e4m3 attention backward (csrc/attention_fp8_bwd.hip) behind attention_dtype="fp8": the gradient of the quantised function
# the forward ran, instead of the bf16 backward on the bf16 operands.  Off by default until it has been measured in a train step.
ATTN_FP8_BWD = os.environ.get("MGX_ATTN_FP8_BWD", "0") != "0"


def attn_bwd_fp8_workspace(B, H, S, Sp):
    """Bytes of the workspace `attn_bwd_fp8` needs (host code: no GPU)."""
    n = lib().mgx_attn_bwd_fp8_workspace(B, H, S, Sp)
    if n < 0:
        raise ValueError(f"attn_bwd_fp8_workspace: bad sizes B {B} H {H} S {S} Sp {Sp}")
    return n


def attn_bwd_fp8_layout(B, H, S, Sp):
    """name -> (byte offset, shape) of the workspace sections `mgx_attn_bwd_fp8` fills (include/mixgrpo_hip.h)."""
    rb, tb = (B * H * S * 128 + 255) // 256 * 256, B * H * 128 * Sp
    out = {n: (i * rb, (B, H, S, 128)) for i, n in enumerate(("Q8", "K8", "V8", "dO8"))}
    out.update({n: (4 * rb + i * tb, (B, H, 128, Sp)) for i, n in enumerate(("Q8t", "K8t", "dO8t"))})
    return out


def attn_bwd_fp8(Q, K, V, Qt, Kt, O, dO, lse, delta, dOt, dQ, dK, dV, ws, amax, B, H, S, Sp, ldo, o_bstride, scale):
    """attn_bwd on the e4m3 MFMA, from the O / lse of attn_fwd_fp8; ws: `attn_bwd_fp8_workspace` bytes, amax: fp32 [4 * B * H]."""
    check(lib().mgx_attn_bwd_fp8(ptr(Q), ptr(K), ptr(V), ptr(Qt), ptr(Kt), O.data_ptr(), dO.data_ptr(), ptr(lse), ptr(delta),
                                 ptr(dOt), ptr(dQ), ptr(dK), ptr(dV), ptr(ws), ptr(amax), B, H, S, Sp, ldo, o_bstride, scale,
                                 ws.numel(), stream()))


def skinny_linear(x, W, bias, out, N, K):
    """out[b] = bf16(x[b] @ W^T + bias) for <= 16 rows per call (more rows are chunked)."""
    Bn = x.shape[0]
    for b0 in range(0, Bn, 16):
        nb = min(16, Bn - b0)
        check(lib().mgx_skinny_linear(x[b0:].data_ptr(), x.stride(0), ptr(W), K, ptr(bias), out[b0:].data_ptr(),
                                      out.stride(0), nb, N, K, stream()))


def skinny_wgrad(dout, x, dW, dbias, N, K):
    Bn = x.shape[0]
    for b0 in range(0, Bn, 16):
        nb = min(16, Bn - b0)
        check(lib().mgx_skinny_wgrad(dout[b0:].data_ptr(), dout.stride(0), x[b0:].data_ptr(), x.stride(0), ptr(dW), K,
                                     ptr(dbias), nb, N, K, stream()))


def skinny_dgrad(dout, W, dx, N, K, accumulate=True):
    """dx[Bn, K] (+)= bf16(dout[Bn, N] @ W[N, K]) from the row-major bf16 weight."""
    Bn = dout.shape[0]
    for b0 in range(0, Bn, 8):
        nb = min(8, Bn - b0)
        ws = scratch("skinny_dgrad", lib().mgx_skinny_dgrad_workspace(nb, K), F32, dout.device)
        check(lib().mgx_skinny_dgrad(dout[b0:].data_ptr(), dout.stride(0), ptr(W), K, dx[b0:].data_ptr(), dx.stride(0),
                                     ptr(ws), nb, N, K, 1 if accumulate else 0, stream()))


def ew(a, b, y, op):
    check(lib().mgx_ew_bf16(ptr(a), ptr(b), ptr(y), a.numel(), op, stream()))


def sincos_embed(t, out):
    check(lib().mgx_sincos_embed(ptr(t), ptr(out), t.numel(), stream()))


def cast_bf16(x, y):
    check(lib().mgx_cast_f32_bf16(ptr(x), ptr(y), x.numel(), stream()))


def gelu_rows(x, ldx, y, ldy, M, N):
    """y[m, :N] = bf16(gelu_tanh(x[m, :N])) for M rows `ldx` / `ldy` elements apart: the bias+GELU epilogue's activation
    re-created from a kept pre-activation (bit-identical, see include/mixgrpo_hip.h)."""
    check(lib().mgx_gelu_bf16(ptr(x), ldx, ptr(y), ldy, M, N, stream()))


def cast_f32(x, y, scale=1.0):
    """y (fp32) = scale * x (bf16)."""
    check(lib().mgx_cast_bf16_f32(ptr(x), ptr(y), x.numel(), float(scale), stream()))


def gate_bwd(dout: Rows, y, gate, gate_ld, dy, dgate, batches, rows_per_batch, D):
    ws = scratch("gate_bwd", lib().mgx_gate_bwd_workspace(batches, rows_per_batch, D), F32, y.device)
    check(lib().mgx_gate_bwd(ptr(dout.t), dout.ld, dout.bstride, ptr(y), D, gate.data_ptr(), gate_ld, ptr(dy), D,
                             dgate.data_ptr(), ptr(ws), batches, rows_per_batch, D, stream()))


def sqnorm(g, out, beta=0.0):
    ws = scratch("sqnorm", lib().mgx_sqnorm_workspace(), torch.float64, g.device)
    check(lib().mgx_sqnorm_f32(ptr(g), g.numel(), ptr(ws), ptr(out), beta, stream()))


def adamw_step(w, w16, g, m, v, lr, beta1, beta2, eps, wd, step, gnorm_sq, max_norm, grad_scale=1.0):
    check(lib().mgx_adamw_step(ptr(w), ptr(w16), ptr(g), ptr(m), ptr(v), w.numel(), lr, beta1, beta2, eps, wd, step,
                               ptr(gnorm_sq), max_norm, grad_scale, stream()))


def attn_bwd(Q, K, V, Qt, Kt, O, dO, lse, delta, dOt, dQ, dK, dV, B, H, S, Sp, ldo, o_bstride, scale):
    check(lib().mgx_attn_bwd(ptr(Q), ptr(K), ptr(V), ptr(Qt), ptr(Kt), O.data_ptr(), dO.data_ptr(), ptr(lse), ptr(delta),
                             ptr(dOt), ptr(dQ), ptr(dK), ptr(dV), B, H, S, Sp, ldo, o_bstride, scale, stream()))


def attn_bwd_kv(Q, K, V, Qt, Kt, O, dO, lse, delta, dOt, dQ, dK, dV, B, H, Sa, kv_len, ldo, o_bstride, scale):
    """attn_bwd on operands allocated at Sa (% 256 == 0) with the keys and queries >= kv_len masked and the rows >= kv_len of
    dQ / dK / dV written as zero (`mgx_attn_bwd_kv`).  False -- nothing launched -- when the 64-wide pair cannot take the
    problem (attn_bwd_kv_path): there is no other kernel behind it."""
    return _try(lib().mgx_attn_bwd_kv, ptr(Q), ptr(K), ptr(V), ptr(Qt), ptr(Kt), O.data_ptr(), dO.data_ptr(), ptr(lse), ptr(delta),
                ptr(dOt), ptr(dQ), ptr(dK), ptr(dV), B, H, Sa, kv_len, ldo, o_bstride, scale, stream())


def attn_bwd_kv_path(B, H, Sa, kv_len, ldo, o_bstride):
    """1 when attn_bwd_kv takes this problem, 0 when it refuses it.  Launches nothing."""
    return lib().mgx_attn_bwd_kv_path(B, H, Sa, kv_len, ldo, o_bstride)


# ------------------------------------------------------------------------------------------------ low-rank adapters (csrc/lora.hip)
LORA_RANKS = (16, 32, 64, 128)


def lora_proj(inp: Rows, P, out, Kin, r, scale):
    """out[M, r] = bf16(scale * inp[M, Kin] @ P[r, Kin]^T); `inp` any row-batched view, `P` / `out` plain bf16 matrices."""
    check(lib().mgx_lora_proj(ptr(inp.t), ptr(P), ptr(out), inp.M, Kin, r, inp.ld, min(inp.rpb, 1 << 40), inp.bstride, float(scale),
                              stream()))


def lora_wgrad_workspace(M, Kin, r):
    """fp32 elements of the workspace `lora_wgrad` needs (host code: no GPU)."""
    n = lib().mgx_lora_wgrad_workspace(M, Kin, r)
    if n < 0:
        raise ValueError(f"lora_wgrad_workspace: unsupported sizes M {M} Kin {Kin} r {r} (r in {LORA_RANKS}, Kin % 64 == 0, M >= 1)")
    return n


def lora_wgrad(small, big: Rows, G, Kin, r, beta=1.0):
    """G[r, Kin] (fp32) = beta * G + small[M, r]^T @ big[M, Kin]; `small` plain bf16, `big` any row-batched view."""
    ws = scratch("lora_wgrad", lora_wgrad_workspace(big.M, Kin, r), F32, G.device)
    check(lib().mgx_lora_wgrad(ptr(small), ptr(big.t), ptr(G), ptr(ws), ws.numel(), big.M, Kin, r, big.ld, min(big.rpb, 1 << 40),
                               big.bstride, float(beta), stream()))


def lora_merge(W0, Bt, A, W16, N, K, r, s):
    """W16[N, K] = bf16(W0 + s * Bt[r, N]^T @ A[r, K]) from the fp32 masters: fp64 sum, one rounding."""
    check(lib().mgx_lora_merge(ptr(W0), ptr(Bt), ptr(A), ptr(W16), N, K, r, float(s), stream()))


# ------------------------------------------------------------------------------------------------ VAE decode (csrc/vae.hip)
def _interior(outpad, W, C):
    """The zero-bordered [(H+2), (W+2), C] image `outpad` from its first interior pixel on: one row and one pixel in"""
    return outpad.view(-1)[(W + 2) * C + C:]


def conv3x3(xpad, Wt, bias, out, H, W, C, Cout, ones=None, ld_out=None):
    """out[H W, Cout] (+)= conv3x3(xpad) + bias: xpad zero-bordered NHWC [(H+2), (W+2), C], Wt [Cout, 3, 3, C].
    `ones` given: the residual form out = bf16(out + bf16(conv + bias))."""
    check(lib().mgx_conv3x3_nhwc(ptr(xpad), ptr(Wt), ptr(bias), ptr(out), Cout if ld_out is None else ld_out, ptr(ones), H, W, C,
                                 Cout, 0 if ones is None else 1, stream()))


def group_norm(x, gamma, beta, out, H, W, C, G, silu, padded, eps=1e-6, ld=None):
    """out = [silu](GroupNorm(x)), x plain [H W, C]; `padded`: out is a zero-bordered [(H+2), (W+2), C] image (interior written).
    `ld`: x is the first C columns of a plain [H W, ld] matrix (a tensor whose data_ptr() is its first element)."""
    ws = scratch("group_norm", lib().mgx_group_norm_workspace(H * W, C, G), F32, x.device)
    if padded:
        o, out_row = _interior(out, W, C), (W + 2) * C
    else:
        o, out_row = out, W * C
    check(lib().mgx_group_norm_nhwc(ptr(x) if ld is None else x.data_ptr(), C if ld is None else ld, ptr(gamma), ptr(beta),
                                    o.data_ptr(), out_row, C, ptr(ws), H, W, C, G, eps, 1 if silu else 0, stream()))


def upsample2x_pad(x, outpad, H, W, C):
    """plain [H W, C] -> interior of the zero-bordered [(2H+2), (2W+2), C] image `outpad`"""
    check(lib().mgx_upsample2x_pad_nhwc(ptr(x), _interior(outpad, 2 * W, C).data_ptr(), H, W, C, stream()))


def latents_to_pad(z, outpad, Cin, H, W, C):
    check(lib().mgx_latents_to_pad_nhwc(ptr(z), _interior(outpad, W, C).data_ptr(), Cin, H, W, C, stream()))


def nhwc_to_image(x, ld, img, Cout, H, W):
    check(lib().mgx_nhwc_to_image(ptr(x), ld, ptr(img), Cout, H, W, stream()))


def conv3x3s2(xpad, Wt, bias, out, H, W, C, Cout, ld_out=None):
    """out[(H/2)(W/2), Cout] = conv3x3(F.pad(x, (0, 1, 0, 1)), stride 2) + bias: xpad the zero-bordered NHWC image
    [(H+2), (W+2), C] of the H x W activation x (H, W even), Wt [Cout, 3, 3, C]."""
    check(lib().mgx_conv3x3s2_nhwc(ptr(xpad), ptr(Wt), ptr(bias), ptr(out), Cout if ld_out is None else ld_out, H, W, C, Cout,
                                   stream()))


def pad_nhwc(x, ld, outpad, H, W, C):
    """first C channels of plain [H W, ld] -> interior of the zero-bordered [(H+2), (W+2), C] image `outpad`"""
    check(lib().mgx_pad_nhwc(ptr(x), ld, _interior(outpad, W, C).data_ptr(), H, W, C, stream()))


def diag_gaussian(moments, ld, noise, mean, std, sample, Cz, H, W):
    """moments plain NHWC [H W, ld] (mean | logvar) -> mean, std, sample [Cz, H, W] bf16; noise None: sample = mean"""
    check(lib().mgx_diag_gaussian_nhwc(ptr(moments), ld, ptr(noise), ptr(mean), ptr(std), ptr(sample), Cz, H, W, stream()))


def softmax_rows(S, P, M, n, scale):
    check(lib().mgx_softmax_rows_f32(ptr(S), S.stride(0), ptr(P), P.stride(0), M, n, scale, stream()))


# ------------------------------------------------------------------------------------------------ CLIP ViT tower (csrc/clip.hip)
ACT_GELU, ACT_QUICK_GELU = 0, 1


def clip_patch_cols(patch):
    """Columns of a patch row: 3 p p rounded up to the GEMM's K % 64 == 0 (588 -> 640)."""
    return (3 * patch * patch + 63) // 64 * 64


def clip_preprocess(image, R, patch, mean, std, patches, levels=None):
    """image [3, H, W] bf16 in about [-1, 1] -> patches [(R / p)^2, clip_patch_cols(p)] bf16 (`mgx_clip_preprocess`); `levels`:
    optional uint8 [3, R, R] that receives the resized, cropped 0..255 image."""
    import ctypes
    _, H, W = image.shape
    ws = scratch("clip_preprocess", lib().mgx_clip_preprocess_workspace(H, W, R), F32, image.device)
    f3 = ctypes.c_float * 3
    check(lib().mgx_clip_preprocess(ptr(image), H, W, R, patch, f3(*mean), f3(*std), ptr(patches), patches.shape[-1], ptr(levels),
                                    ptr(ws), ws.numel(), stream()))


def vit_embed(patch_out, cls, pos, x, B, S, width):
    check(lib().mgx_vit_embed(ptr(patch_out), ptr(cls), ptr(pos), ptr(x), B, S, width, stream()))


def layer_norm_affine(x, ldx, gamma, beta, y, ldy, M, D, eps):
    """y[m, :D] = bf16(LN(x[m, :D]; eps) * gamma + beta); x, y: tensors whose data_ptr() is the first element, rows ldx / ldy
    elements apart (y may be x)."""
    check(lib().mgx_layer_norm_affine(x.data_ptr(), ldx, ptr(gamma), ptr(beta), y.data_ptr(), ldy, M, D, float(eps), stream()))


def vit_attn_fwd(qkv, ld_qkv, O, ldo, B, H, S, d, scale):
    """O[b S + s, h d:] = softmax(scale q k^T) v from the packed projection rows q | k | v (`mgx_vit_attn_fwd`); qkv, O: tensors
    whose data_ptr() is the first element.  False -- nothing launched -- for S > 4096."""
    return _try(lib().mgx_vit_attn_fwd, qkv.data_ptr(), ld_qkv, O.data_ptr(), ldo, B, H, S, d, float(scale), stream())


def act_rows(x, ldx, y, ldy, M, N, act):
    check(lib().mgx_act_rows(x.data_ptr(), ldx, y.data_ptr(), ldy, M, N, act, stream()))


def l2_normalize_rows(f, out):
    check(lib().mgx_l2_normalize_rows(ptr(f), f.stride(0), ptr(out), f.shape[0], f.shape[1], stream()))


def cosine_score(f, t, out, logit_scale=1.0, mean=0.0, std=1.0):
    """out[b] = (logit_scale cos(f[b], t[b]) - mean) / std; f [B, n], t [B, n] or [1, n], bf16 or fp32 rows."""
    for a in (f, t):
        if a.dtype not in (BF16, F32):
            raise ValueError("cosine_score takes bf16 or fp32 rows")
    B, n = f.shape
    check(lib().mgx_cosine_score(ptr(f), int(f.dtype == F32), f.stride(0), ptr(t), int(t.dtype == F32),
                                 0 if t.shape[0] == 1 else t.stride(0), ptr(out), B, n,
                                 float(logit_scale), float(mean), float(std), stream()))


# ------------------------------------------------------------------------------------------------ text encoders (csrc/text.hip)
ACT_GELU_TANH = 2


def text_attn_fwd(qkv, ld_qkv, O, ldo, B, H, S, d, scale, causal=False, rel_bias=None):
    """`vit_attn_fwd` with a causal mask and / or a relative-position bias table [H, 2 S - 1] fp32 (`mgx_text_attn_fwd`).
    False -- nothing launched -- for S > 4096."""
    if rel_bias is not None and (rel_bias.dtype != F32 or tuple(rel_bias.shape) != (H, 2 * S - 1)):
        raise ValueError(f"rel_bias must be fp32 [{H}, {2 * S - 1}], not {rel_bias.dtype} {tuple(rel_bias.shape)}")
    return _try(lib().mgx_text_attn_fwd, qkv.data_ptr(), ld_qkv, O.data_ptr(), ldo, B, H, S, d, float(scale), int(bool(causal)),
                ptr(rel_bias), stream())


def rms_norm_affine(x, ldx, gamma, y, ldy, M, D, eps):
    """y[m, :D] = bf16(x[m, :D] * rsqrt(mean(x^2) + eps) * gamma); x, y: tensors whose data_ptr() is the first element, rows
    ldx / ldy elements apart (y may be x)."""
    check(lib().mgx_rms_norm_affine(x.data_ptr(), ldx, ptr(gamma), y.data_ptr(), ldy, M, D, float(eps), stream()))


def gated_act_rows(a, lda, b, ldb, y, ldy, M, N, act):
    """y = bf16(act(a) * b) on rows lda / ldb / ldy elements apart (y may be a); act: ACT_GELU, ACT_QUICK_GELU, ACT_GELU_TANH"""
    check(lib().mgx_gated_act_rows(a.data_ptr(), lda, b.data_ptr(), ldb, y.data_ptr(), ldy, M, N, act, stream()))


def token_embed(input_ids, table, pos, x):
    """x[b S + s] = bf16(table[input_ids[b, s]] + pos[s]) (`mgx_token_embed`); `input_ids` an integer tensor [B, S], normally on
    the host: the ids are checked where they are, before the copy to the device, and an id outside [0, V) raises a ValueError
    that names it and its position -- nothing is launched.  pos fp32 [>= S, D] or None."""
    if input_ids.dim() != 2 or input_ids.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool):
        raise ValueError(f"input_ids must be an integer tensor [B, S], not {input_ids.dtype} {tuple(input_ids.shape)}")
    B, S = input_ids.shape
    V, D = table.shape
    bad = ((input_ids < 0) | (input_ids >= V)).nonzero()
    if bad.numel():
        b, s = (int(v) for v in bad[0])
        raise ValueError(f"token id {int(input_ids[b, s])} at position ({b}, {s}) is outside the vocabulary [0, {V})")
    if pos is not None and (pos.shape[0] < S or pos.shape[1] != D):
        raise ValueError(f"{S} positions of width {D} need pos [>= {S}, {D}], not {tuple(pos.shape)}")
    ids = input_ids.to(device=table.device, dtype=torch.int32).contiguous()
    check(lib().mgx_token_embed(ptr(ids), ptr(table), ptr(pos), ptr(x), B * S, S, D, V, stream()))


# ------------------------------------------------------------------------------------------------ ImageReward (csrc/blip.hip)
def check_kv_len(kv_len, B, Skv):
    """The contract of `mgx_xattn_fwd`'s key lengths, checked where the tensor is (normally the host): an integer tensor [B]
    with every entry in [1, Skv]; anything else raises a ValueError that names it."""
    if kv_len.dim() != 1 or kv_len.shape[0] != B or kv_len.dtype.is_floating_point or kv_len.dtype == torch.bool:
        raise ValueError(f"kv_len must be an integer tensor [{B}], not {kv_len.dtype} {tuple(kv_len.shape)}")
    bad = ((kv_len < 1) | (kv_len > Skv)).nonzero()
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"key length {int(kv_len[b])} of sample {b} is outside [1, {Skv}]")


def xattn_fwd(q, ldq, k, ldk, v, ldv, O, ldo, B, H, Sq, Skv, d, scale, kv_len=None, kv_len_checked=False):
    """O[b Sq + s, h d:] = softmax(scale q k^T over the keys t < kv_len[b]) v with q, k, v in buffers of their own
    (`mgx_xattn_fwd`); q, k, v, O: tensors whose data_ptr() is the first element, rows ldq / ldk / ldv / ldo elements apart.
    `kv_len`: an integer tensor [B], normally on the host, or None (all Skv keys): the lengths are checked where they are
    (`check_kv_len`), before the copy to the device -- nothing is launched on a bad one.  `kv_len_checked`: the caller has done
    that already and passes the lengths on the device (a layer loop checks and copies once).  False -- nothing launched -- for
    Sq > 4096 or Skv > 4096."""
    lens = None
    if kv_len is not None:
        if not kv_len_checked:
            check_kv_len(kv_len, B, Skv)
        lens = kv_len.to(device=O.device, dtype=torch.int32).contiguous()
    return _try(lib().mgx_xattn_fwd, q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, O.data_ptr(), ldo, B, H, Sq, Skv, d,
                float(scale), ptr(lens), stream())


def linear_rows_f32(x, W, bias, out, shift=None, scale=None):
    """out[M, N] (fp32) = x[M, K] @ W[N, K]^T + bias, then `(. - shift) / scale` when both are given (`mgx_linear_rows_f32`).
    x bf16 or fp32 rows (stride(0) elements apart), W and bias (or None) fp32, out fp32 rows."""
    if x.dtype not in (BF16, F32) or W.dtype != F32 or out.dtype != F32 or (bias is not None and bias.dtype != F32):
        raise ValueError("linear_rows_f32 takes bf16 or fp32 rows and fp32 weights, bias and output")
    if (shift is None) != (scale is None):
        raise ValueError("give shift and scale, or neither")
    M, K = x.shape
    N = W.shape[0]
    if W.shape[1] != K or tuple(out.shape) != (M, N) or (bias is not None and tuple(bias.shape) != (N,)):
        raise ValueError(f"x {tuple(x.shape)} W {tuple(W.shape)} out {tuple(out.shape)} do not fit")
    if x.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("x and out must have unit column stride")
    check(lib().mgx_linear_rows_f32(x.data_ptr(), int(x.dtype == F32), x.stride(0) if M > 1 else max(x.stride(0), K), ptr(W),
                                    ptr(bias), out.data_ptr(), out.stride(0) if M > 1 else max(out.stride(0), N), M, N, K,
                                    int(shift is not None), float(shift or 0.0), float(1.0 if scale is None else scale), stream()))
