"""fp64 references of the e4m3 attention backward (mixgrpo_amd/csrc/attention_fp8_bwd.hip, `mgx_attn_bwd_fp8`).

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED against the reference: it has no fp8 attention (oracle/attention_fp8.py); what is
pinned instead is the kernel against its own recipe.  Two gradients of O = softmax(scale Q8 K8^T) V8 on the dequantised e4m3
operands of the forward (oracle.attention_fp8.quantize):
  (a) `backward(..., faithful=False)`: straight-through exact -- exact dO, P, dS; delta = rowsum(dO * O) from the O passed in;
  (b) `backward(..., faithful=True)`: the kernel's quantisation points applied through torch.float8_e4m3fn casts:
      dO8 (per-(batch, head) amax, scale 448 / amax) in dP, delta and dV, P8 = e4m3(256 P) in dV, and dS as MX blocks in dK and dQ:
      32 contiguous values along the contraction dimension (a column of one 32 x 32 accumulator block, the group the MFMA's block
      scale covers) share 2^e, e = floor(log2(448 / amax_block)).
      The blocks run along the queries for dK and along the keys for dQ.
`full_precision` is the same backward on the unquantised operands."""
import torch

from oracle import attention_fp8 as OA

F8 = torch.float8_e4m3fn


def accumulator_order():
    """Position p = 32 h + 16 b + i of a 64-row block -> row: lane half h of the MFMA that consumes a 64-wide score tile holds,
    as element 16 b + i of its operand, accumulator register i of 32-row block b, whose row is 32 b + 8 (i >> 2) + 4 h + (i & 3)
    (the 32x32 accumulator layout).  The transposed images Q8t, K8t, dO8t store their columns in this order."""
    return [32 * b + 8 * (i >> 2) + 4 * h + (i & 3) for h in range(2) for b in range(2) for i in range(16)]


def transposed_image(x8, Sp):
    """x8 [B, H, S, 128] float8 -> uint8 [B, H, 128, Sp]: transposed, zero from column S on, every 64-block in
    `accumulator_order()`."""
    B, H, S, hd = x8.shape
    xt = torch.zeros(B, H, hd, Sp, dtype=torch.uint8)
    xt[..., :S] = x8.view(torch.uint8).transpose(2, 3)
    return xt.view(B, H, hd, Sp // 64, 64)[..., torch.tensor(accumulator_order())].reshape(B, H, hd, Sp).contiguous()


def amax_table(Q, K, V, dO):
    """[4, B*H] fp32: max |x| of Q, K, V, dO [B, H, S, hd] per (batch, head)."""
    B, H = Q.shape[:2]
    return torch.stack([t.float().abs().reshape(B * H, -1).amax(dim=1) for t in (Q, K, V, dO)])


def dequantize(x8, amax):
    B, H = x8.shape[:2]
    return x8.to(torch.float64) * (amax.double().clamp_min(1e-30) / OA.F8_MAX).view(B, H, 1, 1)


def mx_quantize(x, dim):
    """x fp64 [..]: every MX block along `dim` -- 32 contiguous indices from a multiple of 32: one column of a 32 x 32 accumulator
    block, the values the hardware scales with one E8M0 byte -- is scaled by 2^e, e = floor(log2(448 / amax)) (0 for an all-zero
    block), cast to e4m3 and scaled back."""
    x = x.movedim(dim, -1)
    n = x.shape[-1]
    npad = (n + 31) // 32 * 32
    xp = torch.zeros(*x.shape[:-1], npad, dtype=torch.float64)
    xp[..., :n] = x
    blk = xp.view(*x.shape[:-1], npad // 32, 32)
    am = blk.abs().amax(dim=-1, keepdim=True)
    mant, ex = torch.frexp(am)                                  # am = mant * 2^ex, mant in [0.5, 1)
    e = 9 - ex - (mant > 0.875).to(ex.dtype)                    # 448 = 0.875 * 2^9
    e = torch.where(am == 0, torch.zeros_like(e), e).clamp(-126, 127)
    sc = torch.exp2(e.double())
    y = (blk * sc).float().to(F8).to(torch.float64) / sc
    return y.view(*x.shape[:-1], npad)[..., :n].movedim(-1, dim)


def _backward(q, k, v, do_q, O, scale, faithful):
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    P = torch.exp(s - torch.logsumexp(s, dim=-1, keepdim=True))
    O = torch.einsum("bhqk,bhkd->bhqd", P, v) if O is None else O.double()
    delta = (do_q * O).sum(-1, keepdim=True)                    # from the dO that dP is formed from: sum_k dS = 0
    dS = P * (torch.einsum("bhqd,bhkd->bhqk", do_q, v) - delta)
    Pv = (P * 256.0).float().to(F8).to(torch.float64) / 256.0 if faithful else P
    dV = torch.einsum("bhqk,bhqd->bhkd", Pv, do_q)
    dK = scale * torch.einsum("bhqk,bhqd->bhkd", mx_quantize(dS, -2) if faithful else dS, q)
    dQ = scale * torch.einsum("bhqk,bhkd->bhqd", mx_quantize(dS, -1) if faithful else dS, k)
    return dQ, dK, dV


def backward(Q, K, V, O, dO, scale, faithful):
    """Q, K, V, O, dO [B, H, S, 128] bf16 (O = None: the exact output) -> (dQ, dK, dV) fp64 of the e4m3 forward: reference (a) or
    (b) of the module text."""
    am = amax_table(Q, K, V, dO)
    q, k, v = (dequantize(OA.quantize(x, am[i]), am[i]) for i, x in enumerate((Q, K, V)))
    do_q = dequantize(OA.quantize(dO, am[3]), am[3]) if faithful else dO.double()
    return _backward(q, k, v, do_q, O, scale, faithful)


def full_precision(Q, K, V, dO, scale):
    """The gradient of full-precision attention on the unquantised operands (delta from its own output)."""
    return _backward(Q.double(), K.double(), V.double(), dO.double(), None, scale, False)


def rel_l2(x, ref):
    return ((x.double() - ref).norm() / ref.norm()).item()
