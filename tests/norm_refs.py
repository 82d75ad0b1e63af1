"""float64 restatements of the HBM-bound per-row kernels (csrc/norm.hip, csrc/small.hip) and the tolerance predicates their
kernel-level tests use.  Plain torch, device-agnostic: the GPU tests evaluate them on the device in float64, the CPU test
(test_norm_refs.py) checks them against oracle/mmdit.py and checks that the predicates can see a dropped row.

Rounding points kept (oracle/mmdit.py, include/mixgrpo_hip.h): bf16(1 + scale) of the modulation, bf16(gate * dout) of the
gated residual's input gradient, and one bf16 rounding per kernel output -- everything else is exact float64.  `bf` is
straight-through, so torch.autograd of these functions in float64 is the reference for the backward kernels.

Tolerance rule:
  * a bf16 output lies within one bf16 ulp of the float64 value, plus `fp32_bound` = c * 2^-24 * sum|terms| where the kernel's
    fp32 terms cancel; and at most `frac` of the elements differ from the correctly rounded float64 value;
  * a reduction (column sums, row statistics, weight gradients) lies within c * 2^-24 * sum|terms| of the float64 value, c
    the length of the kernel's longest sequential fp32 chain plus a small allowance; one bf16 ulp on top when it is stored
    as bf16.  Each reduction test also checks that the reference without one row's contribution is rejected."""
import math

import torch

F64 = torch.float64
EPS = 1e-6
U32 = 2.0 ** -24          # unit roundoff of fp32


class _RoundBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def bf(x):
    """Round to bf16 (through fp32, as a kernel rounds its fp32 value), keep the dtype; straight-through gradient."""
    return _RoundBF16.apply(x)


def bf16_ulp(x):
    """One bf16 ulp at |x| (float64): 2^(e - 7) for |x| in [2^e, 2^(e+1)), floored at the smallest subnormal 2^-133."""
    x = x.double().abs()
    _, e = torch.frexp(x)                          # x = m 2^e, m in [0.5, 1)
    u = torch.ldexp(torch.ones_like(x), (e - 8).clamp(min=-133))
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -133), u)


# ------------------------------------------------------------------------------------------------------------- forward maths
def layer_norm(x, eps=EPS):
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps), mean, torch.rsqrt(var + eps)


def scale1(scale):
    """bf16(1 + scale): the sum in fp32 (the oracle's fp32 tensor, the kernel's fp32 register), rounded once."""
    return (1 + scale.float()).bfloat16().to(F64)


def modulate(x, shift, scale, eps=EPS):
    """x [B, R, D], shift / scale [B, D] (bf16 values): LN(x) * bf16(1 + scale) + shift, float64."""
    xh, _, _ = layer_norm(x, eps)
    return xh * scale1(scale)[:, None] + shift.to(F64)[:, None]


def rms_norm_rope(x, w, cos, sin, q_scale=1.0, eps=EPS):
    """x [..., S, 128] (bf16 values), w [128], cos / sin [S, 128] general tables (the two entries of a pair may differ):
    RMSNorm(eps) * w, then interleaved-pair RoPE (x0 c0 - x1 s0, x1 c1 + x0 s1), times q_scale.  float64."""
    x = x.to(F64)
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.to(F64)
    c, s = cos.to(F64), sin.to(F64)
    y0, y1 = y[..., 0::2], y[..., 1::2]
    out = torch.stack([y0 * c[:, 0::2] - y1 * s[:, 0::2], y1 * c[:, 1::2] + y0 * s[:, 1::2]], -1).flatten(-2)
    return out * q_scale


def rms_norm_rope_abs(x, w, cos, sin, q_scale=1.0, eps=EPS):
    """The same expression on absolute values (|y0 c0| + |y1 s0|, ...): the size of the terms the RoPE sum cancels."""
    x = x.to(F64)
    y = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.to(F64)).abs()
    c, s = cos.to(F64).abs(), sin.to(F64).abs()
    y0, y1 = y[..., 0::2], y[..., 1::2]
    out = torch.stack([y0 * c[:, 0::2] + y1 * s[:, 0::2], y1 * c[:, 1::2] + y0 * s[:, 1::2]], -1).flatten(-2)
    return out * abs(q_scale)


def gated_residual(x, gate, y):
    """bf16(x + bf16(gate[b] * y)) with x, y [B, R, D], gate [B, D]: the residual update of the FLUX blocks
    (oracle/mmdit.py forward's gated_residual)."""
    return bf(x.to(F64) + bf(gate.to(F64)[:, None] * y.to(F64)))


def silu(a):
    a = a.to(F64)
    return a * torch.sigmoid(a)


def dsilu_times(a, b):
    """b * silu'(a) from autograd of `silu` in float64."""
    a = a.to(F64).detach().requires_grad_(True)
    (g,) = torch.autograd.grad(silu(a), a, b.to(F64))
    return g


def sincos256(t):
    """Timesteps(256, flip_sin_to_cos=True, shift 0): [cos(t f_k) | sin(t f_k)], f_k = 10000^(-k/128), float64."""
    f = torch.exp(-math.log(10000.0) * torch.arange(128, dtype=F64, device=t.device) / 128)
    ang = t.to(F64)[:, None] * f[None]
    return torch.cat([torch.cos(ang), torch.sin(ang)], -1), ang


# ------------------------------------------------------------------------------------------------------------ backward maths
def modulate_bwd(x, scale, dy):
    """(dx, dshift, dscale) of `modulate` for upstream dy [B, R, D]: autograd in float64 (per-batch column sums for
    dshift / dscale)."""
    x = x.to(F64).detach().requires_grad_(True)
    sh = torch.zeros(scale.shape, dtype=F64, device=x.device, requires_grad=True)
    sc = scale.to(F64).detach().requires_grad_(True)
    xh, _, _ = layer_norm(x)
    y = xh * bf(1 + sc)[:, None] + sh[:, None]         # (bf: the same bf16(1 + scale) with a straight-through gradient)
    return torch.autograd.grad(y, (x, sh, sc), dy.to(F64))


def rms_norm_rope_bwd(x, w, cos, sin, dout, q_scale=1.0):
    """(dx, dw) of `rms_norm_rope` for upstream dout: autograd in float64 (dw summed over every leading index and position)."""
    x = x.to(F64).detach().requires_grad_(True)
    w = w.to(F64).detach().requires_grad_(True)
    return torch.autograd.grad(rms_norm_rope(x, w, cos, sin, q_scale), (x, w), dout.to(F64))


def gated_residual_bwd(x, gate, y, dout):
    """(dgate [B, D], dy) of `gated_residual` for upstream dout; dy keeps its rounding point: bf16(gate * dout)."""
    gate = gate.to(F64).detach().requires_grad_(True)
    y = y.to(F64).detach().requires_grad_(True)
    dg, dy = torch.autograd.grad(gated_residual(x, gate, y), (gate, y), dout.to(F64))
    return dg, dy


# ------------------------------------------------------------------------------------------------------------- predicates
def bf16_close(out, ref, bound=0.0, frac=0.01):
    """`out` (bf16) within one bf16 ulp of the float64 `ref` plus `bound` (an fp32 bound on cancelling terms) everywhere, and
    at most `frac` of the elements different from bf16(ref).  Returns (ok, message)."""
    o, r = out.to(F64), ref.to(F64)
    if not torch.isfinite(o).all():
        return False, "non-finite output"
    excess = (o - r).abs() - bf16_ulp(r) - bound
    if (excess > 0).any():
        i = int(excess.flatten().argmax())
        return False, f"|out - ref| over 1 ulp + bound by {excess.max().item():.3g} (out {o.flatten()[i].item()}, ref {r.flatten()[i].item()})"
    miss = (out.to(torch.bfloat16) != bf(r).to(torch.bfloat16)).double().mean().item()
    if miss > frac:
        return False, f"{miss:.4f} of the elements differ from the correctly rounded value (> {frac})"
    return True, ""


def reduction_close(out, ref, abs_terms, c, bf16_out=False):
    """A reduction's `out` within c * 2^-24 * sum|terms| (`abs_terms`, same shape as ref) of the float64 `ref`, plus one bf16
    ulp when the output is stored as bf16.  Returns (ok, message)."""
    o, r = out.to(F64), ref.to(F64)
    tol = c * U32 * abs_terms.to(F64)
    if bf16_out:
        tol = tol + bf16_ulp(r)
    if not torch.isfinite(o).all():
        return False, "non-finite output"
    excess = (o - r).abs() - tol
    if (excess > 0).any():
        return False, f"reduction off by {excess.max().item():.3g} beyond c * 2^-24 * sum|terms| (c = {c})"
    return True, ""


def assert_ok(res):
    ok, msg = res
    assert ok, msg
