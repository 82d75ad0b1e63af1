"""CPU checks of the float64 references in norm_refs.py: each agrees with oracle/mmdit.py at fp32 level, and the tolerance
predicates the kernel-level GPU tests use (test_hip_norm_kernels.py) reject a column sum that lost one row of the last
partial block of the last batch, a reduction that swapped two batches, and a LayerNorm-backward output rounded twice."""
import math

import torch

import norm_refs as R
from norm_refs import F64, U32
from oracle import mmdit as OM


def _bf16_values(t):
    return t.bfloat16().float()


def test_modulate_matches_oracle():
    g = torch.Generator().manual_seed(0)
    B, Rn, D = 2, 5, 256
    x = _bf16_values(torch.randn(B, Rn, D, generator=g) * 2 + 3)
    shift, scale = (_bf16_values(torch.randn(B, D, generator=g) * 0.5) for _ in range(2))
    ref = R.modulate(x, shift, scale)
    got = OM.modulate(x, shift, scale)
    xh, _, rstd = R.layer_norm(x)
    # fp32 LayerNorm: mean / variance of D terms, then the product and the sum with shift
    bound = (D / 8) * U32 * ((xh.abs() + x.abs().mean(-1, keepdim=True) * rstd) * R.scale1(scale)[:, None].abs()
                             + shift.double().abs()[:, None])
    assert ((got.double() - ref).abs() <= bound).all()


def test_rms_norm_rope_matches_oracle():
    g = torch.Generator().manual_seed(1)
    B, H, S = 2, 3, 17
    x = _bf16_values(torch.randn(B, H, S, 128, generator=g))
    w = 1 + 0.2 * torch.randn(128, generator=g)
    cos, sin = torch.cos(torch.rand(S, 128, generator=g) * 6.28), torch.sin(torch.rand(S, 128, generator=g) * 6.28)
    ref = R.rms_norm_rope(x, w, cos, sin)
    got = OM.apply_rope(OM.rms_norm(x, w), cos, sin)
    assert ((got.double() - ref).abs() <= 16 * U32 * R.rms_norm_rope_abs(x, w, cos, sin)).all()
    # q_scale multiplies the whole output
    assert torch.allclose(R.rms_norm_rope(x, w, cos, sin, q_scale=0.3), 0.3 * ref, rtol=1e-15, atol=0)


def test_sincos256_matches_oracle():
    t = torch.tensor([0.0, 1.0, 952.0, 1000.0, 17.25, 499.5])
    ref, ang = R.sincos256(t)
    got = OM.sincos256(t)
    k = torch.arange(128, dtype=F64)
    # the oracle's fp32 frequency exp(-ln(1e4) k / 128) is off by <= (2|z| + 3) ulp (z its exponent); the angle error follows
    ang_err = ang.abs() * (2 * math.log(10000.0) * k / 128 + 3) * U32
    bound = torch.cat([ang_err, ang_err], -1) + 4 * U32
    assert ((got.double() - ref).abs() <= bound).all()


def test_silu_and_gated_residual_match_oracle():
    g = torch.Generator().manual_seed(2)
    a = _bf16_values(torch.randn(4096, generator=g) * 4)
    ok, msg = R.bf16_close(OM.silu(a).bfloat16(), R.silu(a), bound=8 * U32 * R.silu(a).abs())
    assert ok, msg
    B, Rn, D = 3, 7, 64
    x, y = (_bf16_values(torch.randn(B, Rn, D, generator=g)) for _ in range(2))
    gate = _bf16_values(torch.randn(B, D, generator=g))
    want = OM._bf(x + OM._bf(gate[:, None] * y))            # oracle/mmdit.py forward: gated_residual
    assert torch.equal(R.gated_residual(x, gate, y).float(), want)
    # the backward of silu is autograd's: b * sigmoid(a) (1 + a (1 - sigmoid(a)))
    s = torch.sigmoid(a.double())
    b = torch.randn(4096, generator=g, dtype=F64)
    assert torch.allclose(R.dsilu_times(a, b), b * s * (1 + a.double() * (1 - s)), rtol=1e-12, atol=1e-300)


def _column_sums(dout, y, drop_last=False, swap=False):
    """What the gate-backward kernels compute: fp32 per-batch column sums of dout * y, rounded once to bf16; optionally
    with the last row of the last batch's last (partial) 64-row block left out, or with batches 0 and 1 swapped."""
    p = (dout.float() * y.float())
    if drop_last:
        p = p.clone()
        p[-1, -1] = 0
    s = p.sum(1).bfloat16()
    return s[[1, 0] + list(range(2, s.shape[0]))] if swap else s


def test_tolerance_rejects_a_dropped_tail_row_and_swapped_batches():
    g = torch.Generator().manual_seed(3)
    B, rows, D = 3, 100, 3072                   # 64-row blocks: batch 2's second block holds 36 rows, the dropped one among them
    dout, y = (torch.randn(B, rows, D, generator=g).bfloat16() for _ in range(2))
    gate = torch.randn(B, D, generator=g).bfloat16()
    ref, _ = R.gated_residual_bwd(torch.zeros(B, rows, D), gate, y, dout)
    terms = (dout.double() * y.double()).abs().sum(1)
    c = 64 + 2 + 4                               # the kernel's chain: 64 rows, 2 partials, two tree levels (+ slack)
    assert R.reduction_close(_column_sums(dout, y), ref, terms, c, bf16_out=True)[0]
    assert not R.reduction_close(_column_sums(dout, y, drop_last=True), ref, terms, c, bf16_out=True)[0]
    assert not R.reduction_close(_column_sums(dout, y, swap=True), ref, terms, c, bf16_out=True)[0]
    # the GPU tests' own power check: the reference without one row's contribution is rejected for the correct result
    ref_drop = ref.clone()
    ref_drop[-1] -= dout[-1, -1].double() * y[-1, -1].double()
    assert not R.reduction_close(_column_sums(dout, y), ref_drop, terms, c, bf16_out=True)[0]


def test_tolerance_rejects_a_second_rounding_in_the_layernorm_backward():
    """dx (+)= dLN is ONE rounding of old + dLN: a kernel that rounded dLN to bf16 first differs from the correctly rounded
    value in far more than the allowed fraction of elements."""
    g = torch.Generator().manual_seed(4)
    B, rows, D = 2, 16, 1024
    x, dy, old = (_bf16_values(torch.randn(B, rows, D, generator=g)) for _ in range(3))
    scale = _bf16_values(torch.randn(B, D, generator=g) * 0.3)
    dx, _, _ = R.modulate_bwd(x, scale, dy)
    ref = old.double() + dx
    once = ref.float().bfloat16()
    twice = (old + dx.float().bfloat16().float()).bfloat16()
    bound = 64 * U32 * (old.double().abs() + dx.abs())
    assert R.bf16_close(once, ref, bound)[0]
    assert not R.bf16_close(twice, ref, bound)[0]
