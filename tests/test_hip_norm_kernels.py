"""Kernel-level GPU tests of the HBM-bound per-row kernels against float64 references (norm_refs.py, evaluated on the device):
`mgx_ln_modulate_fwd / _bwd`, `mgx_qk_norm_rope_fwd_qs / _bwd_qs` (csrc/norm.hip), `mgx_gate_bwd`, `mgx_ew_bf16`,
`mgx_sincos_embed` and the two casts (csrc/small.hip), through the `ops` wrappers and `Rows` views the model uses.

Shapes go where these kernels have edges: row counts that are no multiple of the kernels' row groups (4 rows per LayerNorm
workgroup, 32 / 64 rows per backward block, 64 tokens per RMSNorm block), several partial blocks per batch (so the finish
kernels' strided walk runs for b > 0), B up to 8, the joint-sequence views of flux.py (`_stream_rows`), chunk offsets inside
the modulation vector, and block counts on both sides of the weight-gradient reduction's first stage (QK_FIN_G = 128).
Memory a kernel must not touch holds a sentinel and is checked afterwards.

Tolerances (norm_refs.py): a bf16 output within one bf16 ulp of the float64 value plus c * 2^-24 * sum|terms| where the fp32
terms cancel, and at most 1 % of the elements different from the correctly rounded value; a reduction within
c * 2^-24 * sum|terms| (c: the kernel's longest sequential fp32 chain plus a small allowance, stated at each use), one bf16 ulp
on top when stored as bf16 -- and the same reference without one row's contribution must fail that predicate."""
import math

import pytest
import torch

import norm_refs as R
from norm_refs import F64, U32, assert_ok

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENT = -776.0                    # exact in bf16 and fp32: memory a kernel must leave alone holds it
QS = 1.4426950408889634 / math.sqrt(128)     # the attention path's q_scale (softmax scale * log2 e)


def _g(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, g, std=1.0, mean=0.0):
    return (torch.randn(shape, device="cuda", generator=g) * std + mean).to(BF)


def _ops():
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    return ops, Rows


# ------------------------------------------------------------------------------------------------------- AdaLN modulate
def _check_ln_fwd(y, stats, x, shift, scale):
    """y [B, R, D] bf16 and stats [B, R, 2] fp32 of mgx_ln_modulate_fwd against float64."""
    D = x.shape[-1]
    xh, mean, rstd = R.layer_norm(x)
    s1 = R.scale1(scale)[:, None]
    ref = xh * s1 + shift.to(F64)[:, None]
    # c: a lane's D / 64 sequential terms, the 6-level wave tree, rsqrt and the products.  The normalised value carries the
    # mean's error (relative to mean|x|, scaled by rstd) and rstd's; then one product and one sum with shift.
    c = D / 64 + 8
    mabs = x.to(F64).abs().mean(-1, keepdim=True)
    bound = c * U32 * (xh.abs() + mabs * rstd) * s1.abs() + 2 * U32 * (xh.abs() * s1.abs() + shift.to(F64).abs()[:, None])
    assert_ok(R.bf16_close(y, ref, bound))
    # stats: the mean is a D-term sum (c * 2^-24 * mean|x|); rstd = rsqrt(var + eps), var a sum of positive terms: relative
    # error c / 2 + 3 ulp
    assert_ok(R.reduction_close(stats[..., 0], mean[..., 0], mabs[..., 0], c))
    assert_ok(R.reduction_close(stats[..., 1], rstd[..., 0], rstd[..., 0], c / 2 + 3))
    # power: the mean without the row's last element is rejected
    assert not R.reduction_close(stats[..., 0], mean[..., 0] - x[..., -1].to(F64) / D, mabs[..., 0], c)[0]


@pytest.mark.parametrize("D", [512 * k for k in range(1, 9)])
def test_ln_modulate_fwd_every_width(D):
    """All eight instantiations on 3 batches of 23 rows (69: the last workgroup runs one of its four waves) read through a
    row-batched view with two junk rows between batches; shift / scale are chunks of a [B, 3D] modulation vector."""
    ops, Rows = _ops()
    g = _g(D)
    B, rpb, pad = 3, 23, 2
    M = B * rpb
    xs = _randn((B, rpb + pad, D), g, 1.5, 0.3)
    mod = _randn((B, 3 * D), g, 0.5)
    shift, scale = mod[:, 2 * D:], mod[:, D:2 * D]
    y = torch.full((M + 1, D), SENT, dtype=BF, device="cuda")
    stats = torch.full((M + 1, 2), SENT, device="cuda")
    ops.ln_modulate(Rows(xs, M, D, rpb, (rpb + pad) * D), shift, scale, 3 * D, y, D, stats=stats)
    _check_ln_fwd(y[:M].view(B, rpb, D), stats[:M].view(B, rpb, 2), xs[:, :rpb], shift, scale)
    assert (y[M] == SENT).all() and (stats[M] == SENT).all()


@pytest.mark.parametrize("B,L,N", [(3, 45, 77), (8, 512, 4096)])
def test_ln_modulate_fwd_joint_views(B, L, N):
    """D = 3072 through the joint-sequence views flux.py builds (`_stream_rows`): the text rows and the image rows of one
    [B, L + N, d] buffer (bstride = S d), each stream against its own chunks of a [B, 6d] modulation vector.  The image rows
    have a large mean and a small spread.  (3, 45, 77): rows per stream no multiple of 32; (8, 512, 4096): the rollout's size."""
    ops, Rows = _ops()
    d, S = 3072, L + N
    g = _g(B + L + N)
    X = torch.cat([_randn((B, L, d), g, 1.0, 0.2), _randn((B, N, d), g, 0.5, 24.0)], 1).contiguous()
    m = _randn((B, 6 * d), g, 0.5)
    nrm = torch.full((B * S + 1, d), SENT, dtype=BF, device="cuda")
    stats = torch.full((B * S + 1, 2), SENT, device="cuda")
    views = {"txt": (Rows(X, B * L, d, L, S * d), 0, L, 0), "img": (Rows(X[0, L:], B * N, d, N, S * d), B * L, N, L)}
    for name, (xr, r0, rows, s0) in views.items():
        ops.ln_modulate(xr, m[:, 3 * d:4 * d] if name == "img" else m[:, 0:d], m[:, 4 * d:5 * d] if name == "img" else m[:, d:2 * d],
                        6 * d, nrm[r0:r0 + B * rows], d, stats=stats[r0:r0 + B * rows])
    for name, (xr, r0, rows, s0) in views.items():
        shift, scale = (m[:, 3 * d:4 * d], m[:, 4 * d:5 * d]) if name == "img" else (m[:, 0:d], m[:, d:2 * d])
        _check_ln_fwd(nrm[r0:r0 + B * rows].view(B, rows, d), stats[r0:r0 + B * rows].view(B, rows, 2), X[:, s0:s0 + rows],
                      shift, scale)
    assert (nrm[B * S] == SENT).all() and (stats[B * S] == SENT).all()


# (B, rows per batch, D, mod_ld / D, accumulate, stream whose rows of the joint buffer are used)
LN_BWD = [(1, 1, 512, 2, 0, "img"), (3, 31, 3072, 6, 1, "txt"), (3, 33, 1024, 3, 0, "img"), (8, 100, 3072, 6, 1, "img"),
          (3, 4096, 3072, 3, 1, "img"), (8, 4096, 3072, 6, 0, "txt"), (1, 4096, 4096, 2, 1, "txt")]
# where scale sits in the modulation vector and where dshift / dscale go, per mod_ld (flux.py / flux_backward.py's chunks)
MOD_CHUNKS = {2: (0, 1, 0), 3: (1, 0, 1), 6: (4, 3, 4)}


@pytest.mark.parametrize("B,rows,D,k,acc,stream", LN_BWD)
def test_ln_modulate_bwd(B, rows, D, k, acc, stream):
    """dx (written, or ONE rounding of old + dLN with accumulate), dshift / dscale (per-batch column sums, WRITTEN as bf16)
    against float64 autograd of the modulation.  x and dx are one stream's rows of joint [B, S, D] buffers: the other
    stream's 7 rows per batch keep their values; the other chunks of the [B, k D] gradient vector keep the sentinel.
    rows 4096: 128 blocks per batch, the finish kernel's four-lane walk 32 deep."""
    ops, Rows = _ops()
    g = _g(B * 10007 + rows + D + k + acc)
    other = 7
    S = rows + other
    off = 0 if stream == "txt" else other
    M = B * rows
    X = _randn((B, S, D), g, 1.0, 0.5)
    dX0 = _randn((B, S, D), g, 0.7)
    dX = dX0.clone()
    dy = _randn((M, D), g)
    mod = _randn((B, k * D), g, 0.5)
    c_sc, c_dsh, c_dsc = MOD_CHUNKS[k]
    scale = mod[:, c_sc * D:(c_sc + 1) * D]
    dmod = torch.full((B, k * D), SENT, dtype=BF, device="cuda")
    dshift, dscale = dmod[:, c_dsh * D:(c_dsh + 1) * D], dmod[:, c_dsc * D:(c_dsc + 1) * D]
    view = lambda t: Rows(t[0, off:] if off else t, M, D, rows, S * D)     # noqa: E731
    ops.ln_modulate_bwd(dy, view(X), scale, k * D, view(dX), acc, dshift, dscale, D)

    x, dyv = X[:, off:off + rows], dy.view(B, rows, D)
    dx64, dsh64, dsc64 = R.modulate_bwd(x, scale, dyv)
    # dx: dLN = rstd (gx - mean(gx) - xh mean(gx xh)), gx = dy bf16(1 + scale) (exact in fp32); c covers the two D-term means
    # and the normalised value's error (its mean and rstd), then the sum with the old value
    xh, mean, rstd = R.layer_norm(x)
    gx = (dyv.to(F64) * R.scale1(scale)[:, None]).abs()
    mabs_r = x.to(F64).abs().mean(-1, keepdim=True) * rstd
    c = D / 64 + 8
    old = dX0[:, off:off + rows].to(F64) if acc else torch.zeros_like(dx64)
    a = rstd * (gx + gx.mean(-1, keepdim=True) + (xh.abs() + mabs_r) * (gx * xh.abs()).mean(-1, keepdim=True)
                + xh.abs() * (gx * (xh.abs() + mabs_r)).mean(-1, keepdim=True))
    bound = c * U32 * (a + dx64.abs() + old.abs())
    assert_ok(R.bf16_close(dX[:, off:off + rows], old + dx64, bound))
    # the other stream's rows are untouched
    keep = torch.ones(S, dtype=torch.bool, device="cuda")
    keep[off:off + rows] = False
    assert torch.equal(dX[:, keep], dX0[:, keep])
    # dshift / dscale: each wave sums 8 rows of its 32-row block, 4 waves combine, 4 lanes walk blocks_per_batch / 4 partials,
    # two tree levels; dscale's terms carry the normalised value's error (c above, relative to |xh| + mean|x| rstd)
    bpb = (rows + 31) // 32
    cr = 8 + 4 + bpb / 4 + 2 + 2
    ad = dyv.to(F64).abs()
    t_sh = ad.sum(1)
    t_sc = (ad * (xh.abs() + (c / cr) * (xh.abs() + mabs_r))).sum(1)
    assert_ok(R.reduction_close(dshift, dsh64, t_sh, cr, bf16_out=True))
    assert_ok(R.reduction_close(dscale, dsc64, t_sc, cr, bf16_out=True))
    untouched = torch.ones(k * D, dtype=torch.bool, device="cuda")
    for t in (dshift, dscale):
        o = (t.data_ptr() - dmod.data_ptr()) // 2
        untouched[o:o + D] = False
    assert (dmod[:, untouched] == SENT).all()
    # power: without the last row of the last batch (the last partial block's) the references are rejected
    dsh_drop, dsc_drop = dsh64.clone(), dsc64.clone()
    dsh_drop[-1] -= dyv[-1, -1].to(F64)
    dsc_drop[-1] -= dyv[-1, -1].to(F64) * xh[-1, -1]
    assert not R.reduction_close(dshift, dsh_drop, t_sh, cr, bf16_out=True)[0]
    assert not R.reduction_close(dscale, dsc_drop, t_sc, cr, bf16_out=True)[0]


# ------------------------------------------------------------------------------------------------------ QK norm + RoPE
def _qk_case(B, H, S, rows, seed):
    g = _g(seed)
    qkv = _randn((B * rows, 3 * H * 128), g)
    wq = 1 + 0.2 * torch.randn(128, device="cuda", generator=g)
    wk = 1 + 0.2 * torch.randn(128, device="cuda", generator=g)
    # general tables: the two entries of a rotation pair differ
    cos = torch.cos(torch.rand(S, 128, device="cuda", generator=g) * 6.28)
    sin = torch.sin(torch.rand(S, 128, device="cuda", generator=g) * 6.28)
    return g, qkv, wq, wk, cos, sin


def _heads(t, B, rows, H):
    """[B rows, H 128] -> [B, H, rows, 128]"""
    return t.reshape(B, rows, H, 128).permute(0, 2, 1, 3)


# (B, H, S, Sp, rows per batch, s0, extras V / Qt / Kt, V^T written, q_scale)
QK_FWD = [(2, 3, 200, 256, 150, 50, True, True, QS), (3, 2, 61, 64, 61, 0, False, False, 1.0),
          (1, 4, 700, 768, 188, 512, True, True, 1.0), (2, 2, 130, 192, 127, 0, False, True, QS),
          (2, 3, 600, 640, 77, 50, False, True, 1.0)]


@pytest.mark.parametrize("B,H,S,Sp,rows,s0,extras,vt,qs", QK_FWD)
def test_qk_norm_rope_fwd(B, H, S, Sp, rows, s0, extras, vt, qs):
    """Q, K against float64 RMSNorm + RoPE (general cos / sin tables, Q times q_scale); V^T, V copies of the v columns and
    Q^T, K^T the transposed Q, K, bit for bit.  Positions outside s0 .. s0 + rows (and the Sp > S padding) keep the sentinel.
    s0 = 50: the transposed stores take the scalar path; rows 61 / 127 / 77: tails of a 64-token block and of a 4-token pass."""
    ops, _ = _ops()
    g, qkv, wq, wk, cos, sin = _qk_case(B, H, S, rows, B * 1000 + rows + s0)
    d = H * 128
    full = lambda *s: torch.full(s, SENT, dtype=BF, device="cuda")      # noqa: E731
    Q, K = full(B, H, S, 128), full(B, H, S, 128)
    Vt = full(B, H, 128, Sp) if vt else None
    ex = dict(V=full(B, H, S, 128), Qt=full(B, H, 128, Sp), Kt=full(B, H, 128, Sp)) if extras else {}
    ops.qk_norm_rope(qkv, wq, wk, cos, sin, Q, K, Vt, B, H, S, Sp, rows, s0, q_scale=qs, **ex)
    sl = slice(s0, s0 + rows)
    cs, ss = cos[sl], sin[sl]
    for out, cols, w, scale in ((Q, slice(0, d), wq, qs), (K, slice(d, 2 * d), wk, 1.0)):
        x = _heads(qkv[:, cols], B, rows, H)
        ref = R.rms_norm_rope(x, w, cs, ss, scale)
        # c = 16: the 64-pair tree sum and rsqrt (r to ~7 ulp), the two products, w * q_scale rounded, the RoPE sum
        assert_ok(R.bf16_close(out[:, :, sl], ref, 16 * U32 * R.rms_norm_rope_abs(x, w, cs, ss, scale)))
        assert (out[:, :, :s0] == SENT).all() and (out[:, :, s0 + rows:] == SENT).all()
    v = _heads(qkv[:, 2 * d:], B, rows, H)
    pairs = [(Vt, v.transpose(-1, -2))] if vt else []
    if extras:
        pairs += [(ex["Qt"], Q[:, :, sl].transpose(-1, -2)), (ex["Kt"], K[:, :, sl].transpose(-1, -2))]
        assert torch.equal(ex["V"][:, :, sl], v)
        assert (ex["V"][:, :, :s0] == SENT).all() and (ex["V"][:, :, s0 + rows:] == SENT).all()
    for t, want in pairs:
        assert torch.equal(t[..., sl], want)
        assert (t[..., :s0] == SENT).all() and (t[..., s0 + rows:] == SENT).all()


# (B, H, S, Sp, rows per batch, s0, ld_dqkv / d, q_scale): per-block partials 18 / 2 (< QK_FIN_G = 128) and 180 / 384 (>)
QK_BWD = [(2, 3, 200, 256, 150, 50, 3, QS), (1, 2, 64, 64, 1, 0, 3, 1.0), (3, 12, 330, 384, 300, 30, 7, 1.0),
          (2, 24, 600, 640, 512, 64, 7, QS)]


@pytest.mark.parametrize("B,H,S,Sp,rows,s0,ldm,qs", QK_BWD)
def test_qk_norm_rope_bwd(B, H, S, Sp, rows, s0, ldm, qs):
    """dqkv (dq, dk: float64 autograd of the forward; dv: the incoming dV, passed through bit for bit) and the RMSNorm weight
    gradients, which the kernel ADDS to gwq / gwk (started here from nonzero values).  ld_dqkv = 7d: the single blocks'
    [M, 7d] staging matrix, whose columns beyond 3d keep the sentinel."""
    ops, _ = _ops()
    g, qkv, wq, wk, cos, sin = _qk_case(B, H, S, rows, B * 77 + rows + H)
    d = H * 128
    dQ, dK, dV = (_randn((B, H, S, 128), g) for _ in range(3))
    dqkv = torch.full((B * rows, ldm * d), SENT, dtype=BF, device="cuda")
    g0q, g0k = torch.randn(128, device="cuda", generator=g) * 10, torch.randn(128, device="cuda", generator=g) * 10
    gwq, gwk = g0q.clone(), g0k.clone()
    ops.qk_norm_rope_bwd(qkv, wq, wk, cos, sin, dQ, dK, dV, dqkv, gwq, gwk, B, H, S, Sp, rows, s0, ld_dqkv=ldm * d, q_scale=qs)
    sl = slice(s0, s0 + rows)
    cs, ss = cos[sl], sin[sl]
    nblocks = (rows + 63) // 64 * H * B
    for cols, w, dO, scale, gw, g0 in ((slice(0, d), wq, dQ, qs, gwq, g0q), (slice(d, 2 * d), wk, dK, 1.0, gwk, g0k)):
        x = _heads(qkv[:, cols], B, rows, H).to(F64)
        dout = dO[:, :, sl].to(F64)
        dx, dw = R.rms_norm_rope_bwd(x, w, cs, ss, dout, scale)
        # size of the terms: gy = rope^T(dout q_scale) (|go0 c0| + |go1 s1|, ...), dx = r gy w - x r^3 mean(gy w x)
        go = dout.abs() * scale
        ca, sa = cs.to(F64).abs(), ss.to(F64).abs()
        gy = torch.stack([go[..., 0::2] * ca[:, 0::2] + go[..., 1::2] * sa[:, 1::2],
                          go[..., 0::2] * sa[:, 0::2] + go[..., 1::2] * ca[:, 1::2]], -1).flatten(-2)
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + R.EPS)
        gz = gy * w.to(F64).abs()
        a = r * gz + x.abs() * r ** 3 * (gz * x.abs()).mean(-1, keepdim=True)
        # c = 32: r (~7 ulp) enters cubed, the 64-lane sum of the dot product, the RoPE transpose's sums
        got = dqkv[:, cols].reshape(B, rows, H, 128).permute(0, 2, 1, 3)
        assert_ok(R.bf16_close(got, dx, 32 * U32 * a))
        # weight gradient: 16 tokens per lane, 4 waves, ceil(nblocks / 128) partials per first-stage workgroup, 8 + 16 in the
        # second stage, the += ; the terms (gy x r) carry ~12 ulp of their own
        terms = (gy * x.abs() * r).sum((0, 1, 2))
        cg = 16 + 4 + (nblocks + 127) // 128 + 8 + 16 + 1 + 12
        assert_ok(R.reduction_close(gw, g0.to(F64) + dw, terms + g0.to(F64).abs(), cg))
        # power: without the last token of the last head of the last batch the reference is rejected
        _, dw1 = R.rms_norm_rope_bwd(x[-1:, -1:, -1:], w, cs[-1:], ss[-1:], dout[-1:, -1:, -1:], scale)
        assert not R.reduction_close(gw, g0.to(F64) + dw - dw1, terms + g0.to(F64).abs(), cg)[0]
    assert torch.equal(dqkv[:, 2 * d:3 * d], dV[:, :, sl].permute(0, 2, 1, 3).reshape(B * rows, d))
    assert (dqkv[:, 3 * d:] == SENT).all()


# -------------------------------------------------------------------------------------------------------- gated residual
# (B, rows per batch, D, gate_ld / D, gate chunk): 64-row blocks -- rows 1 / 63 / 65 / 300 / 4096 give 1, 1, 2, 5, 64 per
# batch; D = 1000: a partial 512-column block
GATE = [(1, 1, 3072, 3, 2), (3, 63, 3072, 6, 2), (8, 65, 3072, 6, 5), (3, 300, 1000, 6, 5), (8, 4096, 3072, 6, 2),
        (1, 4096, 1000, 3, 2)]


@pytest.mark.parametrize("B,rows,D,k,chunk", GATE)
def test_gate_bwd(B, rows, D, k, chunk):
    """Backward of x + gate * y: dy = bf16(gate * dout) -- a product of two bf16 values, exact in fp32, so equal BIT FOR BIT
    to the correctly rounded float64 value -- and dgate = per-batch column sums of dout * y (bf16), against float64 autograd.
    dout is one stream's rows of a joint [B, S, D] buffer (d_bstride = S D != rows D); gate / dgate are chunks of [B, k D]
    vectors whose other chunks keep the sentinel; dy's row after the last keeps it too."""
    ops, Rows = _ops()
    g = _g(B * 31 + rows + D + k)
    other = 7
    S, M = rows + other, B * rows
    J = _randn((B, S, D), g)
    y = _randn((M, D), g)
    gate = _randn((B, k * D), g)[:, chunk * D:(chunk + 1) * D]
    dmod = torch.full((B, k * D), SENT, dtype=BF, device="cuda")
    dgate = dmod[:, chunk * D:(chunk + 1) * D]
    dy = torch.full((M + 1, D), SENT, dtype=BF, device="cuda")
    ops.gate_bwd(Rows(J[0, other:], M, D, rows, S * D), y, gate, k * D, dy, dgate, B, rows, D)
    dout = J[:, other:]
    dg64, dy64 = R.gated_residual_bwd(torch.zeros(B, rows, D, device="cuda"), gate, y.view(B, rows, D), dout)
    assert torch.equal(dy[:M].view(B, rows, D), dy64.float().bfloat16())
    assert (dy[M] == SENT).all()
    # dgate: 64 rows per thread, blocks_per_batch / 4 partials per lane, two tree levels (+ 2); the products are exact
    bpb = (rows + 63) // 64
    c = 64 + bpb / 4 + 2 + 2
    terms = (dout.to(F64) * y.view(B, rows, D).to(F64)).abs().sum(1)
    assert_ok(R.reduction_close(dgate, dg64, terms, c, bf16_out=True))
    keep = torch.ones(k * D, dtype=torch.bool, device="cuda")
    keep[chunk * D:(chunk + 1) * D] = False
    assert (dmod[:, keep] == SENT).all()
    # power: without the last row of the last batch the reference is rejected
    drop = dg64.clone()
    drop[-1] -= dout[-1, -1].to(F64) * y[-1].to(F64)
    assert not R.reduction_close(dgate, drop, terms, c, bf16_out=True)[0]


# -------------------------------------------------------------------------------------------- elementwise, embeddings, casts
@pytest.mark.parametrize("n", [1, 257, 2048 * 256 * 2 + 77])
@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_ew_bf16(op, n):
    """op 0 bf16(silu(a)), 1 bf16(b silu'(a)), 2 bf16(a + b), 3 y = bf16(y + a) against float64, with a = +-100 (expf
    overflows / underflows) among the inputs; n > 2048 * 256 runs the grid-stride loop."""
    ops, _ = _ops()
    g = _g(op * 7 + n)
    a = _randn(n, g, 4.0)
    a[:8] = torch.tensor([100.0, -100.0, 88.0, -88.0, 0.0, 20.0, -20.0, -1.28125], device="cuda").to(BF)[:n]
    b = _randn(n, g)
    y0 = _randn(n, g)
    y = y0.clone()
    ops.ew(a, b if op in (1, 2) else None, y, op)
    A, Bv = a.to(F64), b.to(F64)
    if op == 0:
        ref = R.silu(a)
        bound = 8 * U32 * ref.abs()                       # expf, 1 + e, the division
    elif op == 1:
        ref = R.dsilu_times(a, b)
        s = torch.sigmoid(A)
        bound = 8 * U32 * Bv.abs() * s * (1 + 2 * A.abs())   # 1 + a (1 - s) cancels near a = -1.28; 1 - s carries s's error
    else:
        ref = A + (Bv if op == 2 else y0.to(F64))
        bound = 2 * U32 * (A.abs() + (Bv if op == 2 else y0.to(F64)).abs())
    assert_ok(R.bf16_close(y, ref, bound))


@pytest.mark.parametrize("Bn", [1, 7])
def test_sincos_embed(Bn):
    """Timesteps(256, flip_sin_to_cos) against float64.  Tolerance: one bf16 ulp plus the angle error of the fp32 frequency
    exp(-ln(1e4) k / 128) ((2|z| + 3) ulp of the angle, z the exponent) and 4 ulp of sin / cos; the angle error also moves
    isolated elements across a rounding boundary (<= 5 % may differ from the correctly rounded value)."""
    ops, _ = _ops()
    g = _g(Bn)
    rnd = torch.rand(Bn, device="cuda", generator=g) * 1000
    t = torch.cat([torch.tensor([0.0, 1.0, 952.0, 1000.0], device="cuda"), rnd])[:Bn] if Bn >= 4 else rnd
    t = t.contiguous()
    out = torch.full((Bn + 1, 256), SENT, dtype=BF, device="cuda")
    ops.sincos_embed(t, out)
    ref, ang = R.sincos256(t)
    k = torch.arange(128, dtype=F64, device="cuda")
    ang_err = ang.abs() * (2 * math.log(10000.0) * k / 128 + 3) * U32
    assert_ok(R.bf16_close(out[:Bn], ref, torch.cat([ang_err, ang_err], -1) + 4 * U32, frac=0.05))
    assert (out[Bn] == SENT).all()


def _f32_bits(vals):
    return torch.tensor(vals, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_cast_f32_bf16_matches_torch_bit_for_bit():
    """mgx_cast_f32_bf16 against torch's .to(bfloat16): round-to-nearest-even ties (both parities), +-inf, values past the
    bf16 maximum (below / at / above the midpoint to infinity), fp32 subnormals, -0, on more elements than one grid pass
    (4096 workgroups x 1024); NaN stays NaN."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(11)
    n = 4096 * 1024 + 1028
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 30, (n,), generator=g).float())
    up = torch.randint(0, 1 << 15, (64,), generator=g, dtype=torch.int64)
    special = [(int(u) << 16) | 0x8000 for u in up]                                  # exact ties, even and odd upper halves
    special += [0x7F800000, 0xFF800000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F0000,
                0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00400000, 0x80000000, 0x00000000]
    sp = _f32_bits(special)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp
    nan_at = torch.tensor([100, 101, n - 200])
    x[nan_at] = _f32_bits([0x7FC00000, 0xFF800001, 0x7F800001])
    y = torch.empty(n + 8, dtype=BF, device="cuda")
    y[n:] = SENT
    ops.cast_bf16(x.cuda(), y[:n])
    got = y[:n].cpu()
    want = x.to(BF)
    isn = torch.isnan(x)
    assert torch.isnan(got[isn]).all()
    assert torch.equal(got[~isn].view(torch.int16), want[~isn].view(torch.int16))
    assert (y[n:] == SENT).all()


@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0])
def test_cast_bf16_f32_matches_torch_bit_for_bit(scale):
    """mgx_cast_bf16_f32: y = float(x) * scale, equal bit for bit to x.float() * scale (IEEE fp32 product), on more elements
    than one grid pass (4096 workgroups x 2048), with +-inf, -0, bf16 subnormals and NaN among the inputs."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(12)
    n = 4096 * 2048 + 1040
    xb = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())).to(BF)
    sp = torch.tensor([0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F, 0x0040, 0x7F7F, 0xFFC0], dtype=torch.int64).to(torch.int16).view(BF)
    xb[:sp.numel()] = sp
    xb[-sp.numel():] = sp
    y = torch.full((n + 8,), SENT, device="cuda")
    ops.cast_f32(xb.cuda(), y[:n], scale)
    got = y[:n].cpu()
    want = xb.float() * torch.tensor(scale, dtype=torch.float32)
    isn = torch.isnan(want)
    assert torch.isnan(got[isn]).all()
    assert torch.equal(got[~isn].view(torch.int32), want[~isn].view(torch.int32))
    assert (y[n:] == SENT).all()
