"""The skinny linears of the temb / AdaLN-modulation path (csrc/small.hip): forward, weight gradient and the input gradient
`mgx_skinny_dgrad`, against autograd of `torch.nn.functional.linear` on the same bf16 operands (what `loss.backward()`,
fastvideo/train_grpo_flux.py:600, runs through diffusers' AdaLayerNormZero.linear under bf16 autocast: fp32 accumulation, a
bf16 result per linear, bf16 accumulation of the per-user gradients of silu(temb))."""
import pytest
import torch

from helpers import grid as _grid, sentinel as _sentinel

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize("Bn,N,K", [(7, 6 * 3072, 3072),      # double-block modulation at micro-batch 7
                                     (8, 3 * 3072, 3072),      # single-block modulation
                                     (1, 2 * 3072, 3072),      # norm_out, one sample
                                     (12, 3072, 3072),         # temb MLP, 12 rows: two calls of the 8-row kernel
                                     (3, 130, 264)])           # ragged: rows not a multiple of the 128 row groups, K % 2048 != 0
def test_skinny_dgrad_vs_autograd(Bn, N, K):
    from mixgrpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
    dout = torch.randn(Bn, N, device="cuda", generator=g).to(BF16)
    acc0 = torch.randn(Bn, K, device="cuda", generator=g).to(BF16)
    ref = (dout.double() @ W.double())                                  # exact contraction
    want = (acc0.float() + ref.float().to(BF16).float()).to(BF16)      # bf16 result, added to the running bf16 sum
    got = acc0.clone()
    ops.skinny_dgrad(dout, W, got, N, K)
    # fp32 accumulation in a different order than the exact sum: at most one bf16 ulp on the linear's result, then one more
    # on the running sum
    err = (got.float() - want.float()).abs()
    tol = 2.0 ** -7 * want.float().abs().clamp_min(ref.float().abs()) + 1e-6
    assert (err <= tol).all(), (err / tol).max().item()
    assert (got == want).float().mean().item() > 0.98                  # almost all elements bit-identical
    fresh = torch.full((Bn, K), 7.0, device="cuda", dtype=BF16)
    ops.skinny_dgrad(dout, W, fresh, N, K, accumulate=False)           # overwrite form
    assert (fresh.float() - ref.float()).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item() + 1e-6


def test_skinny_linear_and_wgrad_vs_autograd():
    from mixgrpo_amd import ops
    Bn, N, K = 7, 3 * 3072, 3072
    g = torch.Generator(device="cuda").manual_seed(12)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
    b = torch.randn(N, device="cuda", generator=g).to(BF16)
    x = torch.randn(Bn, K, device="cuda", generator=g).to(BF16)
    out = torch.empty(Bn, N, device="cuda", dtype=BF16)
    ops.skinny_linear(x, W, b, out, N, K)
    want = (x.double() @ W.double().t() + b.double())
    assert (out.double() - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item() + 1e-6
    dout = torch.randn(Bn, N, device="cuda", generator=g).to(BF16)
    dW = torch.randn(N, K, device="cuda", generator=g) * 0.1
    db = torch.randn(N, device="cuda", generator=g) * 0.1
    dW0, db0 = dW.clone(), db.clone()
    ops.skinny_wgrad(dout, x, dW, db, N, K)
    assert torch.allclose(dW, dW0 + (dout.float().t() @ x.float()), rtol=1e-5, atol=1e-5)
    assert torch.allclose(db, db0 + dout.float().sum(0), rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- exact-grid edges
# Operands on a grid whose every partial sum is exact in fp32 (x, bias, dout: randint(-4, 5) / 8; W: randint(-2, 3) / 4; products
# are multiples of 1/32 with |sum| <= 768 / 4), so any split of K over the waves and any order give the fp64 result, and the
# one bf16 rounding of the output is the reference's.  Outputs are pre-filled with `helpers.sentinel`.
F32, I16 = torch.float32, torch.int16


SKINNY_LINEAR_CASES = [(1, 48, 32, True),        # one K-step: three of the four waves idle
                       (7, 40, 160, True),       # 5 K-steps split 2 / 2 / 1 / 0; N % 16 = 8: the row clamp and the n < N mask
                       (16, 16, 544, True),      # 17 steps: 160 per wave = the 128-step loop + the 32-step tail; row 15 stores
                       (17, 40, 256, True),      # the wrapper's chunks of 16 + 1 rows; K of the timestep embedding
                       (3, 24, 768, True),       # K of the pooled text projection
                       (7, 40, 160, False)]      # bias == NULL


@pytest.mark.parametrize("Bn,N,K,with_bias", SKINNY_LINEAR_CASES)
def test_skinny_linear_exact_on_the_grid(Bn, N, K, with_bias):
    from mixgrpo_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(Bn * 1000 + N + K)
    x, W = _grid((Bn, K), -4, 5, 8, gen), _grid((N, K), -2, 3, 4, gen)
    b = _grid((N,), -4, 5, 8, gen) if with_bias else None
    want = x.double() @ W.double().t()
    if with_bias:
        want = want + b.double()
    sent = _sentinel((Bn + 2, N))
    out = sent.clone()                                                  # over-allocated: rows >= Bn must stay as they are
    ops.skinny_linear(x, W, b, out, N, K)
    assert torch.equal(out[:Bn], want.to(BF16))
    assert torch.equal(out[Bn:].view(I16), sent[Bn:].view(I16))


def test_skinny_linear_on_column_slices():
    """x and out as column slices of wider buffers (row strides > K and > N): nothing outside the slice is written."""
    from mixgrpo_amd import ops
    Bn, N, K = 7, 40, 160
    gen = torch.Generator(device="cuda").manual_seed(21)
    xbig, W, b = _grid((Bn, K + 16), -4, 5, 8, gen), _grid((N, K), -2, 3, 4, gen), _grid((N,), -4, 5, 8, gen)
    x = xbig[:, 8:8 + K]                                                # 16-byte aligned rows, stride K + 16
    sent = _sentinel((Bn + 2, N + 11))
    obig = sent.clone()
    out = obig[:, 3:3 + N]
    assert x.stride(0) > K and out.stride(0) > N
    ops.skinny_linear(x, W, b, out, N, K)
    assert torch.equal(out[:Bn], (x.double() @ W.double().t() + b.double()).to(BF16))
    keep = torch.ones_like(sent, dtype=torch.bool)
    keep[:Bn, 3:3 + N] = False
    assert torch.equal(obig.view(I16)[keep], sent.view(I16)[keep])


SKINNY_WGRAD_CASES = [(1, 3, 4, True),           # one active thread in all
                      (7, 40, 1028, True),       # two column blocks, the second with one active thread
                      (16, 5, 2048, True),       # all 16 rows, two full column blocks
                      (17, 8, 1024, True),       # chunks of 16 + 1 rows: dW and dbias receive both
                      (7, 40, 1028, False)]      # dbias == NULL


@pytest.mark.parametrize("Bn,N,K,with_bias", SKINNY_WGRAD_CASES)
def test_skinny_wgrad_exact_on_the_grid(Bn, N, K, with_bias):
    from mixgrpo_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(Bn * 1000 + N + K)
    dout, x = _grid((Bn, N), -4, 5, 8, gen), _grid((Bn, K), -4, 5, 8, gen)
    dW0, db0 = _grid((N, K), -4, 5, 8, gen, dtype=F32), _grid((N,), -4, 5, 8, gen, dtype=F32)
    dW, db = dW0.clone(), db0.clone()
    ops.skinny_wgrad(dout, x, dW, db if with_bias else None, N, K)
    assert torch.equal(dW.double(), dW0.double() + dout.double().t() @ x.double())
    assert torch.equal(db.double(), db0.double() + (dout.double().sum(0) if with_bias else 0.0))
