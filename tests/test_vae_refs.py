"""CPU checks of tests/vae_refs.py and of the premises tests/test_hip_vae_kernels.py rests on: the references against torch's
own operators in double, the exact-sum premise of the convolution operands, the kernel family of every convolution case
(through the host query `mgx_gemm_plan`, without a GPU), and that a plain fp32 evaluation of GroupNorm, the softmax and the
attention stays inside the bounds the kernels are held to.  The measured shares are printed (pytest -s)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import test_hip_vae
import test_hip_vae_encoder
import test_hip_vae_kernels as K
import vae_refs as R
from helpers import grid, sentinel

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ helpers
def test_ulp_and_ordinal():
    v = torch.tensor([1.0, 1.5, 2.0, -3.0, 0.75, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=F64)
    assert R.ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8] + [2.0 ** -133] * 3
    b = torch.tensor([1.0, 1.0078125, -1.0, -1.0078125, 0.0, -0.0], dtype=BF16)
    o = R.ordinal(b)
    assert o[1] - o[0] == 1 and o[3] - o[2] == -1 and o[4] == o[5] == 0
    bits = R.random_bits((4096,), _gen(0))
    assert torch.isnan(bits).any() and (bits.float().abs() < 2.0 ** -126).any() and bits.view(torch.int16).unique().numel() > 3000


def test_sentinel_is_no_value_of_a_grid():
    s = sentinel((300,), device="cpu").float()
    assert (s != 0).all() and s.abs().max().item() < 2.0 ** -120                  # tiny: no multiple of 1/8 or 1/4


# ------------------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("H,W,C,Cout", [(1, 1, 8, 4), (3, 1, 8, 4), (5, 7, 16, 12), (8, 6, 8, 4)])
def test_im2col_reference_is_conv2d_in_double(H, W, C, Cout):
    g = _gen(H + W)
    x = torch.randn(C, H, W, generator=g, dtype=F64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=F64)
    b = torch.randn(Cout, generator=g, dtype=F64)
    xpad = torch.zeros(H + 2, W + 2, C, dtype=F64)
    xpad[1:-1, 1:-1] = x.permute(1, 2, 0)
    wt = w.permute(0, 2, 3, 1).contiguous()
    want = F.conv2d(x[None], w, b, padding=1)[0].permute(1, 2, 0).reshape(H * W, Cout)
    assert torch.allclose(R.conv3x3_ref(xpad, wt, b, H, W, 1, chunk_rows=2 * W), want, rtol=1e-12, atol=1e-12)
    if H % 2 == 0 and W % 2 == 0:
        xpad[0], xpad[:, 0] = float("nan"), float("nan")                           # stride 2 never reads the top / left border
        want = F.conv2d(F.pad(x[None], (0, 1, 0, 1)), w, b, stride=2)[0].permute(1, 2, 0).reshape(H * W // 4, Cout)
        assert torch.allclose(R.conv3x3_ref(xpad, wt, b, H, W, 2, chunk_rows=W), want, rtol=1e-12, atol=1e-12)


def test_grid_operands_sum_exactly_in_fp32_in_any_order():
    """The premise of the exact convolution tests, at the largest K = 9 * 512: magnitudes, and a forward, a backward and a
    pairwise fp32 summation of the same products all equal to the fp64 sum."""
    assert 9 * 512 * (4 / 8) * (2 / 4) == 1152 and 1152 * 32 < 2 ** 24
    g = _gen(1)
    a = grid((64, 4608), -4, 5, 8, g, device="cpu").float()
    w = grid((64, 4608), -2, 3, 4, g, device="cpu").float()
    assert a.abs().max() == 0.5 and w.abs().max() == 0.5
    prod = a * w
    assert torch.equal(prod.double(), a.double() * w.double()) and torch.equal(prod * 32, (prod * 32).round())
    want = prod.double().sum(1)
    for order in (prod, prod.flip(1)):
        acc = torch.zeros(64)
        for j in range(order.shape[1]):
            acc = acc + order[:, j]
        assert torch.equal(acc.double(), want)
    assert torch.equal(prod.view(64, 72, 64).sum(2).sum(1).double(), want)
    bias = grid((64,), -4, 5, 8, g, device="cpu").float()
    assert torch.equal((want.float() + bias).double(), want + bias.double())
    y = (want.float() + bias).to(BF16)
    res = grid((64,), -4, 5, 8, g, device="cpu")
    assert torch.equal((res.float() + y.float()).double(), res.double() + y.double())          # the residual sum, before its rounding
    assert (y.float() != want.float() + bias).any()                                           # and bf16 does round these sums


def _plan(M, N, Kdim):
    from mixgrpo_amd import _lib
    out = (ctypes.c_int * 6)()
    assert _lib.lib().mgx_gemm_plan(M, N, Kdim, 0, out, 6) == 6, (M, N, Kdim)
    return dict(zip(("family", "grid", "band", "minparts", "nfix", "xcds"), out))


def test_every_convolution_case_runs_the_kernel_family_it_is_there_for():
    """family 1 = the persistent 256x256 kernel, 0 = the 128x128 kernel, as launch() decides for M = the output pixels,
    N = Cout, K = 9 C (the convolution entries pass span32 = 1, which the query derives as true for these sizes too)."""
    for H, W, C, Cout, _ in K.CONV_PERSISTENT:
        p = _plan(H * W, Cout, 9 * C)
        assert p["family"] == 1, (H, W, C, Cout)
    for H, W, C, Cout, _ in K.CONV_PERSISTENT_S2:
        assert _plan(H * W // 4, Cout, 9 * C)["family"] == 1, (H, W, C, Cout)
    for H, W, C, Cout, _ in K.CONV_SMALL:
        assert _plan(H * W, Cout, 9 * C)["family"] == 0, (H, W, C, Cout)
    for H, W, C, Cout, _ in K.CONV_SMALL_S2:
        assert _plan(H * W // 4, Cout, 9 * C)["family"] == 0, (H, W, C, Cout)
    tiles = {(H, W, C): math.ceil(H * W / 256) * math.ceil(Cout / 256) for H, W, C, Cout, _ in K.CONV_PERSISTENT}
    assert tiles[(128, 128, 64)] == 128 and tiles[(130, 127, 128)] == 130 and tiles[(176, 192, 64)] == 264
    assert 130 * 127 % 256 == 126 and all((r * 127) % 256 for r in range(1, 130))             # no image row starts a tile
    p = _plan(176 * 192, 512, 9 * 64)
    assert p["grid"] < tiles[(176, 192, 64)] and p["nfix"] == 0                                # a workgroup takes a second tile
    assert {C for _, _, C, _, _ in K.CONV_PERSISTENT} == {64, 128, 256, 512}                   # conv_shift 0 .. 3
    assert any(ld % 8 for _, _, _, _, ld in K.CONV_PERSISTENT)                                 # rowwise_ok = 0 in one case


def test_family_of_the_existing_convolution_cases():
    """What the random-data cases of tests/test_hip_vae.py and tests/test_hip_vae_encoder.py run: of the stride-1 cases none
    reaches the persistent kernel (128 tiles of 256 x 256 are its threshold); of the stride-2 cases the last one does."""
    cases = test_hip_vae.test_conv3x3_implicit_gemm_vs_torch.pytestmark[0].args[1]
    assert (128, 128, 256, 256) in cases and (64, 128, 512, 512) in cases and len(cases) == 5
    for H, W, C, Cout in cases:
        assert _plan(H * W, (Cout + 3) // 4 * 4, 9 * C)["family"] == 0, (H, W, C, Cout)
    assert math.ceil(128 * 128 / 256) * 1 == 64 and math.ceil(64 * 128 / 256) * 2 == 64
    s2 = test_hip_vae_encoder.test_conv3x3_stride2_vs_torch.pytestmark[0].args[1]
    assert [_plan(H * W // 4, Cout, 9 * C)["family"] for H, W, C, Cout in s2] == [0, 0, 0, 1]


# -------------------------------------------------------------------------------------------------------------- GroupNorm
def test_group_norm_reference_is_torch_group_norm_in_double():
    for M, C, G, silu in ((7, 8, 1, False), (30, 64, 32, True), (513, 16, 16, True)):
        x, gamma, beta = K.gn_inputs(M, C, G, 1, "cpu")
        want = F.group_norm(x.double().t().reshape(1, C, M, 1), G, gamma.double(), beta.double(), eps=1e-6)
        want = (F.silu(want) if silu else want)[0, :, :, 0].t()
        ref, bound = R.group_norm_ref(x, gamma, beta, G, silu)
        assert torch.allclose(ref, want, rtol=1e-9, atol=1e-9)
        assert (bound >= R.ulp_bf16(ref)).all()


def test_fp32_group_norm_stays_inside_the_bound():
    """torch's fp32 group_norm (+ silu), rounded to bf16, on the GPU test's inputs -- groups with mean 12 and std 1/4 among them:
    at most 0.52 of the bound (the store's rounding is 0.50 of it) and a differing share far under 0.02."""
    used_max, share_max = 0.0, 0.0
    k = 0
    for C in (8, 64, 256, 2048):
        for G in K.gn_groups(C):
            for H, W in ((73, 7), (27, 19), (41, 25)):
                M = H * W
                x, gamma, beta = K.gn_inputs(M, C, G, k, "cpu")
                silu = k % 2 == 0
                t = F.group_norm(x.float().t().reshape(1, C, M, 1), G, gamma.float(), beta.float(), eps=1e-6)
                got = (F.silu(t) if silu else t)[0, :, :, 0].t().to(BF16)
                used, share, _ = K.gn_judge(got, *R.group_norm_ref(x, gamma, beta, G, silu))
                used_max, share_max = max(used_max, used), max(share_max, share)
                k += 1
    print(f"fp32 group_norm: {used_max:.3f} of the bound, differing share at most {share_max:.5f}")
    assert used_max <= 0.52 and share_max < K.GN_SHARE


def test_group_norm_cases_cover_the_entry():
    assert [C for C in range(8, 2049, 8) if 256 % (C // 8) == 0] == list(K.GN_CHANNELS)         # what the entry accepts
    assert {256 // (C // 8) for C in K.GN_CHANNELS} == {256, 128, 64, 32, 16, 8, 4, 2, 1}        # rows per pass
    Ms = [H * W for H, W in K.GN_IMAGES]
    assert Ms[:6] == [1, 2, 511, 512, 513, 1025] and Ms[6] < 256
    assert all(W & (W - 1) for H, W in K.GN_IMAGES if H * W not in (1, 2, 512))                  # W no power of two where M allows
    assert K.gn_groups(8) == [1, 8] and K.gn_groups(64) == [1, 32, 64]
    for mean, std in K.GN_PROFILES:                                                               # bf16 resolves every profile
        assert std / R.ulp_bf16(torch.tensor(abs(mean), dtype=F64)).item() >= 4


# ---------------------------------------------------------------------------------------------------------------- softmax
def test_fp32_softmax_stays_within_one_ulp_at_every_length():
    used_max = 0.0
    for n in K.SOFTMAX_LENGTHS:
        for i, scale in enumerate(K.SOFTMAX_SCALES):
            S = K.softmax_rows_input(n, K.SOFTMAX_AMPS[(i + n) % 3], "cpu", seed=i)
            ref = R.softmax_ref(S, scale)
            got = torch.softmax(S * torch.tensor(scale, dtype=F32), -1).to(BF16)
            used_max = max(used_max, ((got.double() - ref).abs() / R.softmax_bound(ref)).max().item())
            assert (got[S == float("-inf")] == 0).all() and (ref[S == float("-inf")] == 0).all()
            assert torch.allclose(ref.sum(-1), torch.ones(4, dtype=F64))
            assert torch.equal(ref[2].to(F32).to(BF16), torch.full((n,), 1.0 / n, dtype=F64).to(F32).to(BF16))
    print(f"fp32 softmax: {used_max:.3f} of the bound")
    assert used_max <= 1.0


def test_one_over_n_is_far_from_a_bf16_rounding_boundary():
    """A row of n equal values gives bf16(1 / n) whatever the last bits of the fp32 reciprocal: fp32(1 / n) moved by four fp32
    ulps either way rounds to the same bf16 value, for every tested length."""
    for n in K.SOFTMAX_LENGTHS:
        r = torch.tensor(1.0 / n, dtype=F64).to(F32)
        near = (r.view(torch.int32) + torch.arange(-4, 5, dtype=torch.int32)).view(F32)
        assert (near.to(BF16) == r.to(BF16)).all(), n


# -------------------------------------------------------------------------------------------------------------- attention
def test_attention_restatement_is_scaled_dot_product_attention_in_double():
    C, H, W = 64, 5, 6
    x, P = K.attention_input(C, H, W), R.attention_weights(C, seed=1)
    w = {k: v.double() for k, v in P.items()}
    n = F.group_norm(x.double().t().reshape(1, C, H * W, 1), 32, w["group_norm.weight"], w["group_norm.bias"], eps=1e-6)
    n = n[0, :, :, 0].t()
    q, k, v = (n @ w[f"to_{c}.weight"].t() + w[f"to_{c}.bias"] for c in "qkv")
    o = F.scaled_dot_product_attention(q[None], k[None], v[None])[0]
    want = x.double() + o @ w["to_out.0.weight"].t() + w["to_out.0.bias"]
    assert torch.allclose(R.attention_ref(x, P, C, 32, False), want, rtol=1e-9, atol=1e-9)
    rounded = R.attention_ref(x, P, C, 32, True)
    assert rounded.dtype == BF16 and R.rel_l2(rounded, want) < 1e-2


def test_attention_rounding_cost():
    """What one set of bf16 rounding points costs, per case: the GPU test allows the kernels twice this."""
    for C, H, W in K.ATTN_CASES + K.ATTN_ODD[:1]:
        cost = K.attention_cost(C, H, W)[3]
        print(f"attention C {C} {H}x{W}: rounding cost rel-L2 {cost:.3e}")
        assert 1e-4 < cost < 1e-2                                                 # a bf16 rounding is 2^-9 relative at the most
