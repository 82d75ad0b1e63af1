"""The VAE kernels at their edges: the implicit 3x3 convolution of csrc/gemm.hip (`mgx_conv3x3_nhwc`, `mgx_conv3x3s2_nhwc`),
GroupNorm, the row softmax and the copy / layout kernels of csrc/vae.hip, and `AutoencoderKL._attention` that sequences them,
against the plain fp64 references of tests/vae_refs.py.  The references and the premises of the bounds are checked on the CPU
in tests/test_vae_refs.py, which also proves through `mgx_gemm_plan` which kernel family every convolution case below runs.
The GPU tests carry `@gpu` one by one; the case lists and input builders are importable without a GPU.

CONVOLUTION: exact.  Image, bias and residual are randint(-4, 5) / 8, the weight randint(-2, 3) / 4.  With C <= 512 every
product is a multiple of 1/32 of magnitude <= 1/4 and every partial sum of the 9 C <= 4608 terms stays below 1152 = 36864 units
of 1/32 < 2^24: any summation order gives the fp64 sum in fp32, adding the bias (a multiple of 1/8) stays exact, and the one
bf16 rounding is the reference's.  The residual form is bf16(res + bf16(conv + bias)), again an exact fp32 sum.  So EVERY
element must equal the reference, in each of three launches over a pre-filled output (a stage overwritten early or a pipeline
that runs on across tiles shows in some launch, like tests/test_hip_gemm.py's integer-operand screen of the plain GEMM).

GROUPNORM bound, per element:  |got - ref| <= ulp_bf16(ref) + 2^-20 ((|x| + |mean|) rstd |gamma| + |beta|).
  With A = (|x| + |mean|) rstd |gamma| and u = 2^-24: the kernel forms t = (x - mean) rstd gamma + beta in fp32 from the
  fp32 roundings of the group's mean and rstd.  mean's rounding moves t by u |mean| rstd |gamma| <= u A, the subtraction rounds
  by u |x - mean| rstd |gamma| <= u A, rstd's rounding and the two products add 3 u |t - beta| <= 3 u A, the sum u |t|:
  under 6 u (A + |beta|) for exact statistics.  SiLU has slope <= 1.1 and its fast exponential a relative error of a few u:
  inside the same 2^-20 = 16 u.  What is left, about 10 u A, is the room of the statistics' own error where ref is near zero
  and its ulp is no help -- where beta cancels (x - mean) rstd gamma.  A relative error e_r of rstd moves t by e_r |t - beta|,
  and |t - beta| / A = |x - mean| / (|x| + |mean|) is z std / (2 mean) for x = mean + z std: e_r <= 20 u (mean / std) / z, with
  mean / std = 48 and z = 4 about 240 u.  The variance is E[x^2] - mean^2, so a relative error e of the sum of squares is
  e_r = e (1 + mean^2 / var) / 2 = 1152 e there: e <= u / 5.  The sums have to be right to fp32's last bit as a whole, which
  one fp32 chain over hundreds of rows is not, and which 64-row fp32 chains (exact: bf16 squares have 16 significant bits)
  folded into fp64 are.  So the issue's constant stands, and it is a demand on the kernel's sums.  The first term is the
  store's rounding (half an ulp) plus a flip where those errors carry t across a rounding boundary.  On the CPU
  (tests/test_vae_refs.py) torch's fp32 group_norm (+ silu) uses 0.50 of the bound -- the rounding alone -- and differs from
  bf16(ref) on at most 0.4 % of the elements.
  DIFFERING SHARE: the elements that differ at all from bf16(ref) stay below 0.02 (the bar of tests/test_hip_gemm.py for a bf16
  output of fp32 arithmetic), asserted for every case of at least 2048 elements and for all cases of one channel count taken
  together (in an 8-element case one legitimate flip is 12.5 %).
  MEASURED on an MI355X.  With stage-1 sums in fp32 over the whole 512-row slab (the kernel before these tests) C = 8 and
  C = 2048 failed: 9.0 % of the elements differed at C = 8, G = 1, 32 x 16 (the fp32 sum over the 256 rows of a pass), and
  3.83 bounds were used at C = 2048, G = 1, 73 x 7 (one fp32 chain of 511 rows per thread); C = 16 .. 1024 used 0.51 .. 0.55.
  With 64-row fp32 chains folded into fp64 every channel count uses 0.4997 .. 0.4999 of the bound -- the rounding alone -- and
  0.015 % .. 0.075 % of the elements differ.

SOFTMAX bound:  |P - ref| <= ulp_bf16(ref) + 2^-120: the fast exponential's relative error is about |arg| 2^-24, far under
  half a bf16 ulp; the floor covers flushed denormals.  Measured: at most 0.5005 of the bound, at every length.

ATTENTION: the restatement `vae_refs.attention_ref` rounds where the host code stores bf16.  cost = rel-L2 between it and the
  same computation with no rounding at all, measured on the CPU, is what one set of rounding points costs; the kernels differ
  from the restatement only by rounding flips and must stay within 2 cost.  Measured: cost 1.70e-3 .. 1.91e-3 over the cases;
  the kernels are 0 .. 8.0e-5 from the restatement (bit-identical at 8 x 8 x 64, 6 x 6 and 5 x 7; 99.93 % of the elements
  at the worst, 8 x 8 x 128).  H W % 4 != 0 is supported (5 x 7, 39 x 39); before, such a tile failed inside the GEMM entry
  with "N must be a multiple of 4"."""
import json
import os

import pytest
import torch

import vae_refs as R
from helpers import grid, sentinel

gpu = pytest.mark.gpu
BF16, F32, F64, I16 = torch.bfloat16, torch.float32, torch.float64, torch.int16
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to vae_kernels.json in that directory

# ---- convolution cases (H, W, C, Cout, ld_out); tests/test_vae_refs.py asserts the kernel family of each
CONV_PERSISTENT = [(128, 128, 64, 512, 512),      # exactly 128 tiles; 9 K-tiles: an odd ring position
                   (130, 127, 128, 512, 512),     # M = 16510: last tile row 126 rows deep, no image row aligned to a tile; 130 tiles
                   (176, 192, 64, 512, 512),      # 264 tiles > the launch's workgroups: a workgroup runs on into a second tile
                   (128, 128, 256, 512, 512),     # conv_shift 2
                   (128, 128, 512, 512, 512),     # conv_shift 3
                   (130, 127, 128, 512, 516)]     # ld_out = Cout + 4: the generic 8-byte epilogue inside the persistent kernel
CONV_PERSISTENT_S2 = [(256, 256, 64, 512, 512), (260, 254, 128, 512, 512)]                  # M = 128 * 128 and 130 * 127
CONV_SMALL = [(1, 1, 64, 4, 8),                   # every tap but the centre on the border
              (3, 1, 128, 8, 8),
              (24, 20, 128, 64, 64),
              (17, 23, 512, 132, 132),            # a ragged N tile
              (32, 32, 128, 4, 8)]                # conv_out: columns 4 .. 7 keep their bits
CONV_SMALL_S2 = [(2, 2, 64, 4, 8), (40, 72, 128, 128, 128)]
LAUNCHES = 3

# ---- GroupNorm cases
GN_CHANNELS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)                      # every channel count the entry accepts
GN_IMAGES = ((1, 1), (2, 1), (73, 7), (32, 16), (27, 19), (41, 25), (10, 10))  # M = 1, 2, 511, 512, 513, 1025 around GN_ROWS = 512
# (512 has no divisor that is not a power of two, 1 and 2 none but themselves; 10 x 10 is below rpp = 256 at C = 8)
GN_PROFILES = ((0.5, 2.0), (6.0, 0.25), (-3.0, 0.125), (12.0, 0.25))           # (mean, std) of a group; bf16 resolves all four
GN_SECOND_PASS = (264, 512, 64)                                                # 264 * 512 * 64 / 8 > 2^20: gn_apply's second grid pass
GN_SHARE = 0.02

SOFTMAX_LENGTHS = (1, 63, 64, 255, 256, 257, 1000, 4099, 16384)                # 64 registers x 256 threads: around 256 k, and full
SOFTMAX_SCALES = (0.25, 512 ** -0.5, 1.0)
SOFTMAX_AMPS = (5.0, 20.0, 50.0)

ATTN_CASES = [(64, 8, 8), (128, 8, 8), (64, 20, 28), (128, 20, 28), (64, 6, 6), (128, 6, 6)]   # (C, H, W): M = 64, 560 (padded P), 36
ATTN_ODD = [(64, 5, 7), (64, 39, 39)]                                           # H W % 4 != 0: S's columns and the k rows padded


def _record(**kw):
    for k, v in kw.items():
        print(f"{k}: {v}")
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "vae_kernels.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d.update(kw)
    json.dump(d, open(path, "w"), indent=1)


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(I16), b.contiguous().view(I16))


def gn_groups(C):
    return sorted({1, C} | ({32} if C % 32 == 0 else set()))


def gn_inputs(M, C, G, k, device, seed=0):
    """x [M, C] bf16 whose group g has the mean and the spread of GN_PROFILES[(g + k) % 4]; gamma, beta [C] bf16."""
    g = _gen(1000 * seed + 7 * C + M + G, device)
    prof = torch.tensor([GN_PROFILES[(i + k) % 4] for i in range(G)], device=device)
    mu, sd = (prof[:, j].repeat_interleave(C // G) for j in (0, 1))
    x = (torch.randn(M, C, generator=g, device=device) * sd + mu).to(BF16)
    gamma = (1 + 0.2 * torch.randn(C, generator=g, device=device)).to(BF16)
    beta = (0.1 * torch.randn(C, generator=g, device=device)).to(BF16)
    return x, gamma, beta


def gn_judge(got, ref, bound):
    """(largest share of the bound used, share of elements that differ from bf16(ref), their number)"""
    used = ((got.to(F64) - ref).abs() / bound).max().item()
    differ = (got != ref.to(F32).to(BF16)).sum().item()
    return used, differ / got.numel(), differ


def softmax_rows_input(n, amp, device, seed=0):
    """S fp32 [4, n]: a random row, a row with -inf entries (n > 1), a row of equal values, a second random row."""
    g = _gen(seed + n, device)
    S = torch.randn(4, n, generator=g, device=device) * amp
    if n > 1:
        S[1, torch.randperm(n, generator=g, device=device)[:max(1, n // 3)]] = float("-inf")
    S[2] = 1.75
    return S


# ------------------------------------------------------------------------------------------------------------ convolution
def _conv_operands(H, W, C, Cout, stride, seed):
    g = _gen(seed, "cuda")
    xpad = torch.zeros(H + 2, W + 2, C, dtype=BF16, device="cuda")
    xpad[1:-1, 1:-1] = grid((H, W, C), -4, 5, 8, g)
    if stride == 2:                                   # the top and left border are never read: no output may see them
        xpad[0] = float("nan")
        xpad[:, 0] = float("nan")
    wt = grid((Cout, 3, 3, C), -2, 3, 4, g)
    bias = torch.zeros(Cout + 8, dtype=BF16, device="cuda")
    bias[:Cout] = grid((Cout,), -4, 5, 8, g)
    M = H * W if stride == 1 else (H // 2) * (W // 2)
    res = grid((M, Cout), -4, 5, 8, g)
    return xpad, wt, bias, res, M


def _assert_all_equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {bad.sum().item()} of {bad.numel()} elements differ, first at {idx[0].tolist()} "
                             f"(got {got[tuple(idx[0])].item()}, want {want[tuple(idx[0])].item()}), last at {idx[-1].tolist()}")


def _run_conv(H, W, C, Cout, ld, stride):
    from mixgrpo_amd import ops
    xpad, wt, bias, res, M = _conv_operands(H, W, C, Cout, stride, seed=H * W + C + Cout + ld)
    want = R.conv3x3_ref_bf16(xpad, wt, bias, H, W, stride)
    fill = sentinel((M, ld))
    for launch in range(LAUNCHES):
        out = fill.clone()
        if stride == 1:
            ops.conv3x3(xpad, wt, bias, out, H, W, C, Cout, ld_out=ld)
        else:
            ops.conv3x3s2(xpad, wt, bias, out, H, W, C, Cout, ld_out=ld)
        _assert_all_equal(out[:, :Cout], want, f"launch {launch}")
        assert _bits_equal(out[:, Cout:], fill[:, Cout:]), f"launch {launch}: spare columns written"
    if stride == 1 and Cout >= 8:                                                               # residual form: out += conv
        want2 = R.conv3x3_ref_bf16(xpad, wt, bias, H, W, stride, res=res)
        ones = torch.ones(Cout + 8, dtype=BF16, device="cuda")
        for launch in range(LAUNCHES):
            out = fill.clone()
            out[:, :Cout] = res
            ops.conv3x3(xpad, wt, bias, out, H, W, C, Cout, ones=ones, ld_out=ld)
            _assert_all_equal(out[:, :Cout], want2, f"residual launch {launch}")
            assert _bits_equal(out[:, Cout:], fill[:, Cout:]), f"residual launch {launch}: spare columns written"


@gpu
@pytest.mark.parametrize("H,W,C,Cout,ld", CONV_PERSISTENT + CONV_SMALL)
def test_conv3x3_every_element_exact(H, W, C, Cout, ld):
    _run_conv(H, W, C, Cout, ld, 1)


@gpu
@pytest.mark.parametrize("H,W,C,Cout,ld", CONV_PERSISTENT_S2 + CONV_SMALL_S2)
def test_conv3x3_stride2_every_element_exact(H, W, C, Cout, ld):
    _run_conv(H, W, C, Cout, ld, 2)


# -------------------------------------------------------------------------------------------------------------- GroupNorm
def _run_gn(x, gamma, beta, H, W, C, G, silu, padded, ld):
    """One launch -> the interior [M, C]; the input a column slice when ld > C; a padded output's border must keep its bits."""
    from mixgrpo_amd import ops
    M = H * W
    if ld > C:
        wide = sentinel((M, ld))
        wide[:, :C] = x
        xin = wide[:, :C]
    else:
        xin = x
    if padded:
        fill = sentinel((H + 2, W + 2, C))
        out = fill.clone()
    else:
        out = torch.full((M, C), float("nan"), dtype=BF16, device="cuda")
    ops.group_norm(xin, gamma, beta, out, H, W, C, G, silu, padded, ld=ld if ld > C else None)
    if not padded:
        return out
    keep = torch.ones(H + 2, W + 2, dtype=torch.bool, device="cuda")
    keep[1:-1, 1:-1] = False
    assert _bits_equal(out[keep], fill[keep]), "border written"
    return out[1:-1, 1:-1].reshape(M, C)


@gpu
@pytest.mark.parametrize("C", GN_CHANNELS)
def test_group_norm_every_shape_within_the_bound(C):
    used_max, differ_all, count_all, k = 0.0, 0, 0, 0
    for G in gn_groups(C):
        for H, W in GN_IMAGES:
            M = H * W
            x, gamma, beta = gn_inputs(M, C, G, k, "cuda")
            # plain output from a column slice (ld = C + 8), and the padded output; SiLU on alternately
            for silu, padded, ld in ((k % 2 == 1, False, C + 8), (k % 2 == 0, True, C)):
                ref, bound = R.group_norm_ref(x, gamma, beta, G, silu)
                got = _run_gn(x, gamma, beta, H, W, C, G, silu, padded, ld)
                used, share, differ = gn_judge(got, ref, bound)
                assert used <= 1.0, (C, G, H, W, silu, padded, used)
                assert M * C < 2048 or share < GN_SHARE, (C, G, H, W, silu, padded, share)
                used_max, differ_all, count_all = max(used_max, used), differ_all + differ, count_all + M * C
            k += 1
    _record(**{f"group_norm_C{C}": {"bound_used": round(used_max, 4), "differing_share": round(differ_all / count_all, 6)}})
    assert differ_all / count_all < GN_SHARE


@gpu
def test_group_norm_second_grid_pass():
    H, W, C = GN_SECOND_PASS
    assert H * W * C // 8 > 4096 * 256                                   # more work items than the capped grid has threads
    x, gamma, beta = gn_inputs(H * W, C, 32, 1, "cuda")
    ref, bound = R.group_norm_ref(x, gamma, beta, 32, True)
    got = _run_gn(x, gamma, beta, H, W, C, 32, True, True, C)
    used, share, _ = gn_judge(got, ref, bound)
    _record(group_norm_second_pass={"bound_used": round(used, 4), "differing_share": round(share, 6)})
    assert used <= 1.0 and share < GN_SHARE, (used, share)


@gpu
@pytest.mark.parametrize("C", (8, 64, 2048))
def test_group_norm_constant_groups_give_exactly_the_bias(C):
    """Every group constant (var = 0): sums of n copies of c and of c^2 are exact (n c^2 < 2^24 units of its last bit for the
    512 rows of a block), so mean = c, var = 0 and the output is bf16([silu](beta)) exactly."""
    H, W = 27, 19
    consts = torch.tensor([3.09375, -0.4375, 12.0, 0.0], device="cuda")
    for G in gn_groups(C):
        _, gamma, beta = gn_inputs(H * W, C, G, 0, "cuda")
        x = consts[torch.arange(G, device="cuda") % 4].repeat_interleave(C // G).expand(H * W, C).to(BF16).contiguous()
        for silu in (False, True):
            b = beta.to(F64)
            want = ((b * torch.sigmoid(b)) if silu else b).to(F32).to(BF16).expand(H * W, C)
            for padded in (False, True):
                got = _run_gn(x, gamma, beta, H, W, C, G, silu, padded, C)
                _assert_all_equal(got, want, f"C {C} G {G} silu {silu} padded {padded}")


# ---------------------------------------------------------------------------------------------------------------- softmax
def _softmax(S, n, scale, lds, ldp):
    """The entry called on S [4, lds] / P [4, ldp] with row length n; P pre-filled with the sentinel."""
    from mixgrpo_amd import _lib
    fill = sentinel((S.shape[0], ldp))
    P = fill.clone()
    _lib.check(_lib.lib().mgx_softmax_rows_f32(S.data_ptr(), lds, P.data_ptr(), ldp, S.shape[0], n, scale, _lib.stream()))
    assert _bits_equal(P[:, n:], fill[:, n:]), "spare columns written"
    return P[:, :n]


@gpu
@pytest.mark.parametrize("n", SOFTMAX_LENGTHS)
def test_softmax_rows_within_one_ulp(n):
    used_max = 0.0
    for i, scale in enumerate(SOFTMAX_SCALES):
        amp = SOFTMAX_AMPS[(i + n) % 3]
        S = softmax_rows_input(n, amp, "cuda", seed=i)
        wide = torch.full((4, n + 3), float("nan"), device="cuda")           # S.stride(0) > n; the spare columns poison a read
        wide[:, :n] = S
        for lds, ldp, src in ((n + 3, n + 5, wide), (n, n, S.contiguous())):
            got = _softmax(src, n, scale, lds, ldp)
            ref = R.softmax_ref(S, scale)
            used = ((got.to(F64) - ref).abs() / R.softmax_bound(ref)).max().item()
            used_max = max(used_max, used)
            assert used <= 1.0, (n, scale, amp, used)
            assert (got.view(I16)[S == float("-inf")] == 0).all()           # exact zeros where the input is -inf
            _assert_all_equal(got[2], torch.full((n,), 1.0 / n, dtype=F64).to(F32).to(BF16).cuda(), "row of equal values")
    _record(**{f"softmax_n{n}": {"bound_used": round(used_max, 4)}})


@gpu
def test_softmax_rows_refuses_a_row_longer_than_its_registers():
    from mixgrpo_amd import _lib, ops
    S = torch.zeros(1, 16385, device="cuda")
    fill = sentinel((1, 16385))
    P = fill.clone()
    with pytest.raises(_lib.MgxError, match="16384"):
        ops.softmax_rows(S, P, 1, 16385, 1.0)
    assert _bits_equal(P, fill)


# ------------------------------------------------------------------------------------------- copy and layout kernels
@gpu
@pytest.mark.parametrize("H,W,C", [(264, 256, 64), (3, 5, 8)])           # 4 * 264 * 256 * 64 / 8 > 2^20 work items; tiny and ragged
def test_upsample2x_pad_bit_for_bit(H, W, C):
    from mixgrpo_amd import ops
    x = R.random_bits((H * W, C), _gen(H + C, "cpu"), "cuda")
    want = sentinel((2 * H + 2, 2 * W + 2, C))
    out = want.clone()
    want[1:-1, 1:-1] = x.view(H, W, C).repeat_interleave(2, 0).repeat_interleave(2, 1)
    ops.upsample2x_pad(x, out, H, W, C)
    assert _bits_equal(out, want)


@gpu
@pytest.mark.parametrize("H,W,C,ld", [(264, 512, 64, 72), (5, 7, 8, 24)])
def test_pad_nhwc_bit_for_bit(H, W, C, ld):
    from mixgrpo_amd import ops
    x = R.random_bits((H * W, ld), _gen(H + ld, "cpu"), "cuda")
    want = sentinel((H + 2, W + 2, C))
    out = want.clone()
    want[1:-1, 1:-1] = x[:, :C].reshape(H, W, C)
    ops.pad_nhwc(x, ld, out, H, W, C)
    assert _bits_equal(out, want)


@gpu
@pytest.mark.parametrize("Cin,H,W,C", [(16, 264, 256, 64), (3, 5, 7, 8)])
def test_latents_to_pad_bit_for_bit(Cin, H, W, C):
    """fp32 -> bf16, round to nearest even: half the values random, half on a grid of 17 significant bits, where ties occur."""
    from mixgrpo_amd import ops
    g = _gen(H + Cin, "cpu")
    z = torch.randn(Cin, H, W, generator=g) * 3
    tie = torch.randint(-(1 << 16), 1 << 16, (Cin, H, W), generator=g).float() / 256
    z = torch.where(torch.rand(Cin, H, W, generator=g) < 0.5, z, tie).cuda()
    want = sentinel((H + 2, W + 2, C))
    out = want.clone()
    want[1:-1, 1:-1, :Cin] = z.permute(1, 2, 0).to(BF16)                  # borders and the spare channels keep their bits
    ops.latents_to_pad(z, out, Cin, H, W, C)
    assert _bits_equal(out, want)


@gpu
@pytest.mark.parametrize("H,W,Cout,ld", [(600, 600, 3, 8), (5, 7, 3, 8), (3, 5, 4, 12)])
def test_nhwc_to_image_bit_for_bit(H, W, Cout, ld):
    from mixgrpo_amd import ops
    x = R.random_bits((H * W, ld), _gen(H + ld, "cpu"), "cuda")
    img = sentinel((Cout, H, W))
    ops.nhwc_to_image(x, ld, img, Cout, H, W)
    assert _bits_equal(img, x[:, :Cout].t().reshape(Cout, H, W))


@gpu
def test_diag_gaussian_second_grid_pass_and_nan_logvar():
    """H W Cz > 2^20, held to the bounds of tests/test_hip_vae_encoder.py: the mean a copy, std within one bf16 ulp of the
    host's, the sample within one ulp at the magnitude of its larger term.  A NaN logvar gives a NaN std and sample, there only."""
    import vae_encoder_ref as ER
    from mixgrpo_amd import ops
    H, W, Cz, ld = 264, 256, 16, 40
    assert H * W * Cz > 4096 * 256
    g = _gen(5, "cpu")
    mom = torch.randn(H * W, ld, generator=g)
    mom[:, Cz:2 * Cz] *= 4.0
    mom[::1001, Cz + 3] = -40.0
    mom[7::1003, 2 * Cz - 1] = 25.0
    mom = mom.to(BF16)
    nan_at = (H * W - 5, 9)                                                # (pixel, channel), reached in the last grid pass
    mom[nan_at[0], Cz + nan_at[1]] = float("nan")
    noise = torch.randn(Cz, H, W, generator=g).to(BF16)
    nchw = mom[:, :2 * Cz].reshape(H, W, 2 * Cz).permute(2, 0, 1).contiguous()
    w_mean, w_std, w_sample = ER.gaussian(nchw, noise)
    mean, std, sample = (sentinel((Cz, H, W)) for _ in range(3))
    ops.diag_gaussian(mom.cuda(), ld, noise.cuda(), mean, std, sample, Cz, H, W)
    mean, std, sample = mean.cpu(), std.cpu(), sample.cpu()
    assert _bits_equal(mean, w_mean)
    isnan = torch.zeros(Cz, H * W, dtype=torch.bool)
    isnan[nan_at[1], nan_at[0]] = True
    isnan = isnan.view(Cz, H, W)
    assert torch.equal(torch.isnan(std), isnan) and torch.equal(torch.isnan(sample), isnan)
    assert torch.equal(torch.isnan(w_std), isnan)
    ok = ~isnan
    assert torch.isfinite(std[ok]).all() and torch.isfinite(sample[ok]).all()
    d_std = (R.ordinal(std) - R.ordinal(w_std))[ok].abs().max().item()
    prod = (w_std.float() * noise.float()).abs()
    ulp = 2.0 ** (torch.floor(torch.log2(torch.maximum(torch.maximum(prod, w_sample.float().abs()), torch.tensor(1e-30)))) - 7)
    d_sample = ((sample.float() - w_sample.float()).abs() / ulp)[ok].max().item()
    _record(diag_gaussian_second_pass={"std_ulps": d_std, "sample_ulps": round(d_sample, 3)})
    assert d_std <= 1 and d_sample <= 1.0


# ------------------------------------------------------------------------------------------------- mid-block attention
def attention_input(C, H, W):
    """A random bf16 activation [H W, C] (on the host: the CPU premise test measures the same tensors)."""
    g = _gen(C + 31 * H + W, "cpu")
    return (torch.randn(H * W, C, generator=g) * 1.5 + 0.25).to(BF16)


def attention_cost(C, H, W):
    """(x, weights, the restatement's output, cost): cost = rel-L2 between the restatement with its bf16 rounding points and the
    same fp64 computation without any."""
    x, P = attention_input(C, H, W), R.attention_weights(C, seed=C + H)
    rounded = R.attention_ref(x, P, C, 32, True)
    return x, P, rounded, R.rel_l2(rounded, R.attention_ref(x, P, C, 32, False))


def _attention_on_the_kernels(x, P, C, H, W):
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    m = AutoencoderKL(VaeConfig(block_out_channels=(C,), norm_num_groups=32), device="cuda")
    m.P = {"a." + k: v.cuda() for k, v in P.items()}
    return m._attention("a", x.clone().cuda(), H, W, C).cpu()


@gpu
@pytest.mark.parametrize("C,H,W", ATTN_CASES + ATTN_ODD)
def test_mid_block_attention_within_twice_its_rounding_cost(C, H, W):
    """H W % 4 != 0 (ATTN_ODD) is supported: `_attention` pads S's columns and the k rows to a multiple of 4."""
    x, P, want, cost = attention_cost(C, H, W)
    got = _attention_on_the_kernels(x, P, C, H, W)
    rel = R.rel_l2(got, want)
    _record(**{f"attention_C{C}_{H}x{W}": {"rounding_cost_rel_l2": cost, "kernels_vs_restatement_rel_l2": rel,
                                           "bit_equal_share": (got == want).float().mean().item()}})
    assert got.dtype == BF16 and torch.isfinite(got.float()).all()
    assert rel <= 2 * cost, (rel, cost)


@gpu
def test_mid_block_attention_refuses_more_tokens_than_a_softmax_row():
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    m = AutoencoderKL(VaeConfig(block_out_channels=(64,)), device="cuda")
    m.P = {}
    with pytest.raises(ValueError, match="16384 tokens"):
        m._attention("a", torch.zeros(129 * 128, 64, dtype=BF16, device="cuda"), 129, 128, 64)
