"""The hand-over between output tiles of the persistent GEMM (csrc/gemm.hip gemm_pp_kernel): the epilogue of one tile, its
stores, the look-ahead and the first waits of the next tile -- held BIT FOR BIT against CPU references on exactly representable
operands (small integers / 8 and / 4: every product and every partial sum is a multiple of 1/32 far below 2^24 / 32, so the
fp32 sums are exact whatever the summation order, and every later step is a correctly rounded IEEE operation that torch
restates on the CPU).

Shapes: M = 256 * 24 + 128 (the last tile row half outside), N = 8192 / 8200 / 8196 (16-byte paths; N % 8 == 4: the generic
path): 800 - 825 tiles on 256 workgroups, so every workgroup walks at least 3 tiles and hands over at least twice; K = 128, 192,
320 = 2, 3, 5 K-tiles, so the three A stages and two W stages cross the tile boundaries in every phase of their rotation.
C and aux carry guard rows and columns, which have to stay untouched."""
import ctypes
import functools

import pytest
import torch

from helpers import GCOLS, exact_gemm_problem
from helpers import GuardedOut as _Out, grid_ints as _ints, linear_ref as _y_ref, same_bits as _same_bits

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_F32_ACC, EPI_DGELU = 0, 1, 2, 3, 4
M = 256 * 24 + 128
NMAX = 8200
KS = [128, 192, 320]
NS = [8192, 8200, 8196]
RPB = 1152           # 9 x 128 rows per batch of C: tiles cross batch boundaries, a wave's 128 rows do not (the 16-byte paths' condition)


@functools.lru_cache(maxsize=4)
def _problem(Mr, Nr, K):
    """helpers.exact_gemm_problem, computed once per shape and never modified."""
    return exact_gemm_problem(Mr, Nr, K)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_plain_epilogue_is_exact_across_tile_handovers(K, N):
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    A, W, bias, acc = _problem(M, NMAX, K)
    Ad, Wd, bd = A.cuda(), W[:N].contiguous().cuda(), bias[:N].contiguous().cuda()
    g = torch.Generator().manual_seed(K + N)
    for rpb in (None, RPB):
        C = _Out(M, N, rpb, torch.bfloat16, g)
        for with_bias in (True, False):
            C.reset()
            ops.gemm(Rows.of(Ad), Wd, bd if with_bias else None, C.rows, N, K, EPI_BIAS)
            torch.cuda.synchronize()
            _same_bits(C.dense(), _y_ref(acc, bias, N, with_bias))
            assert C.guards_untouched()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gate_residual_epilogue_is_exact_across_tile_handovers(K, N):
    """C = bf16(res + bf16(gate * y)) in fp32 with y = bf16(acc + bias), aux = y (the pre-gate value); gate per batch of C."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    A, W, bias, acc = _problem(M, NMAX, K)
    Ad, Wd, bd = A.cuda(), W[:N].contiguous().cuda(), bias[:N].contiguous().cuda()
    g = torch.Generator().manual_seed(2 * K + N)
    for rpb, with_bias, with_aux in ((None, True, True), (RPB, True, True), (RPB, False, False), (None, False, True)):
        C = _Out(M, N, rpb, torch.bfloat16, g)
        aux = _Out(M, N, None, torch.bfloat16, g) if with_aux else None
        nb = C.store.shape[0]
        gate = _ints((nb, N + GCOLS), -12, 12, 8, g)
        ops.gemm(Rows.of(Ad), Wd, bd if with_bias else None, C.rows, N, K, EPI_GATE_RES, gate=gate.cuda(), gate_ld=N + GCOLS,
                 aux=None if aux is None else aux.store, ldaux=N + GCOLS)
        torch.cuda.synchronize()
        y = _y_ref(acc, bias, N, with_bias)
        res = C.dense(C.init).cpu().float()
        gsel = gate[:, :N].float()[C.batch_of_row()]
        want = (res + (gsel * y.float()).bfloat16().float()).bfloat16()
        _same_bits(C.dense(), want)
        assert C.guards_untouched()
        if aux is not None:
            _same_bits(aux.dense(), y)
            assert aux.guards_untouched()


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_f32_accumulate_epilogue_is_exact_across_tile_handovers(K, N, beta):
    """C = beta * old + acc, one rounding (the reference: fp64, rounded once).  beta = 0 must not read C: it starts as NaN.
    Plain C: the batched form of the epilogue on every full 128 x 64 block, the general form on the ragged edges; batches of
    1000 rows: blocks that cross a batch boundary take the general form in the middle of the matrix as well."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    A, W, bias, acc = _problem(M, NMAX, K)
    Ad, Wd = A.cuda(), W[:N].contiguous().cuda()
    g = torch.Generator().manual_seed(3 * K + N)
    for rpb in (None, RPB, 1000):
        C = _Out(M, N, rpb, torch.float32, g)
        old = C.dense(C.init).cpu()
        if beta == 0.0:
            C.store[~C.guard] = float("nan")
        ops.gemm(Rows.of(Ad), Wd, None, C.rows, N, K, EPI_F32_ACC, beta=beta)
        torch.cuda.synchronize()
        want = (beta * old.double() + acc[:, :N].double()).float() if beta else acc[:, :N].contiguous()
        _same_bits(C.dense(), want)
        assert C.guards_untouched()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gelu_epilogue_is_exact_across_tile_handovers(K, N):
    """aux = y exactly, and C bit-equal to what mgx_gelu_bf16 makes of y (the kept pre-activation's contract)."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    A, W, bias, acc = _problem(M, NMAX, K)
    Ad, Wd, bd = A.cuda(), W[:N].contiguous().cuda(), bias[:N].contiguous().cuda()
    g = torch.Generator().manual_seed(5 * K + N)
    y = _y_ref(acc, bias, N, True)
    ypad = torch.zeros(M, NMAX, dtype=torch.bfloat16, device="cuda")
    ypad[:, :N] = y.cuda()
    act = torch.empty_like(ypad)
    ops.gelu_rows(ypad, NMAX, act, NMAX, M, NMAX)
    torch.cuda.synchronize()
    want = act[:, :N].cpu().contiguous()
    for rpb, with_aux in ((None, True), (RPB, False), (RPB, True)):
        C = _Out(M, N, rpb, torch.bfloat16, g)
        aux = _Out(M, N, None, torch.bfloat16, g) if with_aux else None
        ops.gemm(Rows.of(Ad), Wd, bd, C.rows, N, K, EPI_GELU, aux=None if aux is None else aux.store, ldaux=N + GCOLS)
        torch.cuda.synchronize()
        _same_bits(C.dense(), want)
        assert C.guards_untouched()
        if aux is not None:
            _same_bits(aux.dense(), y)
            assert aux.guards_untouched()


def _dgelu(x):
    x = x.double()
    k0, k1 = 0.7978845608028654, 0.044715
    u = k0 * (x + k1 * x ** 3)
    t = torch.tanh(u)
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gelu_backward_epilogue_across_tile_handovers(K, N):
    """C = bf16(y * gelu'(aux)) against fp64, at the tolerance tests/test_hip_gemm.py holds this epilogue to (y is exact here:
    |diff| <= 2^-7 |ref| + 2 * 1.2 * 2^-7 |y| + 2e-3, fewer than 2 % of the elements differing from the rounded reference)."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    A, W, bias, acc = _problem(M, NMAX, K)
    Ad, Wd, bd = A.cuda(), W[:N].contiguous().cuda(), bias[:N].contiguous().cuda()
    g = torch.Generator().manual_seed(7 * K + N)
    y = _y_ref(acc, bias, N, True).float()
    for rpb in (None, RPB):
        C = _Out(M, N, rpb, torch.bfloat16, g)
        aux = _Out(M, N, None, torch.bfloat16, g)
        cg = torch.Generator(device="cuda").manual_seed(K + N + (rpb or 0))
        aux.store.copy_(torch.randn(aux.store.shape, generator=cg, device="cuda").bfloat16())
        aux.init.copy_(aux.store)
        ops.gemm(Rows.of(Ad), Wd, bd, C.rows, N, K, EPI_DGELU, aux=aux.store, ldaux=N + GCOLS)
        torch.cuda.synchronize()
        ref = (y.double() * _dgelu(aux.dense().cpu().float())).float().bfloat16().float()
        out = C.dense().cpu().float()
        assert torch.isfinite(out).all()
        diff = (out - ref).abs()
        tol = ref.abs() * 2.0 ** -7 + 2 * 1.2 * y.abs() * 2.0 ** -7 + 2e-3
        assert (diff <= tol).all(), f"max excess {(diff - tol).max().item()}"
        assert (out != ref).float().mean().item() < 0.02
        assert C.guards_untouched()
        assert torch.equal(aux.store, aux.init)                      # the saved pre-activation is an input here


@pytest.mark.parametrize("tokens,tok_rpb", [(8192, 8192), (8192, 2048), (8200, 8200)])
@pytest.mark.parametrize("K", KS)
def test_transposed_linear_with_row_bias_is_exact_across_tile_handovers(K, tokens, tok_rpb):
    """mgx_linear_bf16_t: rows = features (M = 256 * 24 + 128 of them, bias per ROW), columns = tokens, in one or four column
    batches; Ct[b][f][t] = bf16(acc[f][b * tok_rpb + t] + bias[f]).  Guard: 8 columns left, 56 right, 2 feature rows below."""
    from mixgrpo_amd import ops
    Wf, X, _, acc = _problem(M, NMAX, K)          # the kernel's A operand is the weight (features), its W operand the tokens
    g = torch.Generator().manual_seed(11 * K + tokens)
    bias = _ints((M,), -16, 16, 32, g)
    B, s0 = tokens // tok_rpb, 8
    Sp = tok_rpb + 64
    init = _ints((B, M + 2, Sp), -64, 64, 32, g).cuda()
    Ct = init.clone()
    assert ops.linear_t(X[:tokens].contiguous().cuda(), Wf.cuda(), bias.cuda(), Ct.view(-1)[s0:], tokens, M, K, Sp, tok_rpb,
                        (M + 2) * Sp)
    torch.cuda.synchronize()
    want = (acc[:, :tokens] + bias.float()[:, None]).bfloat16().view(M, B, tok_rpb).transpose(0, 1).contiguous()
    _same_bits(Ct[:, :M, s0:s0 + tok_rpb], want)
    guard = torch.ones(B, M + 2, Sp, dtype=torch.bool, device="cuda")
    guard[:, :M, s0:s0 + tok_rpb] = False
    assert torch.equal(Ct[guard], init[guard])


def _plan(Mr, Nr, K):
    from mixgrpo_amd import _lib
    out = (ctypes.c_int * 6)()
    assert _lib.lib().mgx_gemm_plan(Mr, Nr, K, 1, out, 6) == 6
    return dict(zip(("family", "grid", "band", "minparts", "nfix", "xcds"), out))


def _units(Mr, Nr, K, wg):
    from mixgrpo_amd import _lib
    out = (ctypes.c_int * 320)()
    n = _lib.lib().mgx_gemm_plan_units(Mr, Nr, K, 1, 0, wg, out, 320)
    assert n >= 0
    return [tuple(out[5 * i:5 * i + 5]) for i in range(n)]


SK_M, SK_N, SK_K = 17 * 256, 16 * 256, 2048     # 272 tiles: every XCD one whole round + 2 tiles cut along K


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_F32_ACC])
def test_stream_k_tail_after_a_whole_tile_is_exact(epi):
    """A split launch (asked of mgx_gemm_plan) whose workgroups hand over from a whole tile to their part of a split one: the
    whole tile's epilogue runs between the two K-loops, the part's raw sums go to the workspace and the fix-up kernel runs the
    same epilogue.  Exact operands: the split changes no bit."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    p = _plan(SK_M, SK_N, SK_K)
    assert p["family"] == 1 and p["nfix"] > 0, p
    walks = [_units(SK_M, SK_N, SK_K, wg) for wg in range(p["grid"])]
    tails = [u for u in walks if u and u[-1][4] == 1]
    assert tails and all(len(u) >= 2 and u[-2][4] == 0 for u in tails), "no workgroup runs a whole tile before its tail part"
    assert ops.GEMM_STREAM_K
    A, W, bias, acc = _problem(SK_M, SK_N, SK_K)
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    g = torch.Generator().manual_seed(epi)
    y = _y_ref(acc, bias, SK_N, True)
    if epi == EPI_F32_ACC:
        C = _Out(SK_M, SK_N, None, torch.float32, g)
        ops.gemm(Rows.of(Ad), Wd, None, C.rows, SK_N, SK_K, epi, beta=0.5)
        want = (0.5 * C.dense(C.init).cpu().double() + acc.double()).float()
    else:
        C = _Out(SK_M, SK_N, 1152 if epi == EPI_GATE_RES else None, torch.bfloat16, g)
        aux = _Out(SK_M, SK_N, None, torch.bfloat16, g) if epi != EPI_BIAS else None
        gate = _ints((C.store.shape[0], SK_N), -12, 12, 8, g)
        ops.gemm(Rows.of(Ad), Wd, bd, C.rows, SK_N, SK_K, epi, gate=gate.cuda() if epi == EPI_GATE_RES else None, gate_ld=SK_N,
                 aux=None if aux is None else aux.store, ldaux=SK_N + GCOLS)
        if epi == EPI_BIAS:
            want = y
        elif epi == EPI_GELU:
            act = torch.empty(SK_M, SK_N, dtype=torch.bfloat16, device="cuda")
            ops.gelu_rows(y.cuda(), SK_N, act, SK_N, SK_M, SK_N)
            want = act.cpu()
        else:
            gsel = gate.float()[C.batch_of_row()]
            want = (C.dense(C.init).cpu().float() + (gsel * y.float()).bfloat16().float()).bfloat16()
    torch.cuda.synchronize()
    _same_bits(C.dense(), want)
    assert C.guards_untouched()
    if epi in (EPI_GELU, EPI_GATE_RES):
        _same_bits(aux.dense(), y)
        assert aux.guards_untouched()


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("K", [128, 320])
def test_qk_norm_epilogue_across_tile_handovers(K, paired):
    """mgx_linear_qk_norm_rope against projection + mgx_qk_norm_rope_fwd_qs, bit for bit, where every workgroup walks at least
    3 tiles (5 x 1664 rows = 32.5 tile rows -- M % 256 == 128 -- by 24 tile columns: 792 tiles) at 2 and 5 K-tiles: the
    epilogue's sums of squares reuse the A stage the next tile's DMA is about to fill.  A second launch gives the same bits."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    B, rows, H, s0, S = 5, 1664, 24, 64, 1792
    g = torch.Generator().manual_seed(K + paired)
    d, tokens = H * 128, B * rows
    assert tokens % 256 == 128 and ((tokens + 255) // 256) * (2 * d // 256) >= 3 * 256
    X = (torch.randn(tokens, K, generator=g) * 0.7).bfloat16().cuda()
    W = (torch.randn(3 * d, K, generator=g) * 0.06).bfloat16().cuda()
    bias = (torch.randn(3 * d, generator=g) * 0.3).bfloat16().cuda()
    wq = (1 + 0.2 * torch.randn(128, generator=g)).cuda()
    wk = (1 + 0.2 * torch.randn(128, generator=g)).cuda()
    ang = torch.rand(S, 64, generator=g) * 6.28
    cos = torch.cos(ang).repeat_interleave(2, dim=1).contiguous().cuda()
    sin = torch.sin(ang).repeat_interleave(2, dim=1)
    if not paired:
        sin = sin * (1 + 0.01 * torch.randn(S, 128, generator=g))
    sin = sin.contiguous().cuda()
    pairs = ops.rope_pair_table(cos, sin)
    assert (pairs is not None) == paired
    q_scale = 1.4426950408889634 / 128 ** 0.5
    outs = []
    for _ in range(2):
        Q1 = torch.full((B, H, S, 128), 7.0, dtype=torch.bfloat16, device="cuda")
        K1 = torch.full_like(Q1, 7.0)
        assert ops.linear_qk_norm_rope(X, W[:2 * d], bias[:2 * d], wq, wk, cos, sin, Q1, K1, B, H, S, rows, s0, K, q_scale=q_scale,
                                       pairs=pairs)
        outs.append((Q1, K1))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    qkv = torch.zeros(tokens, 3 * d, dtype=torch.bfloat16, device="cuda")
    sk_default = ops.GEMM_STREAM_K
    ops.GEMM_STREAM_K = False
    try:
        ops.gemm(Rows.of(X), W[:2 * d], bias[:2 * d], Rows(qkv, tokens, 3 * d), 2 * d, K)
    finally:
        ops.GEMM_STREAM_K = sk_default
    Q0 = torch.full_like(outs[0][0], 7.0)
    K0 = torch.full_like(Q0, 7.0)
    ops.qk_norm_rope(qkv, wq, wk, cos, sin, Q0, K0, None, B, H, S, (S + 63) // 64 * 64, rows, s0, q_scale=q_scale)
    torch.cuda.synchronize()
    assert (Q0[:, :, s0:s0 + rows] != 7.0).any()
    assert torch.equal(outs[0][0], Q0) and torch.equal(outs[0][1], K0)
