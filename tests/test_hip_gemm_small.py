"""The 128x128 GEMM kernel (csrc/gemm.hip gemm_kernel: what every problem outside gemm_plan::persistent_shape runs, i.e. most
Linears of the inference encoders and the VAE's attention) held BIT FOR BIT against CPU references, and the promise that a row's
result depends neither on M nor on which of the two kernels takes the problem.

Section 1 uses the construction of test_hip_gemm_handover.py: operands on a grid (A multiples of 1/8, W of 1/4, bias of 1/32),
so every product and partial sum is a multiple of 1/32 and, at the largest K here (10240: |sum| <= 2560), far below 2^24 / 32:
the fp32 sum is exact in any order and every later step is one correctly rounded IEEE operation that torch restates on the CPU.
C and aux carry guard rows and columns that have to come back bit for bit.  Three shapes also take A and W as column slices of
wider buffers (lda > K, ldw > K) whose surplus columns hold NaN: a K-loop that runs one chunk too far shows up as a NaN.
Each case first asserts through mgx_gemm_plan that its shape IS family 0 (tests/test_gemm_plan.py repeats that without a GPU).

Section 2 uses random operands, so that the summation order matters: the rows of prefixes of one problem (family 0) against the
same rows of the full problem (family 1), `stream_k=False` throughout."""
import ctypes
import functools

import pytest
import torch

from helpers import GCOLS, GROWS, GuardedOut, exact_gemm_problem, grid_ints, linear_ref, same_bits

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_F32_ACC, EPI_DGELU = 0, 1, 2, 3, 4

# (M, N, K) -> the edge it reaches
SHAPES = [
    (1, 4, 64),            # one tile, one K-tile, one row, one 4-wide column group: every loader row clamps to row 0 / W row 3
    (5, 132, 64),          # N % 8 == 4, a second tile column of 4 features
    (127, 128, 128),       # one under the tile edge
    (128, 128, 128),       # on it
    (129, 136, 10240),     # one over; 160 K-tiles (T5's d_ff)
    (35, 768, 768),        # one prompt through BERT: 6 tiles, fewer than XCDs
    (77, 768, 3072),       # CLIP-L fc2
    (257, 3840, 1280),     # ViT-H q | k | v at one image: 90 tiles
    (1000, 520, 192),      # 8 x 5 tiles: one full band of 8 tile rows, ragged last tile column
    (1100, 264, 128),      # 9 x 3 = 27 tiles: a last band with a single tile row; 27 = 3 * 8 + 3 (uneven xcd_range)
]
WIDE = [(5, 132, 64), (129, 136, 10240), (1100, 264, 128)]          # also run with lda > K and ldw > K
FORMS = WIDE + [(257, 3840, 1280)]                                   # the shapes of the GELU, fp32 and GELU' forms
RPB = 50                                                             # rows per batch: boundaries inside 16-row MFMA tiles
PADC = 8                                                             # NaN columns left and right of a wide operand (16 bytes)

# section 2: the full problem (family 1: 8 x 16 = 128 tiles of 256 x 256) and its row ranges (first row, rows), all family 0
ROWS_FULL = (2048, 4096, 256)
ROWS_RANGES = [(0, 1), (0, 77), (0, 255), (0, 257), (300, 257)]


def _plan(M, N, K, sk=False):
    from mixgrpo_amd import _lib
    out = (ctypes.c_int * 6)()
    assert _lib.lib().mgx_gemm_plan(M, N, K, int(sk), out, 6) == 6
    return dict(zip(("family", "grid", "band", "minparts", "nfix", "xcds"), out))


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """helpers.exact_gemm_problem, computed once per shape and never modified."""
    return exact_gemm_problem(M, N, K)


class _Operands:
    """The device operands of a shape: A plain and in batches of RPB rows (GROWS NaN rows between batches), W and bias; `wide`:
    A and W are column slices [PADC, PADC + K) of buffers K + 2 PADC wide whose other columns hold NaN."""

    def __init__(self, M, N, K, wide):
        from mixgrpo_amd.ops import Rows
        A, W, bias, _ = _problem(M, N, K)
        pad = PADC if wide else 0
        ld = K + 2 * pad
        nb = (M + RPB - 1) // RPB
        plain = torch.full((M, ld), float("nan"), dtype=torch.bfloat16)
        plain[:, pad:pad + K] = A
        batched = torch.full((nb * (RPB + GROWS), ld), float("nan"), dtype=torch.bfloat16)
        rows = torch.arange(M)
        batched[rows // RPB * (RPB + GROWS) + rows % RPB, pad:pad + K] = A
        w = torch.full((N, ld), float("nan"), dtype=torch.bfloat16)
        w[:, pad:pad + K] = W
        self.keep = [t.cuda() for t in (plain, batched, w)]                    # a Rows / W below points into these
        first = lambda t: t.view(-1)[pad:]                                      # contiguous, data_ptr() = the first element
        self.a = {None: Rows(first(self.keep[0]), M, ld), RPB: Rows(first(self.keep[1]), M, ld, RPB, (RPB + GROWS) * ld)}
        self.w, self.ldw = first(self.keep[2]), ld
        self.bias = bias.cuda()


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, wide):
    return _Operands(M, N, K, wide)


def _cases(M, N, K):
    """Asserts family 0 and yields the operand forms of the shape: dense, and for the WIDE shapes the column slices."""
    assert _plan(M, N, K)["family"] == 0 and _plan(M, N, K, True)["family"] == 0, (M, N, K)
    for wide in ((False, True) if (M, N, K) in WIDE else (False,)):
        yield _operands(M, N, K, wide)


def _gemm(op, rpb, C, N, K, epi, with_bias=True, **kw):
    from mixgrpo_amd import ops
    ops.gemm(op.a[rpb], op.w, op.bias if with_bias else None, C.rows, N, K, epi, ldw=op.ldw, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_plain_epilogue_is_exact(M, N, K):
    """C = bf16(acc + bias), with and without bias; plain C and A, and both in batches of 50 rows with a gap of guard rows."""
    _, _, bias, acc = _problem(M, N, K)
    g = torch.Generator().manual_seed(K + N)
    for op in _cases(M, N, K):
        for rpb in (None, RPB):
            C = GuardedOut(M, N, rpb, torch.bfloat16, g)
            for with_bias in (True, False):
                C.reset()
                _gemm(op, rpb, C, N, K, EPI_BIAS, with_bias)
                same_bits(C.dense(), linear_ref(acc, bias, N, with_bias))
                assert C.guards_untouched()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gate_residual_epilogue_is_exact(M, N, K):
    """C = bf16(res + bf16(gate * y)) with y = bf16(acc + bias), aux = y (the pre-gate value); gate per batch of C, gate_ld =
    N + 8; with and without bias, with and without aux."""
    _, _, bias, acc = _problem(M, N, K)
    g = torch.Generator().manual_seed(2 * K + N)
    for op in _cases(M, N, K):
        for rpb, with_bias, with_aux in ((None, True, True), (RPB, True, True), (RPB, False, False), (None, False, True),
                                         (RPB, False, True), (None, True, False)):
            C = GuardedOut(M, N, rpb, torch.bfloat16, g)
            aux = GuardedOut(M, N, None, torch.bfloat16, g) if with_aux else None
            gate = grid_ints((C.store.shape[0], N + GCOLS), -12, 12, 8, g)
            _gemm(op, rpb, C, N, K, EPI_GATE_RES, with_bias, gate=gate.cuda(), gate_ld=N + GCOLS,
                  aux=None if aux is None else aux.store, ldaux=N + GCOLS)
            y = linear_ref(acc, bias, N, with_bias)
            res = C.dense(C.init).cpu().float()
            gsel = gate[:, :N].float()[C.batch_of_row()]
            same_bits(C.dense(), (res + (gsel * y.float()).bfloat16().float()).bfloat16())
            assert C.guards_untouched()
            if aux is not None:
                same_bits(aux.dense(), y)
                assert aux.guards_untouched()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_residual_epilogue_with_a_ones_gate_is_exact(M, N, K):
    """The encoders' residual Linear (EncoderHost._linear): one vector of bf16 ones as the gate, gate_ld = 0, no aux, C holding
    the residual in place: C = bf16(res + bf16(1 * y)); with and without bias."""
    _, _, bias, acc = _problem(M, N, K)
    g = torch.Generator().manual_seed(4 * K + N)
    ones = torch.ones(N, dtype=torch.bfloat16, device="cuda")
    for op in _cases(M, N, K):
        for rpb in (None, RPB):
            C = GuardedOut(M, N, rpb, torch.bfloat16, g)
            for with_bias in (True, False):
                C.reset()
                _gemm(op, rpb, C, N, K, EPI_GATE_RES, with_bias, gate=ones, gate_ld=0)
                y = linear_ref(acc, bias, N, with_bias)
                same_bits(C.dense(), (C.dense(C.init).cpu().float() + y.float()).bfloat16())
                assert C.guards_untouched()


@functools.lru_cache(maxsize=None)
def _gelu_of(M, N, K, with_bias):
    """(y, what mgx_gelu_bf16 makes of y) on the CPU: the kept pre-activation's contract"""
    from mixgrpo_amd import ops
    _, _, bias, acc = _problem(M, N, K)
    y = linear_ref(acc, bias, N, with_bias)
    Np = (N + 7) // 8 * 8
    ypad = torch.zeros(M, Np, dtype=torch.bfloat16, device="cuda")
    ypad[:, :N] = y.cuda()
    act = torch.empty_like(ypad)
    ops.gelu_rows(ypad, Np, act, Np, M, Np)
    torch.cuda.synchronize()
    return y, act[:, :N].cpu().contiguous()


@pytest.mark.parametrize("M,N,K", FORMS)
def test_gelu_epilogue_is_exact(M, N, K):
    """aux = y exactly, and C bit-equal to what mgx_gelu_bf16 makes of y; with and without aux, with and without bias."""
    g = torch.Generator().manual_seed(5 * K + N)
    for op in _cases(M, N, K):
        for rpb, with_aux, with_bias in ((None, True, True), (RPB, False, True), (RPB, True, True), (None, True, False),
                                         (None, False, False)):
            y, want = _gelu_of(M, N, K, with_bias)
            C = GuardedOut(M, N, rpb, torch.bfloat16, g)
            aux = GuardedOut(M, N, None, torch.bfloat16, g) if with_aux else None
            _gemm(op, rpb, C, N, K, EPI_GELU, with_bias, aux=None if aux is None else aux.store, ldaux=N + GCOLS)
            same_bits(C.dense(), want)
            assert C.guards_untouched()
            if aux is not None:
                same_bits(aux.dense(), y)
                assert aux.guards_untouched()


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("M,N,K", FORMS)
def test_f32_accumulate_epilogue_is_exact(M, N, K, beta):
    """C = beta * old + acc: exact on the grid values of old (multiples of 1/32; beta = 0.5: of 1/64).  beta = 0 must not
    read C: it starts as NaN."""
    _, _, _, acc = _problem(M, N, K)
    g = torch.Generator().manual_seed(3 * K + N)
    for op in _cases(M, N, K):
        for rpb in (None, RPB):
            C = GuardedOut(M, N, rpb, torch.float32, g)
            old = C.dense(C.init).cpu()
            if beta == 0.0:
                C.store[~C.guard] = float("nan")
            _gemm(op, rpb, C, N, K, EPI_F32_ACC, False, beta=beta)
            want = (beta * old.double() + acc[:, :N].double()).float() if beta else acc[:, :N].contiguous()
            same_bits(C.dense(), want)
            assert C.guards_untouched()


def _dgelu(x):
    x = x.double()
    k0, k1 = 0.7978845608028654, 0.044715
    u = k0 * (x + k1 * x ** 3)
    t = torch.tanh(u)
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)


@pytest.mark.parametrize("M,N,K", FORMS)
def test_gelu_backward_epilogue(M, N, K):
    """C = bf16(y * gelu'(aux)) against fp64 at the tolerance of test_gelu_backward_epilogue_across_tile_handovers (y is exact
    here: |diff| <= 2^-7 |ref| + 2 * 1.2 * 2^-7 |y| + 2e-3, fewer than 2 % of the elements differing from the rounded
    reference); the guards stay untouched and aux unchanged.  Its bit-level check is test_rows_do_not_depend_on_m_or_kernel."""
    _, _, bias, acc = _problem(M, N, K)
    g = torch.Generator().manual_seed(7 * K + N)
    y = linear_ref(acc, bias, N, True).float()
    for op in _cases(M, N, K):
        for rpb in (None, RPB):
            C = GuardedOut(M, N, rpb, torch.bfloat16, g)
            aux = GuardedOut(M, N, None, torch.bfloat16, g)
            cg = torch.Generator(device="cuda").manual_seed(K + N + (rpb or 0))
            aux.store.copy_(torch.randn(aux.store.shape, generator=cg, device="cuda").bfloat16())
            aux.init.copy_(aux.store)
            _gemm(op, rpb, C, N, K, EPI_DGELU, True, aux=aux.store, ldaux=N + GCOLS)
            ref = (y.double() * _dgelu(aux.dense().cpu().float())).float().bfloat16().float()
            out = C.dense().cpu().float()
            assert torch.isfinite(out).all()
            diff = (out - ref).abs()
            tol = ref.abs() * 2.0 ** -7 + 2 * 1.2 * y.abs() * 2.0 ** -7 + 2e-3
            assert (diff <= tol).all(), f"max excess {(diff - tol).max().item()}"
            assert (out != ref).float().mean().item() < 0.02
            assert C.guards_untouched()
            assert torch.equal(aux.store, aux.init)                      # the saved pre-activation is an input here


# ----------------------------------------------------------------------------------------- section 2: same rows, any M, either kernel
@functools.lru_cache(maxsize=1)
def _rows_problem():
    """Random bf16 operands of ROWS_FULL on the device: (A, W, bias, residual, saved pre-activation); only read."""
    M, N, K = ROWS_FULL
    g = torch.Generator(device="cuda").manual_seed(20)
    A = torch.randn(M, K, generator=g, device="cuda").bfloat16()
    W = (torch.randn(N, K, generator=g, device="cuda") / 16).bfloat16()       # y ~ N(0, 1): where GELU and GELU' bend
    bias = torch.randn(N, generator=g, device="cuda").bfloat16()
    res = torch.randn(M, N, generator=g, device="cuda").bfloat16()
    pre = torch.randn(M, N, generator=g, device="cuda").bfloat16()
    return A, W, bias, res, pre


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_DGELU], ids=["bias", "gelu", "residual", "dgelu"])
def test_rows_do_not_depend_on_m_or_kernel(epi):
    """`ops.gemm(..., stream_k=False)`: "a row's result does not depend on how many rows the call has" -- also where growing
    M moves the problem from the 128x128 kernel to the persistent one (ViT-H q | k | v between batch 1 and batch 8).  The full
    problem runs on the persistent kernel, the row ranges (0, 1), (0, 77), (0, 255), (0, 257) and (300, 257) of the same A,
    residual and saved pre-activation on the 128x128 kernel; every row -- C, and the aux the GELU form writes -- must equal
    the full run's bit for bit.  The residual form is the encoders': a gate of ones, gate_ld = 0, C in place."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    M, N, K = ROWS_FULL
    assert _plan(M, N, K)["family"] == 1
    A, W, bias, res, pre = _rows_problem()
    ones = torch.ones(N, dtype=torch.bfloat16, device="cuda")

    def run(r0, rows):
        C = res[r0:r0 + rows].clone() if epi == EPI_GATE_RES else torch.full((rows, N), float("nan"), dtype=torch.bfloat16, device="cuda")
        aux = {EPI_GELU: torch.full((rows, N), float("nan"), dtype=torch.bfloat16, device="cuda"), EPI_DGELU: pre[r0:r0 + rows]}.get(epi)
        ops.gemm(Rows(A[r0:r0 + rows], rows, K), W, bias, Rows(C, rows, N), N, K, epi, gate=ones if epi == EPI_GATE_RES else None,
                 gate_ld=0, aux=aux, stream_k=False)
        torch.cuda.synchronize()
        return C, aux

    full_c, full_aux = run(0, M)
    assert torch.isfinite(full_c.float()).all()
    for r0, rows in ROWS_RANGES:
        assert _plan(rows, N, K)["family"] == 0, rows
        c, aux = run(r0, rows)
        same_bits(c, full_c[r0:r0 + rows])
        if epi == EPI_GELU:
            same_bits(aux, full_aux[r0:r0 + rows])
