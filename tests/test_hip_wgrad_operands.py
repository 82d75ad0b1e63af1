"""The kernels that build the operands of every weight / bias gradient (`flux_backward._wgrad`, `_dgrad`): `mgx_transpose_bf16`
on both of its kernels (the 8x8 register kernel `transpose8_kernel` and the generic 64x64 LDS kernel `transpose_kernel`), its
column sums (the kernels' partial row blocks + `colsum_finish_kernel`) and the composition transpose -> transpose -> EPI_F32_ACC
GEMM on stale scratch, against plain references.

The transpose is a copy, so it is held bit for bit on random bf16 BIT PATTERNS (NaN payloads, +-0, denormals).  Sums are held
exactly on operands of a grid whose every partial sum is exact in fp32 (randint(-4, 5) / 8: |sum| <= 1100 / 2 in steps of 1/8,
4400 < 2^24), so any summation order gives the fp64 result bit for bit; random data is held to the chain-length bound of the
summation order read off the kernels.

Output buffers are over-allocated by 3 rows and pre-filled with the bit patterns 1 .. 251 (bf16 denormals: never zero, and no
grid value): rows >= N must keep them, columns M .. ld_out - 1 of rows < N must be exactly zero -- the wgrad GEMM contracts over
those columns, and the model's dCt / At scratch is `torch.empty` memory reused across shapes."""
import pytest
import torch

from helpers import grid as _grid, sentinel as _sentinel

pytestmark = pytest.mark.gpu
BF16, F32, I16 = torch.bfloat16, torch.float32, torch.int16
RPB, PAD = 200, 5          # row-batched layouts: 200 rows per batch (a 128-row tile straddles a batch boundary), 5 rows of padding


def _pad64(n):
    return (n + 63) // 64 * 64


def _bits(shape, gen, device="cuda"):
    """Uniformly random 16-bit patterns as bf16."""
    return (torch.randint(0, 1 << 16, shape, generator=gen, device=device) - (1 << 15)).to(I16).view(BF16)


def _operand(M, N, layout, make):
    """An [M, N] matrix as `ops.Rows` in one layout, and the same values as a (possibly strided) [M, N] tensor.
    "plain"; "cols": the column slice at offset N of an [M, 3N] matrix; "batched": M / 200 batches of 200 rows inside a buffer
    with 5 rows of padding per batch; "batched_cols": both; "ld_in": rows N + 4 elements apart (off 8 elements for N % 8 == 0);
    "shifted": the plain matrix one element into its buffer (a pointer off 16 bytes)."""
    from mixgrpo_amd.ops import Rows
    if layout == "plain":
        t = make((M, N))
        return Rows.of(t), t
    if layout == "cols":
        big = make((M, 3 * N))
        return Rows(big.view(-1)[N:], M, 3 * N), big[:, N:2 * N]
    if layout == "ld_in":
        big = make((M, N + 4))
        return Rows(big.view(-1), M, N + 4), big[:, :N]
    if layout == "shifted":
        flat = make((M * N + 1,))
        return Rows(flat[1:], M, N), flat[1:].view(M, N)
    assert M % RPB == 0
    nb = M // RPB
    if layout == "batched":
        big = make((nb, RPB + PAD, N))
        return Rows(big[0, PAD:], M, N, RPB, (RPB + PAD) * N), big[:, PAD:].reshape(M, N)
    assert layout == "batched_cols"
    big = make((nb, RPB + PAD, 3 * N))
    return Rows(big[0, PAD:].reshape(-1)[N:], M, 3 * N, RPB, (RPB + PAD) * 3 * N), big[:, PAD:, N:2 * N].reshape(M, N)


def _transposed(rows, X, N, ld_out, colsum_out=None, beta=1.0):
    """`ops.transpose` of `rows` into a sentinel-filled [N + 3, ld_out] buffer, checked against the logical matrix X: the
    transpose bit for bit, zero pad columns, rows >= N untouched.  Returns the buffer."""
    from mixgrpo_amd import ops
    M = X.shape[0]
    sent = _sentinel((N + 3, ld_out))
    out = sent.clone()
    ops.transpose(rows, N, out, ld_out, colsum_out=colsum_out, colsum_beta=beta)
    o = out.view(I16)
    where = f"M {M} N {N} ld_out {ld_out}"
    assert torch.equal(o[:N, :M], X.contiguous().view(I16).t()), where
    assert not o[:N, M:].any(), where + ": pad columns not zero"
    assert torch.equal(o[N:], sent.view(I16)[N:]), where + ": rows past N written"
    return out


# ------------------------------------------------------------------------------------------------ a. transpose, bit for bit
M_ALL = (1, 7, 200, 257, 1100)
FAST_N, GENERIC_N = (8, 136, 264), (1, 66, 130)
# every way into the generic kernel at N = 136 besides N % 8 != 0
GENERIC_ROUTES = ("odd_ld_out", "ld_in", "shifted")


@pytest.mark.parametrize("M", M_ALL)
@pytest.mark.parametrize("N", FAST_N)
def test_transpose_fast_kernel_bit_exact(M, N):
    gen = torch.Generator(device="cuda").manual_seed(M * 31 + N)
    rows, X = _operand(M, N, "plain", lambda s: _bits(s, gen))
    for ld_out in ((M + 7) // 8 * 8, _pad64(M), _pad64(M) + 64):
        _transposed(rows, X, N, ld_out)


@pytest.mark.parametrize("M", M_ALL)
@pytest.mark.parametrize("N", GENERIC_N)
def test_transpose_generic_kernel_bit_exact(M, N):
    gen = torch.Generator(device="cuda").manual_seed(M * 31 + N)
    rows, X = _operand(M, N, "plain", lambda s: _bits(s, gen))
    _transposed(rows, X, N, M)


@pytest.mark.parametrize("M", M_ALL)
@pytest.mark.parametrize("route", GENERIC_ROUTES)
def test_transpose_generic_kernel_by_alignment_bit_exact(M, route):
    N = 136
    gen = torch.Generator(device="cuda").manual_seed(M * 31 + len(route))
    rows, X = _operand(M, N, "plain" if route == "odd_ld_out" else route, lambda s: _bits(s, gen))
    ld_out = _pad64(M) + 1 if route == "odd_ld_out" else _pad64(M)
    _transposed(rows, X, N, ld_out)


@pytest.mark.parametrize("layout", ["cols", "batched"])
@pytest.mark.parametrize("N", FAST_N + GENERIC_N)
def test_transpose_strided_and_row_batched_input_bit_exact(N, layout):
    M = 600                                                 # 3 batches of 200 rows: rows 128 .. 255 straddle batches 0 and 1
    gen = torch.Generator(device="cuda").manual_seed(N * 7 + len(layout))
    rows, X = _operand(M, N, layout, lambda s: _bits(s, gen))
    for ld_out in ((_pad64(M), _pad64(M) + 64) if N % 8 == 0 else (M,)):
        _transposed(rows, X, N, ld_out)


# ------------------------------------------------------------------------------------------------ b. column sums, exact
COLSUM_CASES = [("plain", 1), ("plain", 64), ("plain", 200), ("plain", 1100), ("cols", 1), ("cols", 64), ("cols", 200),
                ("cols", 600), ("cols", 1100), ("batched", 600)]


@pytest.mark.parametrize("layout,M", COLSUM_CASES)
@pytest.mark.parametrize("N", [8, 136, 264, 130])          # 130: the generic kernel (64-row partial blocks)
def test_colsum_exact_on_the_grid_and_deterministic(N, layout, M):
    """M = 1100: 9 (fast) and 18 (generic) partial row blocks, so a lane of colsum_finish_kernel's 4-way strided loop takes 3
    and 5 trips."""
    gen = torch.Generator(device="cuda").manual_seed(M * 13 + N)
    rows, X = _operand(M, N, layout, lambda s: _grid(s, -4, 5, 8, gen))
    ld_out = _pad64(M) if N % 8 == 0 else M
    total = X.double().sum(0)
    for beta in (1.0, 0.0, 0.5):
        c0 = _grid((N,), -4, 5, 8, gen, dtype=F32)
        ref = beta * c0.double() + total
        got = []
        for _ in range(2):
            c = c0.clone()
            _transposed(rows, X, N, ld_out, colsum_out=c, beta=beta)
            got.append(c)
        assert torch.equal(got[0].double(), ref), f"beta {beta}"
        assert torch.equal(got[0], got[1]), f"beta {beta}: two calls differ"


# ------------------------------------------------------------------------------------------------ c. column sums, random data
def _chain_fast(M):
    # transpose8_kernel: 8 additions per thread (its 8 rows) + 16 over the row groups of the 128-row block (cs[k][.]);
    # colsum_finish_kernel over nblk = cdiv(M, 128) partials: cdiv(nblk, 4) per lane + 2 levels of (r0 + r1) + (r2 + r3)
    # + 1 for beta * out
    nblk = (M + 127) // 128
    return 8 + 16 + (nblk + 3) // 4 + 2 + 1


def _chain_generic(M):
    # transpose_kernel: 64 additions down the rows of the 64-row tile; finish over nblk = cdiv(M, 64) partials as above
    nblk = (M + 63) // 64
    return 64 + (nblk + 3) // 4 + 2 + 1


@pytest.mark.parametrize("M", [200, 1100])
@pytest.mark.parametrize("N", [136, 130])
def test_colsum_random_vs_fp64(M, N):
    """|got - ref| <= L 2^-24 sum_m |x[m, n]| with L the number of fp32 additions on the longest chain from an element to the
    result, counted from the code (`_chain_fast`, `_chain_generic`): 28 / 30 (M = 200 / 1100) for the fast kernel, 68 / 72 for
    the generic one.  (At least three of those additions start from 0 and are exact, so the first-order bound L u covers
    gamma_{L-3} = (L - 3) u / (1 - (L - 3) u).)"""
    from mixgrpo_amd.ops import Rows
    gen = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn(M, N, device="cuda", generator=gen).to(BF16)
    L = _chain_fast(M) if N % 8 == 0 else _chain_generic(M)
    assert L == {(200, 136): 28, (1100, 136): 30, (200, 130): 68, (1100, 130): 72}[(M, N)]
    c = torch.zeros(N, device="cuda")
    _transposed(Rows.of(x), x, N, _pad64(M) if N % 8 == 0 else M, colsum_out=c, beta=0.0)
    ref = x.double().sum(0)
    bound = L * 2.0 ** -24 * x.double().abs().sum(0)
    err = (c.double() - ref).abs()
    print(f"M {M} N {N} L {L}: max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (err / bound).max().item()


# ------------------------------------------------------------------------------------------------ d. the _wgrad composition
NAN_BITS = 0x7FC1


@pytest.mark.parametrize("M,N,K,layout", [(200, 136, 64, "plain"), (600, 264, 128, "batched_cols"), (1, 8, 64, "plain")])
def test_wgrad_composition_exact_on_stale_scratch(M, N, K, layout):
    """What `flux_backward._wgrad` launches, on scratch full of NaNs: gw += dC^T A and gb += colsum(dC), exactly.  Mp - M is 56,
    40 and 63 columns of padding that the GEMM contracts over: one of them left stale makes the result NaN.  Products are
    multiples of 1/32 with |sum| <= 600 / 4: exact in fp32 in any order (and through the stream-K split)."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import EPI_F32_ACC, Rows
    gen = torch.Generator(device="cuda").manual_seed(M + N + K)
    Mp = _pad64(M)
    assert Mp - M in (56, 40, 63)
    dC_rows, dC = _operand(M, N, layout, lambda s: _grid(s, -4, 5, 8, gen))
    A = _grid((M, K), -2, 3, 4, gen)
    extra = 192                                              # the model's scratch is larger than any one operand
    dCt_buf = torch.full((N * Mp + extra,), NAN_BITS, dtype=I16, device="cuda").view(BF16)
    At_buf = torch.full((K * Mp + extra,), NAN_BITS, dtype=I16, device="cuda").view(BF16)
    assert dCt_buf.isnan().all() and At_buf.isnan().all()
    dCt, At = dCt_buf[:N * Mp].view(N, Mp), At_buf[:K * Mp].view(K, Mp)
    gw0, gb0 = _grid((N, K), -4, 5, 8, gen, dtype=F32), _grid((N,), -4, 5, 8, gen, dtype=F32)
    gw, gb = gw0.clone(), gb0.clone()
    ops.transpose(dC_rows, N, dCt, Mp, colsum_out=gb, colsum_beta=1.0)
    ops.transpose(Rows.of(A), K, At, Mp)
    ops.gemm(Rows.of(dCt), At, None, Rows(gw, N, K), K, Mp, EPI_F32_ACC, beta=1.0, ldw=Mp)
    assert torch.equal(gw.double(), gw0.double() + dC.double().t() @ A.double())
    assert torch.equal(gb.double(), gb0.double() + dC.double().sum(0))
    assert torch.equal(dCt[:, :M], dC.t()) and not dCt[:, M:].view(I16).any()
    assert torch.equal(At[:, :M], A.t()) and not At[:, M:].view(I16).any()
    assert (dCt_buf[N * Mp:].view(I16) == NAN_BITS).all() and (At_buf[K * Mp:].view(I16) == NAN_BITS).all()


def test_dgrad_weight_transpose_bit_exact():
    """`_dgrad` forms W^T [K, N] from the [N, K] weight with `transpose(Rows.of(W), K, Wt, N)`."""
    N, K = 136, 264
    gen = torch.Generator(device="cuda").manual_seed(5)
    W = _bits((N, K), gen)
    from mixgrpo_amd.ops import Rows
    _transposed(Rows.of(W), W, K, N)
