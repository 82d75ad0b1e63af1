"""The tile plan of the bf16 GEMM (csrc/gemm_plan.h), checked WITHOUT a GPU through the host queries mgx_gemm_plan /
mgx_gemm_plan_units: they return what the functions give that gemm_kernel, gemm_pp_kernel, gemm_sk_fixup_kernel and launch()
themselves call.  Held here: the stream-K split decision against an independent restatement of the rule, the walk of every
workgroup and fix-up block for coverage (every output tile and K-tile exactly once, every workspace slot added once and in K
order), and the kernel-family and band predicates."""
import ctypes
import functools
import math

import pytest

from test_hip_gemm import BIG, SK_SHAPES, SMALL
from test_hip_gemm_small import ROWS_FULL, ROWS_RANGES, SHAPES as SMALL_EXACT

SK_F32_SHAPES = [(2048, 4096, 8192 + 64), (3072, 12288, 4096 + 64), (6144, 3072, 4096)]       # test_gemm_stream_k_f32_accumulate


@functools.lru_cache(maxsize=None)
def _h():
    from mixgrpo_amd import _lib
    return _lib.lib()


def _plan(M, N, K, sk):
    """dict(family, grid, band, minparts, nfix, xcds) of the plain mgx_gemm_bf16_sk call."""
    out = (ctypes.c_int * 6)()
    assert _h().mgx_gemm_plan(M, N, K, int(sk), out, 6) == 6, (M, N, K)
    return dict(zip(("family", "grid", "band", "minparts", "nfix", "xcds"), out))


def _units(M, N, K, sk, wg):
    """[(m0, n0, k0, k1, partial)] of workgroup `wg`."""
    out = (ctypes.c_int * 320)()
    n = _h().mgx_gemm_plan_units(M, N, K, int(sk), 0, wg, out, 320)
    assert n >= 0, (M, N, K, wg)
    return [tuple(out[5 * i:5 * i + 5]) for i in range(n)]


def _fixup(M, N, K, sk, block):
    """(m0, n0, [slots in the order they are added]) of fix-up block `block`; slots == [] for an idle block."""
    out = (ctypes.c_int * 16)()
    n = _h().mgx_gemm_plan_units(M, N, K, int(sk), 1, block, out, 16)
    assert n >= 0, (M, N, K, block)
    return out[0], out[1], list(out[2:2 + n])


def _lib_splits(M, N, K):
    """Per XCD: does the library split the XCD's last round (a workspace given)?"""
    p = _plan(M, N, K, True)
    return [bool(p["xcds"] >> x & 1) for x in range(8)]


def _sk_splits(M, N, K):
    """The cost rule of csrc/gemm.hip `launch()` restated, per XCD: T = 0.0247 K us; P = min(8, 32 // R);
    split <=> P >= max(2, floor(1.25 / (1 - 40 / T)) + 1) and K / 64 >= 4 P."""
    import math
    tiles = math.ceil(M / 256) * math.ceil(N / 256)
    room = 1 - 40.0 / (K * 0.0247)
    minparts = 9 if room <= 0 else max(2, math.floor(1.25 / room) + 1)
    q, rem = tiles // 8, tiles % 8
    out = []
    for cnt in [q + (x < rem) for x in range(8)]:
        R = cnt % 32
        P = min(8, 32 // R) if R else 0
        out.append(P >= 2 and P >= minparts and K // 64 >= 4 * P)
    return out


def test_library_rule_equals_the_restatement():
    """The library's split decision (float32, gemm_plan::sk_minparts / sk_on) is the restated rule (double) on every XCD of
    every swept shape that the persistent kernel takes; what goes to the 128x128 kernel (fewer than 128 tiles) is never split."""
    persistent = 0
    for tiles_m in range(1, 41):
        for tiles_n in (12, 16, 36, 48, 89):
            for K in (1024, 3072, 4096, 8192, 15360, 28672):
                M, N = 256 * tiles_m, 256 * tiles_n
                p = _plan(M, N, K, True)
                if p["family"] == 0:
                    assert tiles_m * tiles_n < 128 and p["xcds"] == 0 and p["nfix"] == 0, (M, N, K)
                    continue
                persistent += 1
                assert _lib_splits(M, N, K) == _sk_splits(M, N, K), (M, N, K)
                assert (p["nfix"] > 0) == any(_sk_splits(M, N, K)), (M, N, K)
                assert _plan(M, N, K, False)["nfix"] == 0 and _plan(M, N, K, False)["xcds"] == 0
    assert persistent > 1000


def test_stream_k_rule_splits_the_test_shapes():
    """The shapes of test_hip_gemm.py's stream-K tests ARE split -- otherwise they would silently test the unsplit kernel."""
    for shp in SK_SHAPES + [(2048, 4096, 8192 + 64), (3072, 12288, 4096 + 64), (6144, 3072, 4096)]:
        assert all(_lib_splits(*shp)), shp
    assert not any(_lib_splits(4608, 3072, 15360))       # R = 27: cannot be cut in two, left whole
    assert not any(_lib_splits(3072, 3072, 28672))       # R = 18 likewise


WALKED = SK_SHAPES + SK_F32_SHAPES + BIG + [(4608, 3072, 15360), (3072, 3072, 28672), (36864, 3072, 3072)] + SMALL + SMALL_EXACT


@pytest.mark.parametrize("sk", [False, True])
@pytest.mark.parametrize("M,N,K", WALKED)
def test_walk_covers_every_tile_and_k_tile_once(M, N, K, sk):
    p = _plan(M, N, K, sk)
    T = 256 if p["family"] else 128
    nkt = K // 64
    pieces = {}                      # tile origin -> [(k0, k1, partial, workgroup)]
    for wg in range(p["grid"]):
        for m0, n0, k0, k1, partial in _units(M, N, K, sk, wg):
            assert 0 <= k0 < k1 <= nkt
            if partial:
                assert k1 - k0 >= 2, (wg, k0, k1)          # the prologue loads two K-tiles
            else:
                assert (k0, k1) == (0, nkt), (wg, k0, k1)  # whole units span 0 .. K / 64
            pieces.setdefault((m0, n0), []).append((k0, k1, partial, wg))
    assert set(pieces) == {(i * T, j * T) for i in range(math.ceil(M / T)) for j in range(math.ceil(N / T))}
    for origin, ps in pieces.items():
        ps.sort()
        assert ps[0][0] == 0 and ps[-1][1] == nkt, (origin, ps)
        assert all(a[1] == b[0] for a, b in zip(ps, ps[1:])), (origin, ps)     # no K-tile twice, none left out
        assert len({q[2] for q in ps}) == 1, (origin, ps)                       # all whole (then one) or all partial
        assert ps[0][2] or len(ps) == 1, (origin, ps)
    partial = {origin: [q[3] for q in ps] for origin, ps in pieces.items() if ps[0][2]}       # slots in ascending k0
    if not sk or p["family"] == 0:
        assert p["nfix"] == 0 and not partial
    assert (p["nfix"] > 0) == bool(partial)
    added = {}                       # (wave slot, workspace slot) -> fix-up blocks that add it
    for b in range(p["nfix"]):
        m0, n0, slots = _fixup(M, N, K, sk, b)
        if not slots:
            continue
        assert (m0, n0) in partial, (b, m0, n0)             # no fix-up block touches a tile computed whole
        assert slots == partial[(m0, n0)], (b, slots)       # its tile's parts, all of them, in ascending K
        for s in slots:
            added.setdefault((b & 7, s), []).append(b)
    # every partial unit's slot is added exactly once for each of the main kernel's eight wave slots
    assert sorted(added) == sorted((w, s) for w in range(8) for ss in partial.values() for s in ss)
    assert all(len(v) == 1 for v in added.values())
    assert all(0 <= s < 256 for ss in partial.values() for s in ss)            # inside the 256-slot workspace


def test_family_predicate():
    """Persistent 256x256 kernel for the BIG shapes of test_hip_gemm.py, 128x128 kernel for the SMALL ones.  (6144, 2048, 64) of
    BIG has a single K-tile: the persistent kernel's prologue loads two, so it has always gone to the 128x128 kernel.)"""
    for shp in BIG:
        assert _plan(*shp, True)["family"] == (1 if shp[2] >= 128 else 0), shp
        assert _plan(*shp, False)["family"] == (1 if shp[2] >= 128 else 0), shp
    assert [s for s in BIG if s[2] < 128] == [(256 * 24, 2048, 64)]
    for shp in SMALL:
        assert _plan(*shp, True)["family"] == 0, shp
    for shp in SK_SHAPES + SK_F32_SHAPES:
        assert _plan(*shp, True)["family"] == 1, shp


@pytest.mark.parametrize("M,N,K", SMALL_EXACT)
def test_exact_shapes_of_the_128x128_kernel_are_family_0(M, N, K):
    """The shapes of test_hip_gemm_small.py go to the 128x128 kernel, workspace or not, one workgroup per 128x128 tile in bands
    of SMALL_BAND tile rows -- otherwise they would silently test the other kernel."""
    for sk in (False, True):
        p = _plan(M, N, K, sk)
        assert (p["family"], p["grid"], p["band"], p["nfix"]) == (0, math.ceil(M / 128) * math.ceil(N / 128), 8, 0), (M, N, K, p)


def test_row_ranges_change_kernel_family():
    """test_rows_do_not_depend_on_m_or_kernel: the full problem is the persistent kernel's (128 tiles, nothing split without a
    workspace), every row range of it the 128x128 kernel's."""
    M, N, K = ROWS_FULL
    p = _plan(M, N, K, False)
    assert p["family"] == 1 and p["nfix"] == 0 and math.ceil(M / 256) * math.ceil(N / 256) == 128
    for r0, rows in ROWS_RANGES:
        assert r0 + rows <= M and _plan(rows, N, K, False)["family"] == 0, (r0, rows)


def test_band_rule():
    """1 for tiles_n <= 16, else tiles_m for tiles_m <= 16, else 4."""
    seen = set()
    for tiles_m in range(1, 41):
        for tiles_n in (12, 16, 17, 36, 48, 89):
            p = _plan(256 * tiles_m, 256 * tiles_n, 1024, False)
            if p["family"] == 0:
                continue
            want = 1 if tiles_n <= 16 else (tiles_m if tiles_m <= 16 else 4)
            assert p["band"] == want, (tiles_m, tiles_n)
            seen.add(want)
    assert {1, 4, 16} <= seen


def test_queries_refuse_bad_arguments():
    out = (ctypes.c_int * 8)()
    h = _h()
    for bad in ((0, 256, 64, 0, out, 6), (256, 256, 65, 0, out, 6), (256, 6, 64, 0, out, 6), (256, 256, 64, 0, None, 6),
                (256, 256, 64, 0, out, 5)):
        assert h.mgx_gemm_plan(*bad) == -1, bad
    assert h.mgx_gemm_plan_units(2048, 4096, 8192, 1, 0, 256, out, 8) == -1       # 256 workgroups: 0 .. 255
    assert h.mgx_gemm_plan_units(2048, 4096, 8192, 0, 1, 0, out, 8) == -1         # nothing split: no fix-up blocks
    assert h.mgx_gemm_plan_units(2048, 4096, 8192, 1, 0, 0, out, 4) == -1         # too little room for a unit
