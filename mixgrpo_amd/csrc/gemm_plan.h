// The tile plan of the bf16 GEMM (gemm.hip): which kernel family takes a problem, in which order its workgroups walk the
// output tiles, and how the persistent kernel's last, partial round is shared out along K (the stream-K tail).  The ONE
// derivation in C++: gemm_kernel, gemm_pp_kernel, gemm_sk_fixup_kernel and launch() call these functions, and the host
// queries mgx_gemm_plan / mgx_gemm_plan_units return what they give, which tests/test_gemm_plan.py holds against an
// independent restatement of the rule and checks for coverage (every output tile and K-tile exactly once).
//
// Workgroups go round-robin over the 8 XCDs, so workgroup b runs on XCD b & 7 as that XCD's workgroup b >> 3.  Every XCD owns a
// contiguous range of the tile order (`xcd_range`): its workgroups share their A / W panels in the XCD's private L2.
// The tile order (`tile_origin`): bands of `band` tile rows, column-major inside a band.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

// (always inlined: a kernel that calls these must come out as if their text stood in it)
#define GEMM_PLAN_FN __host__ __device__ inline

namespace gemm_plan {

constexpr int BK = 64;             // K-tile
constexpr int PP_GRID = 256;       // workgroups of the persistent kernel: one per CU (a multiple of 8)
constexpr int PP_MIN_TILES = 128;  // 256x256 tiles from which the persistent kernel takes a problem (measured: persistent_shape)
constexpr int SK_PMAX = 8;         // most parts a tail tile is cut into
constexpr int SMALL_BAND = 8;      // band of the 128x128 kernel

GEMM_PLAN_FN int imin(int a, int b) { return a < b ? a : b; }
GEMM_PLAN_FN int tiles(int n, int t) { return (n + t - 1) / t; }

// the tiles of XCD `xcd` out of nwg: [beg, beg + cnt).  (One tile per workgroup: workgroup b takes tile beg + (b >> 3).)
struct XcdRange {
  int beg, cnt;
};
GEMM_PLAN_FN XcdRange xcd_range(int nwg, int xcd) {
  const int q = nwg >> 3, r = nwg & 7;
  return {xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, xcd < r ? q + 1 : q};
}

// (M0, N0) = first row and column of tile `tl` of the order, for tiles of TM x TN.  A macro, and `tile_origin` its function form:
// gemm_pp_kernel expands the text in place -- through a function, of whatever signature, its instruction stream comes out
// in another order than the one its measurements were taken on.
#define GEMM_PLAN_TILE_ORIGIN(tl, band, tiles_m, tiles_n, TM, TN, M0, N0)                 \
  do {                                                                                    \
    const int per_band_ = (band) * (tiles_n);                                             \
    const int b0_ = (tl) / per_band_;                                                     \
    const int rows_in_band_ = gemm_plan::imin((band), (tiles_m) - b0_ * (band));          \
    const int in_band_ = (tl) - b0_ * per_band_;                                          \
    M0 = (long)(b0_ * (band) + in_band_ % rows_in_band_) * (TM);                          \
    N0 = (long)(in_band_ / rows_in_band_) * (TN);                                         \
  } while (0)
GEMM_PLAN_FN void tile_origin(int tl, int band, int tiles_m, int tiles_n, int tm, int tn, long& m0, long& n0) {
  GEMM_PLAN_TILE_ORIGIN(tl, band, tiles_m, tiles_n, tm, tn, m0, n0);
}

// Band of the persistent kernel.  The activation operand streams from HBM, the weights sit in the Infinity Cache: narrow
// outputs (<= 16 tile columns) take band 1 -- a round is whole tile rows, every A panel is fetched once -- wider ones band 4;
// few tile ROWS (wgrad shapes with 3072 output rows): one band of all rows, every W panel once.  `hint` > 0: the caller's.
GEMM_PLAN_FN int band_of(int hint, int tiles_m, int tiles_n) {
  if (hint > 0) return imin(hint, tiles_m);
  return tiles_n <= 16 ? 1 : (tiles_m <= 16 ? tiles_m : 4);
}

// what the persistent 256x256 kernel takes (the rest goes to gemm_kernel): enough tiles to fill most of the 256 CUs
// (measured, scratch/bench_gemm_small.py: 168 tiles 843-935 vs 591-691 TFLOP/s, 120 tiles equal, 24-96 tiles slower), and
// two K-tiles for its prologue
GEMM_PLAN_FN bool persistent_shape(int M, int N, int K, long min_tiles) {
  const long tiles_big = (long)tiles(M, 256) * tiles(N, 256);
  return M >= 256 && N >= 256 && tiles_big >= min_tiles && (N % 256 == 0 || N >= 2048) && K >= 2 * BK;
}

// ---- stream-K tail.  With R tiles left for an XCD's nw workgroups after its whole rounds, every tile's K range is cut into
// P = nw / R equal parts (2 <= P <= SK_PMAX) and workgroup w = p R + r runs part p of tile r (gemm.hip, "stream-K tail").
GEMM_PLAN_FN int sk_parts(int R, int nw) { return R > 0 ? (nw / R < SK_PMAX ? nw / R : SK_PMAX) : 0; }
// ... if that is at least `minparts` parts of at least four K-tiles each (the prologue loads two)
GEMM_PLAN_FN bool sk_on(int minparts, int R, int nw, int nkt) {
  const int P = sk_parts(R, nw);
  return P >= 2 && P >= minparts && nkt >= 4 * P;
}
// The fewest parts worth a split.  A tile's K-loop takes T ~ K * 0.0247 us (2 * 256 * 256 * K FLOP at the 5.3 TFLOP/s a CU
// sustains in this kernel).  Unsplit, the last round takes T; split P ways it takes T / P -- times a slowdown for the P-fold
// panel traffic of the tail (P parts x (rows + columns) panels per step against one round's) -- plus cost_us for the workspace
// round trip and the fix-up launch:   split  <=>  T * (1 - slow / P) > cost.
inline int sk_minparts(int K, float cost_us, float slow) {
  const float tile_us = (float)K * 0.0247f;
  const float room = 1.f - cost_us / tile_us;                 // split <=> slow / P < room
  const int m = room <= 0.f ? SK_PMAX + 1 : (int)floorf(slow / room) + 1;
  return m < 2 ? 2 : m;
}

// A launch of the persistent kernel: its grid, and -- when the caller allows a split (`sk`) and some XCD's tail is split --
// sk_rmax = the most tail tiles of a splitting XCD: the SK form of the kernel runs and 64 * sk_rmax fix-up blocks follow it.
struct PpLaunch {
  int grid, sk_minparts, sk_rmax, sk_xcds /* bit x: XCD x splits its tail */;
};
inline PpLaunch pp_launch(int M, int N, int K, bool sk, float cost_us, float slow) {
  const int nwg = tiles(M, 256) * tiles(N, 256);
  PpLaunch p{PP_GRID, 0, 0, 0};
  if (sk) {
    p.sk_minparts = sk_minparts(K, cost_us, slow);
    for (int x = 0; x < 8; ++x) {
      const int R = xcd_range(nwg, x).cnt % (PP_GRID / 8);
      if (!sk_on(p.sk_minparts, R, PP_GRID / 8, K / BK)) continue;
      p.sk_xcds |= 1 << x;
      if (R > p.sk_rmax) p.sk_rmax = R;
    }
  }
  if (p.sk_rmax == 0 && nwg < PP_GRID) p.grid = (nwg + 7) / 8 * 8;
  return p;
}

// The work of workgroup w of an XCD that owns xcnt tiles and runs nw workgroups: `nfull` whole tiles (w, w + nw, ... of the
// XCD's range), then at most one tail unit.  sk = false (a launch that splits nothing): the strided walk alone.
struct Unit {
  int tile;       // inside the XCD's range
  int k0, k1;     // K-tiles [k0, k1)
  int partial;    // the accumulators go to workspace slot = the workgroup's index; gemm_sk_fixup_kernel finishes the tile
};
struct Walk {
  int nfull, ntail;
  Unit tail;
};
GEMM_PLAN_FN Walk walk(bool sk, int minparts, int xcnt, int nw, int w, int nkt) {
  Walk k{0, 0, {0, 0, nkt, 0}};
  if (!sk) {
    k.nfull = w < xcnt ? (xcnt - w + nw - 1) / nw : 0;
    return k;
  }
  k.nfull = xcnt / nw;
  const int R = xcnt - k.nfull * nw, base = k.nfull * nw;
  if (!sk_on(minparts, R, nw, nkt)) {
    if (w < R) { k.ntail = 1; k.tail.tile = base + w; }
    return k;
  }
  const int P = sk_parts(R, nw);
  if (w >= P * R) return k;
  const int p = w / R, r = w - p * R;
  k.ntail = 1;
  k.tail = {base + r, p * nkt / P, (p + 1) * nkt / P, 1};
  return k;
}
GEMM_PLAN_FN Unit unit(bool sk, const Walk& k, int i, int w, int nw, int nkt) {
  if (!sk || i < k.nfull) return {w + i * nw, 0, nkt, 0};
  return k.tail;
}

// Fix-up block b = (r * 8 + xcd) * 8 + wave finishes tail tile r of XCD xcd for one wave slot of the main kernel: it adds the
// tile's `parts` workspace slots slot0, slot0 + stride, ... -- ascending K -- and runs the epilogue.  parts = 0: nothing to do.
struct Fixup {
  int parts, tile /* of the whole order */, slot0, stride;
};
GEMM_PLAN_FN Fixup fixup(int nwg, int b, int nw, int minparts, int nkt) {
  const int xcd = (b >> 3) & 7, r = b >> 6;
  const XcdRange x = xcd_range(nwg, xcd);
  const int nfull = x.cnt / nw, R = x.cnt - nfull * nw;
  if (r >= R || !sk_on(minparts, R, nw, nkt)) return {0, 0, 0, 0};
  return {sk_parts(R, nw), x.beg + nfull * nw + r, r * 8 + xcd, R * 8};
}

#undef GEMM_PLAN_FN

}  // namespace gemm_plan
