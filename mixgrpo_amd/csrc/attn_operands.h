// Launch operands of the generated 64-wide attention streams (csrc/gen/attn_fwd64.py, attn_bwd_dq64.py, attn_bwd_dkv64.py):
// what a workgroup's asm statement is given besides pointers and strides.  The ONE derivation in C++: the kernels of
// attention.hip / attention_bwd.hip call these functions, and the host query mgx_attn_kv_operands returns their masked form,
// which tests/test_attn_*64kv_emulated.py hold equal to the generators' `kv_operands` (what the CPU interpreter is fed).
//
// A stream walks tiles (64 keys) or blocks (32 queries) in pairs, the first and the last outside its loop.  Unmasked, all of
// S are walked.  Masked (rows >= kv_len are padding), those with a valid row are, rounded up to a pair and never below four:
// the loop's last pair is peeled too, and the first and the last three carry their count of valid rows, one byte each,
// lowest first, as 8 + count (gen/attn_fwd64.py, mask_key).
#pragma once
#include <hip/hip_runtime.h>

namespace attn_ops {

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }

// units of 2^shift rows walked, and the loop's trips
__host__ __device__ inline int walked(bool masked, int S, int kv_len, int shift) {
  return masked ? imax(4, (((kv_len + (1 << shift) - 1) >> shift) + 1) & ~1) : S >> shift;
}
__host__ __device__ inline int trips(bool masked, int n) { return (n - (masked ? 4 : 2)) >> 1; }
// 8 + the valid rows of the `width`-row unit j
__host__ __device__ inline int count(int kv_len, int width, int j) { return 8 + imin(width, imax(0, kv_len - width * j)); }
__host__ __device__ inline int pack4(int kv_len, int width, int j0, int j1, int j2, int j3) {
  return count(kv_len, width, j0) | count(kv_len, width, j1) << 8 | count(kv_len, width, j2) << 16 |
         count(kv_len, width, j3) << 24;
}
// the last valid row of the 256-row block `block` (>= 0 for every block that holds a valid row)
__host__ __device__ inline int last_row(int kv_len, int block) { return imin(255, kv_len - 1 - 256 * block); }

// forward: trips, the clamps of the K and V^T tile fetches, the counts of the first tile and of the last three, the last valid row
struct Fwd64 {
  int nloop, kmax, vmax, kt, kvm1;
};
__host__ __device__ inline Fwd64 fwd64(bool masked, int S, int kv_len) {
  const int nt = walked(masked, S, kv_len, 6);
  return {trips(masked, nt), (nt - 1) * 16384, (nt - 1) * 128, pack4(kv_len, 64, 0, nt - 3, nt - 2, nt - 1), kv_len - 1};
}

// dQ: trips, the length the key window is clamped at, the counts of the 32-key halves of the first tile and of the last three,
// the block's last valid query row
struct Dq64 {
  int nloop, seq, kt0, kt1, qlast;
};
__host__ __device__ inline Dq64 dq64(bool masked, int S, int kv_len, int qt) {
  const int nt = walked(masked, S, kv_len, 6);
  return {trips(masked, nt), masked ? 64 * nt : S, pack4(kv_len, 32, 0, 1, 2 * nt - 6, 2 * nt - 5),
          pack4(kv_len, 32, 2 * nt - 4, 2 * nt - 3, 2 * nt - 2, 2 * nt - 1), last_row(kv_len, qt)};
}

// dK / dV: trips, the clamps of the Q | dO and lse | delta fetches, the counts of the first 32-query block and of the last
// three, the block's last valid key row
struct Dkv64 {
  int nloop, qmax, cmax, qk, klast;
};
__host__ __device__ inline Dkv64 dkv64(bool masked, int S, int kv_len, int kt) {
  const int nq = walked(masked, S, kv_len, 5);
  return {trips(masked, nq), (nq - 1) * 8192, (nq - 1) * 128, pack4(kv_len, 32, 0, nq - 3, nq - 2, nq - 1),
          last_row(kv_len, kt)};
}

}  // namespace attn_ops
