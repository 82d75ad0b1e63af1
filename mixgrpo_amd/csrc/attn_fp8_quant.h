// What the e4m3 attention forward (attention_fp8.hip) and backward (attention_fp8_bwd.hip) share: the LDS images of their
// tiles, the per-(batch, head) quantiser passes, defined once in attention_fp8.hip, and the launcher of the bf16 backward's
// prep kernel (attention_bwd.hip).  Every launcher enqueues on `st` and returns nothing (callers MGX_CHECK_LAUNCH).
#pragma once
#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// LDS images of the 8 KiB e4m3 tiles, forward and backward alike.
// K8 tile image: [64 keys][8 chunks of 16 B], chunk ^= (key >> 1) & 7; V8t tile image: [128 d][4 chunks of 16 B],
// chunk ^= ((d >> 2) ^ (d >> 1)) & 3.  Both checked against the ds_read_b128 lane groups ({0-3,12-15,20-27},
// {4-11,16-19,28-31} per half): the 16 lanes of a group read the same chunk index of 16 different rows and land on 16
// different bank quads.
__device__ __forceinline__ int k8_off(int key, int chunk) { return key * 128 + ((chunk ^ ((key >> 1) & 7)) << 4); }
__device__ __forceinline__ int v8_off(int d, int chunk) { return d * 64 + ((chunk ^ (((d >> 2) ^ (d >> 1)) & 3)) << 4); }

__device__ __forceinline__ i32x8 frag32(const char* p0, const char* p1) {
  const uint4 a = *reinterpret_cast<const uint4*>(p0), b = *reinterpret_cast<const uint4*>(p1);
  i32x8 f;
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  return f;
}

namespace mgx_f8 {

constexpr int MAX_SRCS = 4;

// One bf16 tensor seen per (batch, head): element (b, h, row, col) at p[b * bstride + h * hstride + row * ld + col], the
// region rows x cols valid.  Every offset is a multiple of 8 elements (16-byte loads).  Its index in `Srcs` is its row of the
// amax table.  dst: the e4m3 image [B*H, rows, 128] of a row-major tensor (cols == 128), or null when only the amax is wanted.
struct Src {
  const bf16_raw* p;
  long bstride, hstride, ld;
  int rows, cols;
  uint8_t* dst;
};
struct Srcs {
  Src s[MAX_SRCS];
};
inline Src rows_src(const bf16_raw* p, int H, int S, uint8_t* dst) { return {p, (long)H * S * 128, (long)S * 128, 128, S, 128, dst}; }

// A transposed bf16 tensor [B*H, 128, Sp] and its e4m3 image of the same shape, the columns of every 64-block in the order
// the accumulator of a 64-wide score tile hands them to the MFMA (oracle.attention_fp8.key_order()).
struct TSrc {
  const bf16_raw* p;
  uint8_t* dst;
  int amax_row;
};
struct TSrcs {
  TSrc s[MAX_SRCS];
};

// amax[i][B*H] = max |x| of srcs.s[i], i < n (the table is zeroed first)
void amax_launch(const Srcs& srcs, int n, float* amax, int B, int H, hipStream_t st);
// srcs.s[i].dst = e4m3(x * 448 / amax[i]) for the row-major tensors i in [i0, n)
void quant_rows_launch(const Srcs& srcs, int i0, int n, const float* amax, int B, int H, hipStream_t st);
// the transposed images; columns >= valid are written as zero bytes (valid == Sp: every column is quantised)
void quant_t_launch(const TSrcs& srcs, int n, const float* amax, int BH, int valid, int Sp, hipStream_t st);

}  // namespace mgx_f8

// attention_bwd.hip: delta = rowsum(dO * O) and dOt = dO^T (zero from column S on), exactly as mgx_attn_bwd begins
void mgx_attn_bwd_prep_launch(const uint16_t* O, const uint16_t* dO, long ldo, long o_bstride, float* delta, uint16_t* dOt,
                              int B, int H, int S, int Sp, hipStream_t st);
