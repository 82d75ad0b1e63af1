// Low-rank adapter (LoRA) kernels: the rank-r halves of a target Linear's backward and the merge of the adapters into the bf16
// compute copy of its weight.  For y = x (W0 + s B A)^T + b with A [r, K], B [N, r] (kept transposed: Bt [r, N], so that both
// adapter halves are "r rows x wide"):
//   mgx_lora_proj    Out[M, r]  = bf16(scale * In[M, Kin] P[r, Kin]^T)      T = s X A^T  and  dT = s dC B
//   mgx_lora_wgrad   G[r, Kin]  = beta G + Small[M, r]^T Big[M, Kin]        dBt += T^T dC  and  dA += dT^T X
//   mgx_lora_merge   W16[n, k]  = bf16(W0[n, k] + s sum_j Bt[j, n] A[j, k])       (fp64 sum of the fp32 masters, one rounding)
// The full [N, K] weight gradient is never formed.  No atomics anywhere: every sum has a fixed order, so results are
// bit-reproducible run to run.
#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

// row m of a row-batched activation (ops.Rows): base + (m / rpb) * bstride + (m % rpb) * ld elements
struct LRows {
  long ld, rpb, bstride;
  __device__ __forceinline__ long off(long m) const { return (m / rpb) * bstride + (m % rpb) * ld; }
};

// ------------------------------------------------------------------------------------------------ proj
// Workgroup = 32 rows of In against all R rows of P; its four waves split Kin (each streams its K-range of the 32 rows
// straight from global memory into MFMA fragments, 16-byte loads; P is small and stays in L2) and wave 0 adds the four partial
// tiles in a fixed order.  v_mfma_f32_16x16x32_bf16 with P as the A operand: a lane ends up with 4 consecutive r-columns of
// one row of Out (one 8-byte store).
template <int R>
__global__ void __launch_bounds__(256) lora_proj_kernel(const bf16_raw* __restrict__ in, const bf16_raw* __restrict__ P,
                                                        bf16_raw* __restrict__ out, long M, int Kin, LRows map, float scale) {
  constexpr int NT = R / 16;
  __shared__ f32x4 red[3][2 * NT][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const long m0 = (long)blockIdx.x * 32;
  long r0 = m0 + fr, r1 = m0 + 16 + fr;
  if (r0 >= M) r0 = M - 1;                                  // (clamped rows are computed and not stored)
  if (r1 >= M) r1 = M - 1;
  const bf16_raw* x0 = in + map.off(r0) + fq * 8;
  const bf16_raw* x1 = in + map.off(r1) + fq * 8;
  const bf16_raw* pp = P + (long)fr * Kin + fq * 8;
  const int ksteps = Kin / 32, per = (ksteps + 3) / 4;
  const int kbeg = min(w * per, ksteps) * 32, kend = min((w + 1) * per, ksteps) * 32;
  f32x4 acc[2][NT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[h][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k = kbeg; k < kend; k += 32) {
    const s16x8 b0 = *reinterpret_cast<const s16x8*>(x0 + k);
    const s16x8 b1 = *reinterpret_cast<const s16x8*>(x1 + k);
    s16x8 a[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const s16x8*>(pp + (long)t * 16 * Kin + k);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b0, acc[0][t], 0, 0, 0);
      acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b1, acc[1][t], 0, 0, 0);
    }
  }
  if (w > 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < NT; ++t) red[w - 1][h * NT + t][lane] = acc[h][t];
  }
  __syncthreads();
  if (w > 0) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const long m = m0 + h * 16 + fr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 v = acc[h][t];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const f32x4 o = red[i][h * NT + t][lane];
        v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
      }
      // D[i = r-column][j = row]: the lane holds row fr, r-columns 16 t + 4 fq + 0..3
      if (m < M) {
        uint2 u;
        u.x = pack_bf16(scale * v[0], scale * v[1]);
        u.y = pack_bf16(scale * v[2], scale * v[3]);
        *reinterpret_cast<uint2*>(out + m * R + t * 16 + fq * 4) = u;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ wgrad
// Both operands are row-major and the contraction runs over their ROWS, so both MFMA fragments are columns of a tile: the
// workgroup stages 64 rows of Small (all R columns) and of Big (128 columns) in LDS and every fragment is taken with the
// transposed LDS read (ds_read_b64_tr_b16: a 16-lane group reads 4 rows x 16 columns and each lane receives one column).
// All 64 lanes of every wave issue every such read: rows past the end of the chunk and columns past Kin are zero-filled in the
// tile, never masked.  The k index of the MFMA is a free permutation as long as both fragments use the same one: lane group
// q takes rows 4q .. 4q+3 and 16 + 4q .. 16 + 4q + 3 of a 32-row step, so a 32-lane half reads 8 consecutive rows, which the
// row stride (an odd multiple of 32 bytes) spreads over all 64 banks.
// Grid: x = 128-column block of Big, y = chunk of rows.  A workgroup writes its [R, 128] partial sum to the workspace;
// lora_wgrad_finish_kernel adds the chunks in order.
constexpr int WG_ROWS = 64, WG_COLS = 128;
constexpr int BIG_STRIDE = WG_COLS + 16;                              // elements: 288 bytes = 9 x 32

__host__ __device__ constexpr int small_stride(int R) { return (R / 16) % 2 ? R : R + 16; }   // elements

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ s16x8 tr_frag(const bf16_raw* tile, int stride, int row, int col) {
  // rows row .. row+3 and row+16 .. row+19, 16 columns from `col`; `row` / `col` already carry this lane's share
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + row * stride + col));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + (row + 16) * stride + col));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int R>
__global__ void __launch_bounds__(256) lora_wgrad_kernel(const bf16_raw* __restrict__ small, const bf16_raw* __restrict__ big,
                                                         float* __restrict__ part, long M, int Kin, LRows map, int tiles_per_chunk) {
  constexpr int NT = R / 16, SS = small_stride(R);
  constexpr int SCH = R / 8;                                          // 16-byte chunks per Small row
  __shared__ __attribute__((aligned(16))) bf16_raw sBig[WG_ROWS * BIG_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16_raw sSmall[WG_ROWS * SS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.x * WG_COLS;
  const long mbeg = (long)blockIdx.y * tiles_per_chunk * WG_ROWS;
  const long mend = min(M, mbeg + (long)tiles_per_chunk * WG_ROWS);
  // this lane's share of a transposed read: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int trow = 4 * g + q, tcol = 4 * p;
  f32x4 acc[2][NT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[h][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging: Big tile = 64 rows x 16 chunks of 16 bytes: 4 per thread; Small tile = 64 x SCH chunks
  constexpr int SPT = (WG_ROWS * SCH + 255) / 256;
  uint4 rb[4], rs[SPT];
  auto load = [&](long m0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + i * 256, row = id >> 4, ch = id & 15;
      const long m = m0 + row;
      rb[i] = make_uint4(0, 0, 0, 0);
      if (m < mend && c0 + ch * 8 < Kin) rb[i] = *reinterpret_cast<const uint4*>(big + map.off(m) + c0 + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      const int id = tid + i * 256, row = id / SCH, ch = id % SCH;
      const long m = m0 + row;
      rs[i] = make_uint4(0, 0, 0, 0);
      if (id < WG_ROWS * SCH && m < mend) rs[i] = *reinterpret_cast<const uint4*>(small + m * R + ch * 8);
    }
  };
  if (mbeg < mend) load(mbeg);
  for (long m0 = mbeg; m0 < mend; m0 += WG_ROWS) {
    __syncthreads();                                                  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + i * 256, row = id >> 4, ch = id & 15;
      *reinterpret_cast<uint4*>(sBig + row * BIG_STRIDE + ch * 8) = rb[i];
    }
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      const int id = tid + i * 256, row = id / SCH, ch = id % SCH;
      if (id < WG_ROWS * SCH) *reinterpret_cast<uint4*>(sSmall + row * SS + ch * 8) = rs[i];
    }
    __syncthreads();
    if (m0 + WG_ROWS < mend) load(m0 + WG_ROWS);                      // the next tile's loads fly under this tile's MFMAs
#pragma unroll
    for (int ks = 0; ks < WG_ROWS / 32; ++ks) {
      const int row = ks * 32 + trow;
      // wave w owns the 16-column tiles 2w and 2w+1 of the 128 columns
      const s16x8 b0 = tr_frag(sBig, BIG_STRIDE, row, (2 * w) * 16 + tcol);
      const s16x8 b1 = tr_frag(sBig, BIG_STRIDE, row, (2 * w + 1) * 16 + tcol);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const s16x8 a = tr_frag(sSmall, SS, row, t * 16 + tcol);
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[1][t], 0, 0, 0);
      }
    }
  }
  // D[i = r-row][j = column]: the lane holds column (lane & 15) of its tile, r-rows 16 t + 4 (lane >> 4) + 0..3
  float* dst = part + (long)blockIdx.y * R * Kin;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int col = c0 + (2 * w + h) * 16 + (lane & 15);
    if (col < Kin) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[(long)(t * 16 + 4 * g + i) * Kin + col] = acc[h][t][i];
    }
  }
}

// G = beta G + part[0] + part[1] + ... in that order (beta == 0: G is not read)
__global__ void __launch_bounds__(256) lora_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ G, long n,
                                                                int chunks, float beta) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float4 s = *reinterpret_cast<const float4*>(part + i);
  for (int c = 1; c < chunks; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(part + (long)c * n + i);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (beta != 0.f) {
    const float4 o = *reinterpret_cast<const float4*>(G + i);
    s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w;
  }
  *reinterpret_cast<float4*>(G + i) = s;
}

// rows of Big per workgroup chunk, in 64-row tiles: enough chunks to fill the device (about 1024 workgroups), never more
// chunks than tiles
static inline int wgrad_tiles_per_chunk(long M, int Kin) {
  const long tiles = (M + WG_ROWS - 1) / WG_ROWS;
  const long colblocks = (Kin + WG_COLS - 1) / WG_COLS;
  long want = (1024 + colblocks - 1) / colblocks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  return (int)((tiles + want - 1) / want);
}
static inline int wgrad_chunks(long M, int Kin) {
  const long tiles = (M + WG_ROWS - 1) / WG_ROWS;
  const int tpc = wgrad_tiles_per_chunk(M, Kin);
  return (int)((tiles + tpc - 1) / tpc);
}

// ------------------------------------------------------------------------------------------------ merge
// Thread = one column k of 8 weight rows.  The fp32 masters are multiplied and summed in fp64 (a product of two fp32 values is
// exact there; j ascending), W0 is added in fp64, and the result is rounded ONCE to bf16: how the full fine-tune refreshes its
// compute copy from the fp32 master.  An fp32 sum is not enough for that: where W0 and s B A cancel (|W| ~ 1e-6 for weights of
// 0.05) its absolute error of ~1e-8 is several bf16 ulps of the result.  The kernel runs twice per train step; fp64 FMA is cheap.
__device__ __forceinline__ bf16_raw f64_to_bf16(double x) {
  // fp64 -> fp32 toward zero with the lost bits folded into the last one (round to odd), then fp32 -> bf16 to nearest even:
  // equal to one nearest-even rounding of x, because fp32 keeps 16 bits more than bf16
  float f = __double2float_rz(x);
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((double)f != x && (u & 0x7f800000u) != 0x7f800000u) u |= 1u;
  return f2bf(__builtin_bit_cast(float, u));
}

__global__ void __launch_bounds__(256) lora_merge_kernel(const float* __restrict__ W0, const float* __restrict__ Bt,
                                                         const float* __restrict__ A, bf16_raw* __restrict__ W16, int N, int K,
                                                         int R, float s) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n0 = blockIdx.y * 8;
  if (k >= K) return;
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0;
  for (int j = 0; j < R; ++j) {
    const double a = (double)A[(long)j * K + k];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = fma((double)Bt[(long)j * N + min(n0 + i, N - 1)], a, acc[i]);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = n0 + i;
    if (n < N) W16[(long)n * K + k] = f64_to_bf16(fma((double)s, acc[i], (double)W0[(long)n * K + k]));
  }
}

bool rank_ok(int r) { return r == 16 || r == 32 || r == 64 || r == 128; }

}  // namespace

extern "C" int mgx_lora_proj(const uint16_t* in, const uint16_t* P, uint16_t* out, long M, int Kin, int r, long ld_in,
                             long in_rpb, long in_bstride, float scale, void* stream) {
  MGX_REQUIRE(in && P && out, "null pointer");
  MGX_REQUIRE(rank_ok(r), "rank must be 16, 32, 64 or 128");
  MGX_REQUIRE(M >= 1 && M < (1L << 31), "M out of range");
  MGX_REQUIRE(Kin >= 64 && Kin % 64 == 0, "Kin must be a positive multiple of 64");
  MGX_REQUIRE(ld_in >= Kin && ld_in % 8 == 0 && in_rpb >= 1 && in_bstride % 8 == 0, "input rows must be 16-byte aligned");
  MGX_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)P % 16 == 0 && (uintptr_t)out % 8 == 0, "pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const LRows map{ld_in, in_rpb, in_bstride};
  const int grid = cdiv(M, 32);
  switch (r) {
    case 16: lora_proj_kernel<16><<<grid, 256, 0, st>>>(in, P, out, M, Kin, map, scale); break;
    case 32: lora_proj_kernel<32><<<grid, 256, 0, st>>>(in, P, out, M, Kin, map, scale); break;
    case 64: lora_proj_kernel<64><<<grid, 256, 0, st>>>(in, P, out, M, Kin, map, scale); break;
    default: lora_proj_kernel<128><<<grid, 256, 0, st>>>(in, P, out, M, Kin, map, scale); break;
  }
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" long mgx_lora_wgrad_workspace(long M, int Kin, int r) {
  if (M < 1 || M >= (1L << 31) || Kin < 64 || Kin % 64 != 0 || !rank_ok(r)) return -1;
  return (long)wgrad_chunks(M, Kin) * r * Kin;
}

extern "C" int mgx_lora_wgrad(const uint16_t* small, const uint16_t* big, float* G, float* workspace, long workspace_elems,
                              long M, int Kin, int r, long ld_big, long big_rpb, long big_bstride, float beta, void* stream) {
  MGX_REQUIRE(small && big && G && workspace, "null pointer");
  MGX_REQUIRE(rank_ok(r), "rank must be 16, 32, 64 or 128");
  MGX_REQUIRE(M >= 1 && M < (1L << 31), "M out of range");
  MGX_REQUIRE(Kin >= 64 && Kin % 64 == 0, "Kin must be a positive multiple of 64");
  MGX_REQUIRE(ld_big >= Kin && ld_big % 8 == 0 && big_rpb >= 1 && big_bstride % 8 == 0, "operand rows must be 16-byte aligned");
  MGX_REQUIRE((uintptr_t)small % 16 == 0 && (uintptr_t)big % 16 == 0 && (uintptr_t)G % 16 == 0 && (uintptr_t)workspace % 16 == 0,
              "pointers must be 16-byte aligned");
  MGX_REQUIRE(workspace_elems >= mgx_lora_wgrad_workspace(M, Kin, r), "workspace too small (mgx_lora_wgrad_workspace)");
  hipStream_t st = (hipStream_t)stream;
  const LRows map{ld_big, big_rpb, big_bstride};
  const int tpc = wgrad_tiles_per_chunk(M, Kin), chunks = wgrad_chunks(M, Kin);
  const dim3 grid(cdiv(Kin, WG_COLS), chunks);
  switch (r) {
    case 16: lora_wgrad_kernel<16><<<grid, 256, 0, st>>>(small, big, workspace, M, Kin, map, tpc); break;
    case 32: lora_wgrad_kernel<32><<<grid, 256, 0, st>>>(small, big, workspace, M, Kin, map, tpc); break;
    case 64: lora_wgrad_kernel<64><<<grid, 256, 0, st>>>(small, big, workspace, M, Kin, map, tpc); break;
    default: lora_wgrad_kernel<128><<<grid, 256, 0, st>>>(small, big, workspace, M, Kin, map, tpc); break;
  }
  MGX_CHECK_LAUNCH();
  const long n = (long)r * Kin;
  lora_wgrad_finish_kernel<<<cdiv(n, 1024), 256, 0, st>>>(workspace, G, n, chunks, beta);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_lora_merge(const float* W0, const float* Bt, const float* A, uint16_t* W16, int N, int K, int r, float s,
                              void* stream) {
  MGX_REQUIRE(W0 && Bt && A && W16, "null pointer");
  MGX_REQUIRE(rank_ok(r), "rank must be 16, 32, 64 or 128");
  MGX_REQUIRE(N >= 1 && K >= 64 && K % 64 == 0, "K must be a positive multiple of 64");
  lora_merge_kernel<<<dim3(cdiv(K, 256), cdiv(N, 8)), 256, 0, (hipStream_t)stream>>>(W0, Bt, A, W16, N, K, r, s);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
