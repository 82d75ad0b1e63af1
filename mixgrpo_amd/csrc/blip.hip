// ImageReward scorer (fastvideo/models/reward_model/image_reward.py:24-40: `RM.load(...)`, `self.model.inference_rank(text,
// [image])` :38): a BLIP ViT image encoder, a BERT text encoder whose every layer cross-attends to the image tokens, and an MLP
// head.  Its Linears run on the GEMM kernels (gemm.hip), LayerNorm / GELU / embeddings on clip.hip and text.hip; this file
// holds the two things those cannot do.  Inference only.
//   mgx_xattn_fwd         attention with q, k and v in separate buffers (Sq != Skv allowed) and a key length per sample
//   mgx_linear_rows_f32   fp32 Linear of a few rows, for the score head
#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

// vit_attn_kernel's scheme (vit_attn.h: one workgroup per (batch, head, block of 64 queries), four waves of 16 queries, keys and
// values through LDS in blocks of 64 with an online softmax, both products transposed so that a query stays on one lane column)
// and its arithmetic, operation for operation, with two differences:
//   - q, k and v have their own base pointers, row strides and row counts (Sq queries, Skv keys per sample);
//   - only the keys t < kvn count, kvn = clamp(kv_len[b], 1, Skv) (Skv without a kv_len).  The rows at or beyond kvn are not
//     read at all: they are zeros in LDS, like the rows beyond the sequence, so that whatever they hold -- inf and NaN
//     included -- meets neither the scores nor the P V product (0 x NaN is NaN on the matrix pipe), and their scores are
//     -inf before the maximum is taken.  Key blocks that start at or beyond kvn are neither loaded nor multiplied.
// kvn >= 1: key 0 is admitted in the first block and k0 < kvn in every later one, so no row meets a block with nothing admitted.
template <int DP>
__global__ void __launch_bounds__(256) xattn_kernel(const bf16_raw* __restrict__ Q, long ldq, const bf16_raw* __restrict__ K, long ldk,
                                                    const bf16_raw* __restrict__ V, long ldv, bf16_raw* __restrict__ O, long ldo, int H,
                                                    int Sq, int Skv, int d, float scale_log2, const int* __restrict__ kv_len) {
  constexpr int KS = DP + 8;     // elements between key rows of the K image
  constexpr int VS = 64 + 4;     // elements between head-column rows of the V^T image
  constexpr int CH = DP / 8;     // 16-byte chunks per key
  __shared__ __attribute__((aligned(16))) bf16_raw Ks[64 * KS];
  __shared__ __attribute__((aligned(16))) bf16_raw Vt[DP * VS];
  const int nqb = (Sq + 63) / 64;
  const int qb = blockIdx.x % nqb, h = (blockIdx.x / nqb) % H, b = blockIdx.x / (nqb * H);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const bf16_raw* qbase = Q + (long)b * Sq * ldq + (long)h * d;
  const bf16_raw* kbase = K + (long)b * Skv * ldk + (long)h * d;
  const bf16_raw* vbase = V + (long)b * Skv * ldv + (long)h * d;
  const int q = qb * 64 + wave * 16 + c;
  int kvn = Skv;
  if (kv_len) {
    kvn = kv_len[b];
    kvn = kvn < 1 ? 1 : (kvn > Skv ? Skv : kvn);
  }

  s16x8 qf[DP / 32];
#pragma unroll
  for (int ks = 0; ks < DP / 32; ++ks) {
    const int col = 32 * ks + 8 * g;
    uint4 u = {0u, 0u, 0u, 0u};
    if (q < Sq && col < d) u = *reinterpret_cast<const uint4*>(qbase + (long)q * ldq + col);
    qf[ks] = __builtin_bit_cast(s16x8, u);
  }
  f32x4 acc[DP / 16];
#pragma unroll
  for (int i = 0; i < DP / 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  for (int k0 = 0; k0 < kvn; k0 += 64) {
    __syncthreads();                                        // the block before this one has been consumed
    for (int i = tid; i < 64 * CH; i += 256) {
      const int key = i / CH, ch = i % CH;
      uint4 u = {0u, 0u, 0u, 0u};
      if (k0 + key < kvn && ch * 8 < d) u = *reinterpret_cast<const uint4*>(kbase + (long)(k0 + key) * ldk + ch * 8);
      *reinterpret_cast<uint4*>(&Ks[key * KS + ch * 8]) = u;
    }
    for (int i = tid; i < 64 * CH; i += 256) {
      const int key = i & 63, ch = i >> 6;
      uint4 u = {0u, 0u, 0u, 0u};
      if (k0 + key < kvn && ch * 8 < d) u = *reinterpret_cast<const uint4*>(vbase + (long)(k0 + key) * ldv + ch * 8);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Vt[(ch * 8 + 2 * e) * VS + key] = (bf16_raw)(w[e] & 0xffff);
        Vt[(ch * 8 + 2 * e + 1) * VS + key] = (bf16_raw)(w[e] >> 16);
      }
    }
    __syncthreads();

    f32x4 sc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      sc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < DP / 32; ++ks) {
        const s16x8 a = *reinterpret_cast<const s16x8*>(&Ks[(16 * s + c) * KS + 32 * ks + 8 * g]);
        sc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[ks], sc[s], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = k0 + 16 * s + 4 * g + r < kvn ? sc[s][r] * scale_log2 : -INFINITY;
        sc[s][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);                          // finite: key k0 < kvn is admitted
    const float alpha = exp2f(m - mn);
    m = mn;
    float rs = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(sc[s][r] - mn);
        sc[s][r] = p;
        rs += p;
      }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    s16x8 pf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const uint4 u = {pack_bf16(sc[2 * t][0], sc[2 * t][1]), pack_bf16(sc[2 * t][2], sc[2 * t][3]),
                       pack_bf16(sc[2 * t + 1][0], sc[2 * t + 1][1]), pack_bf16(sc[2 * t + 1][2], sc[2 * t + 1][3])};
      pf[t] = __builtin_bit_cast(s16x8, u);
    }
#pragma unroll
    for (int dt = 0; dt < DP / 16; ++dt) {
      if (dt * 16 < d) {
        acc[dt][0] *= alpha; acc[dt][1] *= alpha; acc[dt][2] *= alpha; acc[dt][3] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16_raw* vp = &Vt[(dt * 16 + c) * VS + 32 * t + 4 * g];
          const uint2 lo = *reinterpret_cast<const uint2*>(vp), hi = *reinterpret_cast<const uint2*>(vp + 16);
          const uint4 u = {lo.x, lo.y, hi.x, hi.y};
          acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, u), pf[t], acc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (q < Sq) {
    const float inv = 1.f / l;
    bf16_raw* op = O + ((long)b * Sq + q) * ldo + (long)h * d + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DP / 16; ++dt)
      if (dt * 16 < d) {
        const uint2 u = {pack_bf16(acc[dt][0] * inv, acc[dt][1] * inv), pack_bf16(acc[dt][2] * inv, acc[dt][3] * inv)};
        *reinterpret_cast<uint2*>(op + dt * 16) = u;
      }
  }
}

// ----------------------------------------------------------------------------------------------------------- fp32 Linear
template <typename T>
__device__ __forceinline__ float4 ld4(const T* p);
template <>
__device__ __forceinline__ float4 ld4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <>
__device__ __forceinline__ float4 ld4<bf16_raw>(const bf16_raw* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return float4{bf2f((bf16_raw)(u.x & 0xffff)), bf2f((bf16_raw)(u.x >> 16)), bf2f((bf16_raw)(u.y & 0xffff)), bf2f((bf16_raw)(u.y >> 16))};
}

// One wave per output element (m, n): lane j takes the groups of four k at 4 (j + 64 i), in ascending order, then the 6-level
// wave tree.  The head's matrices are at most 1024 x 768: nothing here is worth tiling.
template <typename T>
__global__ void __launch_bounds__(256) linear_rows_f32_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ out, long ldo, long MN,
                                                              int N, int K, int affine, float shift, float scale) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= MN) return;
  const long mrow = e / N;
  const int n = (int)(e - mrow * N);
  const T* xr = x + mrow * ldx;
  const float* wr = W + (long)n * K;
  float acc = 0.f;
  for (int k = 4 * lane; k < K; k += 256) {
    const float4 a = ld4<T>(xr + k), w = ld4<float>(wr + k);
    acc += a.x * w.x;
    acc += a.y * w.y;
    acc += a.z * w.z;
    acc += a.w * w.w;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    if (bias) acc += bias[n];
    if (affine) acc = (acc - shift) / scale;
    out[mrow * ldo + n] = acc;
  }
}

}  // namespace

extern "C" int mgx_xattn_fwd(const uint16_t* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv, uint16_t* O,
                             long ldo, int B, int H, int Sq, int Skv, int d, float scale, const int* kv_len, void* stream) {
  MGX_REQUIRE(q && k && v && O && B > 0 && H > 0 && Sq >= 1 && Skv >= 1, "bad argument");
  MGX_REQUIRE(d > 0 && d % 16 == 0 && d <= 128, "head dim must be a multiple of 16, at most 128");
  if (Sq > 4096 || Skv > 4096) return 1;                         // refused, nothing launched
  const long width = (long)H * d;
  MGX_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldo >= width, "row strides below H d");
  MGX_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "row strides must be multiples of 8 elements");
  MGX_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)O) & 15) == 0, "q, k, v and O must be 16-byte aligned");
  MGX_REQUIRE((long)B * H * ((Sq + 63) / 64) < (1L << 31), "too many workgroups");
  const int grid = B * H * ((Sq + 63) / 64);
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int dp = (d + 31) / 32 * 32;
  if (dp == 32) xattn_kernel<32><<<grid, 256, 0, st>>>(q, ldq, k, ldk, v, ldv, O, ldo, H, Sq, Skv, d, sl2, kv_len);
  else if (dp == 64) xattn_kernel<64><<<grid, 256, 0, st>>>(q, ldq, k, ldk, v, ldv, O, ldo, H, Sq, Skv, d, sl2, kv_len);
  else if (dp == 96) xattn_kernel<96><<<grid, 256, 0, st>>>(q, ldq, k, ldk, v, ldv, O, ldo, H, Sq, Skv, d, sl2, kv_len);
  else xattn_kernel<128><<<grid, 256, 0, st>>>(q, ldq, k, ldk, v, ldv, O, ldo, H, Sq, Skv, d, sl2, kv_len);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_linear_rows_f32(const void* x, int x_is_f32, long ldx, const float* W, const float* bias, float* out, long ldo,
                                   int M, int N, int K, int affine, float shift, float scale, void* stream) {
  MGX_REQUIRE(x && W && out && M >= 1 && N >= 1 && K >= 4 && K % 4 == 0, "M, N >= 1, K % 4 == 0");
  MGX_REQUIRE(ldx >= K && ldx % 4 == 0 && ldo >= N, "ldx >= K, ldx % 4 == 0, ldo >= N");
  MGX_REQUIRE(((uintptr_t)x & (x_is_f32 ? 15 : 7)) == 0 && ((uintptr_t)W & 15) == 0, "x and W must be aligned to four elements");
  MGX_REQUIRE(!affine || scale != 0.f, "scale must not be 0");
  const long MN = (long)M * N;
  const int grid = (int)((MN + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  if (x_is_f32)
    linear_rows_f32_kernel<float><<<grid, 256, 0, st>>>((const float*)x, ldx, W, bias, out, ldo, MN, N, K, affine, shift, scale);
  else
    linear_rows_f32_kernel<bf16_raw><<<grid, 256, 0, st>>>((const bf16_raw*)x, ldx, W, bias, out, ldo, MN, N, K, affine, shift, scale);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
