// Multi-head attention straight from the packed q | k | v projection: the body shared by mgx_vit_attn_fwd (clip.hip, the
// image tower: non-causal, no bias) and mgx_text_attn_fwd (text.hip: CLIP text with a causal mask, T5 with a relative-position
// bias).  CAUSAL and BIAS are compile-time flags; with both off the kernel is the image tower's as it always was, instruction
// for instruction (its argument list included: the bias table is an argument of the BIAS instances only).
#pragma once
#include "common.h"

// One workgroup per (batch, head, block of 64 queries), four waves of 16 queries each.  Keys and values stream through LDS in
// blocks of 64 with an online softmax, so S is not bounded by LDS.  The head dimension is zero-padded in LDS to DP, the next
// multiple of 32 (80 -> 96), for v_mfma_f32_16x16x32_bf16.
// Both products are taken transposed, so that a query stays on one lane column throughout:
//   S^T = K Q^T : A = K rows from LDS (16 bytes of one key), B = Q^T from registers -> lane (c = lane & 15, g = lane >> 4) holds
//                 the scores of query c against the keys 16 s + 4 g + r (s = 0..3 accumulators, r = 0..3 registers);
//   O^T = V^T P^T: B = P^T is those registers as they are: element j of the step t (32 keys) is key 32 t + 16 (j >> 2) + 4 g + (j & 3),
//                 and the A operand reads V^T in the same key order (two 8-byte reads of the transposed V image in LDS).
// Row maxima and sums are reduced over the four lanes of a query (xor 16, 32); the output lands with 4 consecutive head
// columns of one query per lane.
// CAUSAL: key k counts for query q only if k <= q.  The key blocks from 64 (qb + 1) on lie wholly above the workgroup's last
//         query and are neither loaded nor multiplied.
// BIAS:   rel_bias [H][2 S - 1] fp32, rel_bias[h][k - q + S - 1] is added to scale * q.k before the maximum is taken.  A block
//         of 64 queries against 64 keys sees 127 consecutive distances: they are staged in LDS next to K and V (times log2 e,
//         the scores live in the exp2 domain).
namespace {   // per translation unit, as the image tower's kernel always was

template <bool BIAS>
struct BiasLds {          // no LDS at all in the instances without a bias
  __device__ static __forceinline__ float* get() { return nullptr; }
};
template <>
struct BiasLds<true> {
  __device__ static __forceinline__ float* get() {
    __shared__ float B[128];
    return B;
  }
};

__device__ __forceinline__ const float* bias_table() { return nullptr; }
__device__ __forceinline__ const float* bias_table(const float* p) { return p; }

// RelBias: nothing, or `const float* rel_bias` when BIAS -- the instance without mask and bias keeps the image tower's
// argument list.
template <int DP, bool CAUSAL, bool BIAS, typename... RelBias>
__global__ void __launch_bounds__(256) vit_attn_kernel(const bf16_raw* __restrict__ qkv, long ld, bf16_raw* __restrict__ O, long ldo,
                                                       int H, int S, int d, int width, float scale_log2, RelBias... rel_bias_arg) {
  static_assert(sizeof...(RelBias) == (BIAS ? 1 : 0), "the bias table is an argument of the BIAS instances only");
  const float* const rel_bias = bias_table(rel_bias_arg...);
  constexpr int KS = DP + 8;     // elements between key rows of the K image
  constexpr int VS = 64 + 4;     // elements between head-column rows of the V^T image
  constexpr int CH = DP / 8;     // 16-byte chunks per key
  __shared__ __attribute__((aligned(16))) bf16_raw Ks[64 * KS];
  __shared__ __attribute__((aligned(16))) bf16_raw Vt[DP * VS];
  float* const Bs = BiasLds<BIAS>::get();   // Bs[t]: the bias of distance k - q = k0 - 64 qb + t - 63
  const int nqb = (S + 63) / 64;
  const int qb = blockIdx.x % nqb, h = (blockIdx.x / nqb) % H, b = blockIdx.x / (nqb * H);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const bf16_raw* base = qkv + (long)b * S * ld + (long)h * d;
  const int q = qb * 64 + wave * 16 + c;

  s16x8 qf[DP / 32];
#pragma unroll
  for (int ks = 0; ks < DP / 32; ++ks) {
    const int col = 32 * ks + 8 * g;
    uint4 u = {0u, 0u, 0u, 0u};
    if (q < S && col < d) u = *reinterpret_cast<const uint4*>(base + (long)q * ld + col);
    qf[ks] = __builtin_bit_cast(s16x8, u);
  }
  f32x4 acc[DP / 16];
#pragma unroll
  for (int i = 0; i < DP / 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  const int kend = CAUSAL ? (qb * 64 + 64 < S ? qb * 64 + 64 : S) : S;   // causal: nothing above the last query of the block
  for (int k0 = 0; k0 < kend; k0 += 64) {
    __syncthreads();                                        // the block before this one has been consumed
    for (int i = tid; i < 64 * CH; i += 256) {
      const int key = i / CH, ch = i % CH;
      uint4 u = {0u, 0u, 0u, 0u};
      if (k0 + key < S && ch * 8 < d) u = *reinterpret_cast<const uint4*>(base + width + (long)(k0 + key) * ld + ch * 8);
      *reinterpret_cast<uint4*>(&Ks[key * KS + ch * 8]) = u;
    }
    for (int i = tid; i < 64 * CH; i += 256) {
      const int key = i & 63, ch = i >> 6;
      uint4 u = {0u, 0u, 0u, 0u};
      if (k0 + key < S && ch * 8 < d) u = *reinterpret_cast<const uint4*>(base + 2 * width + (long)(k0 + key) * ld + ch * 8);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Vt[(ch * 8 + 2 * e) * VS + key] = (bf16_raw)(w[e] & 0xffff);
        Vt[(ch * 8 + 2 * e + 1) * VS + key] = (bf16_raw)(w[e] >> 16);
      }
    }
    if constexpr (BIAS) {
      if (tid < 128) {
        const int idx = k0 - qb * 64 + tid - 63 + S - 1;    // inside [0, 2 S - 2] for every (query, key) pair of the sequence
        Bs[tid] = idx >= 0 && idx <= 2 * S - 2 ? rel_bias[(long)h * (2 * S - 1) + idx] * 1.4426950408889634f : 0.f;
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
        float v;
        if constexpr (!CAUSAL && !BIAS) {
          v = k0 + 16 * s + 4 * g + r < S ? sc[s][r] * scale_log2 : -INFINITY;
        } else {
          const int kl = 16 * s + 4 * g + r;                // key inside the block
          bool in = k0 + kl < S;
          if constexpr (CAUSAL) in = in && k0 + kl <= q;
          v = sc[s][r] * scale_log2;
          if constexpr (BIAS) v += Bs[kl - (wave * 16 + c) + 63];
          v = in ? v : -INFINITY;
        }
        sc[s][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // finite: key k0 is inside the sequence.  Causal: the loop stops at the block that holds the workgroup's queries, so
    // k0 <= 64 qb <= q for every lane's query (stored or not): key k0 is admitted in every block, and in the diagonal block a
    // stored query also admits itself.  No row ever meets a block with nothing admitted.
    const float mn = fmaxf(m, mx);
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
  if (q < S) {
    const float inv = 1.f / l;
    bf16_raw* op = O + ((long)b * S + q) * ldo + (long)h * d + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DP / 16; ++dt)
      if (dt * 16 < d) {
        const uint2 u = {pack_bf16(acc[dt][0] * inv, acc[dt][1] * inv), pack_bf16(acc[dt][2] * inv, acc[dt][3] * inv)};
        *reinterpret_cast<uint2*>(op + dt * 16) = u;
      }
  }
}

}  // namespace

// The argument checks both entry points share; 0, 1 (S > 4096: refused, nothing launched) or a negative code.
static inline int vit_attn_check(const void* qkv, long ld_qkv, const void* O, long ldo, int B, int H, int S, int d) {
  MGX_REQUIRE(qkv && O && B > 0 && H > 0 && S >= 1, "bad argument");
  MGX_REQUIRE(d > 0 && d % 16 == 0 && d <= 128, "head dim must be a multiple of 16, at most 128");
  if (S > 4096) return 1;
  const long width = (long)H * d;
  MGX_REQUIRE(ld_qkv >= 3L * width && ld_qkv % 8 == 0 && ldo >= width && ldo % 4 == 0, "row strides: ld_qkv % 8, ldo % 4");
  MGX_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)O & 15) == 0, "qkv and O must be 16-byte aligned");
  MGX_REQUIRE((long)B * H * ((S + 63) / 64) < (1L << 31), "too many workgroups");
  return MGX_OK;
}
