// The attention of the five inference-only encoders (CLIP image and text towers, T5, BLIP's ViT, ImageReward's cross-attending
// BERT): one kernel, its one (DP, CAUSAL, BIAS) dispatch and the three entry points that launch it.
//   mgx_vit_attn_fwd      packed q | k | v rows, no mask (the image towers)
//   mgx_text_attn_fwd     packed rows with a causal mask (CLIP text) or a relative-position bias (T5)
//   mgx_xattn_fwd         q, k and v in separate buffers (Sq != Skv allowed) and a key length per sample (BERT)
// The packed entry points pass qkv, qkv + width and qkv + 2 width with one row stride: on the same data all three give the
// same bits.
#include <type_traits>

#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

// One workgroup per (batch, head, block of 64 queries), four waves of 16 queries each.  Keys and values stream through LDS in
// blocks of 64 with an online softmax, so the sequence is not bounded by LDS.  The head dimension is zero-padded in LDS to DP,
// the next multiple of 32 (80 -> 96), for v_mfma_f32_16x16x32_bf16.
// Both products are taken transposed, so that a query stays on one lane column throughout:
//   S^T = K Q^T : A = K rows from LDS (16 bytes of one key), B = Q^T from registers -> lane (c = lane & 15, g = lane >> 4) holds
//                 the scores of query c against the keys 16 s + 4 g + r (s = 0..3 accumulators, r = 0..3 registers);
//   O^T = V^T P^T: B = P^T is those registers as they are: element j of the step t (32 keys) is key 32 t + 16 (j >> 2) + 4 g + (j & 3),
//                 and the A operand reads V^T in the same key order (two 8-byte reads of the transposed V image in LDS).
// Row maxima and sums are reduced over the four lanes of a query (xor 16, 32); the output lands with 4 consecutive head
// columns of one query per lane.
// q, k and v have their own base pointers and row strides, and their own row counts (Sq queries, Skv keys per sample).  Only
// the keys t < kvn count; kvn is Skv, or, in the instance without mask and bias, clamp(kv_len[b], 1, Skv) when it is given a
// kv_len.  The rows at or beyond kvn are not read at all: they are zeros in LDS, like the rows beyond the sequence, so that
// whatever they hold -- inf and NaN included -- meets neither the scores nor the P V product (0 x NaN is NaN on the matrix
// pipe), and their scores are -inf before the maximum is taken.  Key blocks that start at or beyond kvn are neither loaded nor
// multiplied.
// CAUSAL: key k counts for query q only if k <= q.  The key blocks from 64 (qb + 1) on lie wholly above the workgroup's last
//         query and are neither loaded nor multiplied.
// BIAS:   rel_bias [H][2 S - 1] fp32, rel_bias[h][k - q + S - 1] is added to scale * q.k before the maximum is taken.  A block
//         of 64 queries against 64 keys sees 127 consecutive distances: they are staged in LDS next to K and V (times log2 e,
//         the scores live in the exp2 domain).
// The CAUSAL and BIAS instances take Sq == Skv = S and no key lengths.  The last argument is the one pointer an instance can
// use: the bias table in the BIAS instances, the nullable kv_len in the others.
template <int DP, bool CAUSAL, bool BIAS>
__global__ void __launch_bounds__(256) encoder_attn_kernel(const bf16_raw* __restrict__ Q, long ldq, const bf16_raw* __restrict__ K,
                                                           long ldk, const bf16_raw* __restrict__ V, long ldv, bf16_raw* __restrict__ O,
                                                           long ldo, int H, int Sq, int Skv, int d, float scale_log2,
                                                           std::conditional_t<BIAS, const float*, const int*> __restrict__ aux) {
  constexpr int KS = DP + 8;     // elements between key rows of the K image
  constexpr int VS = 64 + 4;     // elements between head-column rows of the V^T image
  constexpr int CH = DP / 8;     // 16-byte chunks per key
  __shared__ __attribute__((aligned(16))) bf16_raw Ks[64 * KS];
  __shared__ __attribute__((aligned(16))) bf16_raw Vt[DP * VS];
  __shared__ float Bs[128];      // BIAS only (no LDS in the other instances): Bs[t] is the bias of distance k - q = k0 - 64 qb + t - 63
  const int nqb = (Sq + 63) / 64;
  const int qb = blockIdx.x % nqb, h = (blockIdx.x / nqb) % H, b = blockIdx.x / (nqb * H);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const bf16_raw* qbase = Q + (long)b * Sq * ldq + (long)h * d;
  const bf16_raw* kbase = K + (long)b * Skv * ldk + (long)h * d;
  const bf16_raw* vbase = V + (long)b * Skv * ldv + (long)h * d;
  const int q = qb * 64 + wave * 16 + c;
  int kvn = Skv;
  if constexpr (!CAUSAL && !BIAS) {
    if (aux) {
      kvn = aux[b];
      kvn = kvn < 1 ? 1 : (kvn > Skv ? Skv : kvn);
    }
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

  const int kend = CAUSAL ? (qb * 64 + 64 < kvn ? qb * 64 + 64 : kvn) : kvn;   // causal: nothing above the last query of the block
  for (int k0 = 0; k0 < kend; k0 += 64) {
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
      // the eight head columns of the one 16-byte load, element by element: taken apart through its 32-bit words instead, the
      // instance that reads kv_len compiles the load in two pieces (12 + 4 bytes), which the image towers' time shows
      const s16x8 w = __builtin_bit_cast(s16x8, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * VS + key] = (bf16_raw)w[e];
    }
    if constexpr (BIAS) {
      if (tid < 128) {
        const int idx = k0 - qb * 64 + tid - 63 + Skv - 1;  // inside [0, 2 S - 2] for every (query, key) pair of the sequence
        Bs[tid] = idx >= 0 && idx <= 2 * Skv - 2 ? aux[(long)h * (2 * Skv - 1) + idx] * 1.4426950408889634f : 0.f;
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
          v = k0 + 16 * s + 4 * g + r < kvn ? sc[s][r] * scale_log2 : -INFINITY;
        } else {
          const int kl = 16 * s + 4 * g + r;                // key inside the block
          bool in = k0 + kl < kvn;
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
    // finite: kvn >= 1, so key 0 is admitted in the first block and k0 < kvn in every later one.  Causal: the loop stops at the
    // block that holds the workgroup's queries, so k0 <= 64 qb <= q for every lane's query (stored or not): key k0 is admitted
    // in every block, and in the diagonal block a stored query also admits itself.  No row ever meets a block with nothing
    // admitted.
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

// What the entry points have checked and hand to the one dispatch.
struct AttnCall {
  const bf16_raw *q, *k, *v;
  long ldq, ldk, ldv;
  bf16_raw* O;
  long ldo;
  int B, H, Sq, Skv, d;
  float scale;
  void* stream;
};

template <bool CAUSAL, bool BIAS>
int launch(const AttnCall& a, std::conditional_t<BIAS, const float*, const int*> aux) {
  const int grid = a.B * a.H * ((a.Sq + 63) / 64);
  const float sl2 = a.scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)a.stream;
  auto go = [&](auto dp) {
    encoder_attn_kernel<decltype(dp)::value, CAUSAL, BIAS><<<grid, 256, 0, st>>>(a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.O, a.ldo, a.H,
                                                                                a.Sq, a.Skv, a.d, sl2, aux);
  };
  const int dp = (a.d + 31) / 32 * 32;
  if (dp == 32) go(std::integral_constant<int, 32>{});
  else if (dp == 64) go(std::integral_constant<int, 64>{});
  else if (dp == 96) go(std::integral_constant<int, 96>{});
  else go(std::integral_constant<int, 128>{});
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

// The argument checks of the two packed entry points; 0, 1 (S > 4096: refused, nothing launched) or a negative code.
int packed_check(const void* qkv, long ld_qkv, const void* O, long ldo, int B, int H, int S, int d) {
  MGX_REQUIRE(qkv && O && B > 0 && H > 0 && S >= 1, "bad argument");
  MGX_REQUIRE(d > 0 && d % 16 == 0 && d <= 128, "head dim must be a multiple of 16, at most 128");
  if (S > 4096) return 1;
  const long width = (long)H * d;
  MGX_REQUIRE(ld_qkv >= 3L * width && ld_qkv % 8 == 0 && ldo >= width && ldo % 4 == 0, "row strides: ld_qkv % 8, ldo % 4");
  MGX_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)O & 15) == 0, "qkv and O must be 16-byte aligned");
  MGX_REQUIRE((long)B * H * ((S + 63) / 64) < (1L << 31), "too many workgroups");
  return MGX_OK;
}

AttnCall packed_call(const uint16_t* qkv, long ld, uint16_t* O, long ldo, int B, int H, int S, int d, float scale, void* stream) {
  const int width = H * d;
  return AttnCall{qkv, qkv + width, qkv + 2 * width, ld, ld, ld, O, ldo, B, H, S, S, d, scale, stream};
}

}  // namespace

extern "C" int mgx_vit_attn_fwd(const uint16_t* qkv, long ld_qkv, uint16_t* O, long ldo, int B, int H, int S, int d, float scale,
                                void* stream) {
  const int rc = packed_check(qkv, ld_qkv, O, ldo, B, H, S, d);
  if (rc != MGX_OK) return rc;                                   // 1: S > 4096, refused, nothing launched
  return launch<false, false>(packed_call(qkv, ld_qkv, O, ldo, B, H, S, d, scale, stream), nullptr);
}

extern "C" int mgx_text_attn_fwd(const uint16_t* qkv, long ld_qkv, uint16_t* O, long ldo, int B, int H, int S, int d, float scale,
                                 int causal, const float* rel_bias, void* stream) {
  if (!causal && !rel_bias) return mgx_vit_attn_fwd(qkv, ld_qkv, O, ldo, B, H, S, d, scale, stream);   // the image towers' path itself
  const int rc = packed_check(qkv, ld_qkv, O, ldo, B, H, S, d);
  if (rc != MGX_OK) return rc;                                   // 1: S > 4096, refused, nothing launched
  const AttnCall a = packed_call(qkv, ld_qkv, O, ldo, B, H, S, d, scale, stream);
  if (rel_bias) return causal ? launch<true, true>(a, rel_bias) : launch<false, true>(a, rel_bias);
  return launch<true, false>(a, nullptr);
}

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
  return launch<false, false>(AttnCall{q, k, v, ldq, ldk, ldv, O, ldo, B, H, Sq, Skv, d, scale, stream}, kv_len);
}
