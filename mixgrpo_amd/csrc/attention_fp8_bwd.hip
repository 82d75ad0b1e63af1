// fp8 (OCP e4m3) backward of the joint attention: the gradient of the function attn_fwd_fp8_kernel ran (attention_fp8.hip),
// opt-in (MGX_ATTN_FP8_BWD, mixgrpo_amd/ops.py); without it the fp8 path trains through the bf16 mgx_attn_bwd.
//
// The reference has no fp8 attention (see attention_fp8.hip).  This is the straight-through gradient of the quantised
// forward: S is recomputed from the same e4m3 Q8, K8 with the forward's instruction and operand order, so
// P = exp2(c * s - lse * log2 e) is the forward's probability and its rows sum to 1; dP uses V8, not the bf16 V.
// All five products run on v_mfma_scale_f32_32x32x64_f8f6f4.  Two kernels, no atomics, bit-reproducible, split as the bf16 pair:
//   attn_bwd_fp8_dkv_kernel : a wave owns 32 keys (K8, V8 fragments in registers), the workgroup (4 waves = 128 keys) sweeps
//                             64-query tiles (two 32-query score blocks: the K = 64 of one MFMA) through two LDS buffers;
//                             S = Q K^T and dP = dO V^T with the KEY on the lane, so P8 and dS8 are the B operands of
//                             dV^T += dO8t P8 and dK^T += Q8t dS8 straight from the accumulators.
//   attn_bwd_fp8_dq_kernel  : a wave owns 32 queries (Q8, dO8 fragments, lse and delta in registers), the workgroup (128 queries)
//                             sweeps 64-key tiles; S^T = K Q^T, dP^T = V dO^T with the QUERY on the lane, dQ^T += K8t dS8^T.
// Quantisation points (tests/attn_fp8_bwd_refs.py mirrors them):
//   Q8, K8, V8 : the forward's quantiser on the bf16 Q, K, V handed in (same inputs, same bits);  dO8: the same, amax row 3;
//   Q8t, K8t, dO8t [B,H,128,Sp]: transposed images, the columns of every 64-block in the order the accumulator hands them to
//                the MFMA (the V8t trick), zero from column S on;
//   P8 = e4m3(256 P): P <= 1, a fixed power of two, representable down to 2^-17;
//   dS8: dS = P (dP - delta) has no a-priori bound, so it is MX-blocked: 32 contiguous values along the contraction dimension
//        (one column of a 32 x 32 accumulator block, held by the two lane halves) share 2^e, e = floor(log2(448 / amax)); the
//        lanes store e4m3(dS 2^e) and pass the E8M0 byte 127 - e as that operand's block scale (the other operand keeps 0x7F;
//        an all-zero block: byte 127).  mx_blocks has the hardware's map of scale bytes to values.
// Row statistics, delta, the accumulators and the outputs stay fp32 / bf16 as in mgx_attn_bwd; dequantisation factors and
// `scale` are applied once, in the epilogue.  attn_bwd_prep_kernel is reused unchanged for dOt; delta is then rewritten from
// the dequantised dO8 (fp8_delta_kernel says why).
// Ragged tails: every global read is clamped in bounds; keys and queries >= S contribute exact zeros by selects; only rows < S
// of dQ, dK, dV are written.
#include "../../include/mixgrpo_hip.h"
#include "attn_fp8_quant.h"
#include "common.h"

#include <type_traits>

namespace {

constexpr int HD = 128;
constexpr int TILE8 = 64 * HD;     // one 64-row e4m3 tile, row-major or transposed: 8 KiB
constexpr float F8_MAX = 448.0f;
constexpr float LOG2E = 1.4426950408889634f;

struct BwdF8Args {
  const uint8_t *Q8, *K8, *V8, *dO8;   // [B,H,S,128]
  const uint8_t *Q8t, *K8t, *dO8t;     // [B,H,128,Sp]
  const float* amax;                   // [4][B*H]: Q, K, V, dO
  const float* lse;                    // [B,H,S]
  const float* delta;                  // [B,H,S]
  bf16_raw *dQ, *dK, *dV;              // [B,H,S,128]
  int B, H, S, Sp;
  float scale, scale_log2e;
};

#define MFMA_F8(A_, B_, C_) \
  __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A_, B_, C_, 0, 0, 0, one_e8m0, 0, one_e8m0)
// B carries an MX block scale (the same E8M0 byte in all four byte lanes of SB_, so the byte select does not matter)
#define MFMA_F8_SB(A_, B_, C_, SB_) \
  __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A_, B_, C_, 0, 0, 0, one_e8m0, 0, SB_)

__device__ __forceinline__ float dequant(float amax) { return fmaxf(amax, 1e-30f) * (1.0f / F8_MAX); }

// The score factor, computed exactly as attn_fwd_fp8_kernel computes it.
__device__ __forceinline__ float score_c(float scale_log2e, float aq, float ak) {
  return fmaxf(scale_log2e * (fmaxf(aq, 1e-30f) * (1.0f / F8_MAX)) * (fmaxf(ak, 1e-30f) * (1.0f / F8_MAX)), 1e-30f);
}

// The 2 x 16 fp32 values of one lane (two accumulator blocks) -> the lane's e4m3 fragment and its E8M0 scale operand.
// Which values share a hardware block scale was settled with exact data (ones in one quarter of an operand, lane l passing 2^l):
// dwords 0-3 of BOTH lane halves -- accumulator block 0, 32 contiguous rows of the score tile -- take the byte of lane r,
// dwords 4-7 of both halves -- block 1 -- the byte of lane r + 32.  So an MX block is one column of one 32 x 32 accumulator
// block, its amax one exchange between the two lane halves, and lane half h passes the scale of block h.
// e = floor(log2(448 / amax)) from the exponent and mantissa bits of amax (448 = 1.75 * 2^8), clamped to what a float power of
// two and the E8M0 byte hold; amax == 0: e = 0.
__device__ __forceinline__ void mx_blocks(const f32x16 (&x)[2], int h, i32x8& frag, int& scale_op) {
  int eb[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) am = fmaxf(am, fabsf(x[b][i]));
    am = fmaxf(am, __shfl_xor(am, 32, 64));
    const uint32_t u = __builtin_bit_cast(uint32_t, am);
    int e = 135 - (int)(u >> 23) - ((u & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    e = min(max(e, -126), 127);
    if (am == 0.f) e = 0;
    eb[b] = e;
    const float sc = __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      int wv = 0;
      wv = __builtin_amdgcn_cvt_pk_fp8_f32(x[b][4 * i4] * sc, x[b][4 * i4 + 1] * sc, wv, false);
      wv = __builtin_amdgcn_cvt_pk_fp8_f32(x[b][4 * i4 + 2] * sc, x[b][4 * i4 + 3] * sc, wv, true);
      frag[b * 4 + i4] = wv;
    }
  }
  scale_op = (127 - (h ? eb[1] : eb[0])) * 0x01010101;
}

// ------------------------------------------------------------------------------------------------ delta
// delta[b,h,s] = sum_d dO8 * O, dequantised: the row sum that belongs to dP = dO8 V8^T.  sum_k P (dP - delta) = 0 needs delta
// from the SAME dO as dP; with the prep kernel's delta (bf16 dO) the mismatch dO - dO8 is not cancelled and, on peaked rows
// where dP - delta is a small difference, costs dQ and dK 5.4-6.2e-2 relative L2 instead of 3.7e-2 (fp64 emulation, gaussian
// inputs at amplitude 2).  One wave per row, two elements per lane; overwrites what the prep kernel wrote.
__global__ void __launch_bounds__(256) fp8_delta_kernel(const uint8_t* __restrict__ dO8, const bf16_raw* __restrict__ O, long ldo,
                                                        long o_bstride, const float* __restrict__ amax_do,
                                                        float* __restrict__ delta, int H, int S, long rows) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {
    const int bh = (int)(row / S), s_ = (int)(row - (long)bh * S);
    const int d8 = *reinterpret_cast<const uint16_t*>(dO8 + row * HD + 2 * lane);
    const uint32_t uo = *reinterpret_cast<const uint32_t*>(O + (long)(bh / H) * o_bstride + (long)s_ * ldo + (bh % H) * HD + 2 * lane);
    float acc = __builtin_amdgcn_cvt_f32_fp8(d8, 0) * bf2f(uo & 0xffff) + __builtin_amdgcn_cvt_f32_fp8(d8, 1) * bf2f(uo >> 16);
    acc = wave_sum(acc);
    if (lane == 0) delta[row] = acc * dequant(amax_do[bh]);
  }
}

// ------------------------------------------------------------------------------------------------ dK, dV
// LDS per 64-query tile: Q8 [64][128] | dO8 [64][128] | Q8t [128][64] | dO8t [128][64] | lse * log2 e - 8 [64] | delta [64]
constexpr int DKV_STAGE = 4 * TILE8 + 512;
// One workgroup per CU: 128 accumulators (dV^T, dK^T) + 64 (S, dP of a 64-query tile) + the K8 / V8 fragments do not fit the 256
// registers of two waves per SIMD (hipcc spills 213 of them into the tile loop); with 512 the accumulators sit in AGPRs, no scratch.
__global__ void __launch_bounds__(256, 1) attn_bwd_fp8_dkv_kernel(BwdF8Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  int one_e8m0 = 0x7F7F7F7F;
  asm volatile("" : "+v"(one_e8m0));

  const int nkb = (g.S + 127) / 128;
  int bid = blockIdx.x;
  xcd_remap(bid, nkb * g.H * g.B);
  const int kt = bid % nkb, bh = bid / nkb;
  const int BH = g.B * g.H;
  const float aq = g.amax[bh], ak = g.amax[BH + bh], av = g.amax[2 * BH + bh], ado = g.amax[3 * BH + bh];
  const float c = score_c(g.scale_log2e, aq, ak);
  const float fdp = dequant(ado) * dequant(av);          // raw dP -> dP

  const long bhS = (long)bh * g.S;
  const uint8_t* Qp = g.Q8 + bhS * HD;
  const uint8_t* dOp = g.dO8 + bhS * HD;
  const uint8_t* Qtp = g.Q8t + (long)bh * HD * g.Sp;
  const uint8_t* dOtp = g.dO8t + (long)bh * HD * g.Sp;
  const float* lsep = g.lse + bhS;
  const float* dltp = g.delta + bhS;

  // own key: K8 and V8 rows as B operands, B[k = d][col = key]
  const int key0 = kt * 128 + wid * 32;
  const bool key_valid = key0 + r < g.S;
  const int krow = key_valid ? key0 + r : g.S - 1;
  i32x8 kf[2], vf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const char* pk = reinterpret_cast<const char*>(g.K8 + (bhS + krow) * HD + ks * 64 + h * 32);
    const char* pv = reinterpret_cast<const char*>(g.V8 + (bhS + krow) * HD + ks * 64 + h * 32);
    kf[ks] = frag32(pk, pk + 16);
    vf[ks] = frag32(pv, pv + 16);
  }
  f32x16 dv[4], dk[4];   // dV^T, dK^T: rows d = 32 dt + ..., column = key r
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dv[dt][i] = dk[dt][i] = 0.f;

  // staging: every 8 KiB tile is 512 16-byte chunks, two per thread
  uint4 sq0, sq1, sdo0, sdo1, sqt0, sqt1, sdot0, sdot1;   // (named, not arrays: arrays captured by the tile lambda stay in scratch)
  float sl = 0.f;
  const int nqt = (g.S + 63) / 64;
#define DKV_LOAD1(t, j)                                                                                          \
  do {                                                                                                           \
    const int id = tid + 256 * (j);                                                                              \
    int qa = (t) * 64 + (id >> 3);                                                                               \
    if (qa >= g.S) qa = g.S - 1;                                                                                 \
    sq##j = *reinterpret_cast<const uint4*>(Qp + (long)qa * HD + (id & 7) * 16);                                 \
    sdo##j = *reinterpret_cast<const uint4*>(dOp + (long)qa * HD + (id & 7) * 16);                               \
    sqt##j = *reinterpret_cast<const uint4*>(Qtp + (long)(id >> 2) * g.Sp + (t) * 64 + (id & 3) * 16);           \
    sdot##j = *reinterpret_cast<const uint4*>(dOtp + (long)(id >> 2) * g.Sp + (t) * 64 + (id & 3) * 16);         \
  } while (0)
#define DKV_LOAD(t)                                                                                              \
  do {                                                                                                           \
    DKV_LOAD1(t, 0);                                                                                             \
    DKV_LOAD1(t, 1);                                                                                             \
    if (tid < 128) {                                                                                             \
      int qa = (t) * 64 + (tid & 63);                                                                            \
      if (qa >= g.S) qa = g.S - 1;                                                                               \
      sl = tid < 64 ? lsep[qa] * LOG2E - 8.0f : dltp[qa];                                                        \
    }                                                                                                            \
  } while (0)
#define DKV_STORE1(buf, j)                                                                                       \
  do {                                                                                                           \
    char* base_ = smem + (buf) * DKV_STAGE;                                                                      \
    const int id = tid + 256 * (j);                                                                              \
    *reinterpret_cast<uint4*>(base_ + k8_off(id >> 3, id & 7)) = sq##j;                                          \
    *reinterpret_cast<uint4*>(base_ + TILE8 + k8_off(id >> 3, id & 7)) = sdo##j;                                 \
    *reinterpret_cast<uint4*>(base_ + 2 * TILE8 + v8_off(id >> 2, id & 3)) = sqt##j;                             \
    *reinterpret_cast<uint4*>(base_ + 3 * TILE8 + v8_off(id >> 2, id & 3)) = sdot##j;                            \
  } while (0)
#define DKV_STORE(buf)                                                                                           \
  do {                                                                                                           \
    char* base_ = smem + (buf) * DKV_STAGE;                                                                      \
    DKV_STORE1(buf, 0);                                                                                          \
    DKV_STORE1(buf, 1);                                                                                          \
    if (tid < 128) reinterpret_cast<float*>(base_ + 4 * TILE8)[tid] = sl;                                        \
  } while (0)

  DKV_LOAD(0);
  DKV_STORE(0);
  __syncthreads();
  int cur = 0;
  auto tile = [&](int t, auto mask_tag) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_tag)::value;
    const char* base = smem + cur * DKV_STAGE;
    const float* nls = reinterpret_cast<const float*>(base + 4 * TILE8);   // lse * log2 e - 8 per query of the tile
    const float* dls = nls + 64;                                           // delta
    // ---- S and dP blocks (32 queries x 32 keys) x 2; S with the forward's two MFMAs in the forward's order
    f32x16 s[2], dp[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      i32x8 qa[2], da[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        qa[ks] = frag32(base + k8_off(qb * 32 + r, 4 * ks + 2 * h), base + k8_off(qb * 32 + r, 4 * ks + 2 * h + 1));
        da[ks] = frag32(base + TILE8 + k8_off(qb * 32 + r, 4 * ks + 2 * h), base + TILE8 + k8_off(qb * 32 + r, 4 * ks + 2 * h + 1));
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) s[qb][i] = dp[qb][i] = 0.f;
      s[qb] = MFMA_F8(qa[0], kf[0], s[qb]);
      s[qb] = MFMA_F8(qa[1], kf[1], s[qb]);
      dp[qb] = MFMA_F8(da[0], vf[0], dp[qb]);
      dp[qb] = MFMA_F8(da[1], vf[1], dp[qb]);
    }
    // the next tile's staging loads: issued here, not at the top -- their 33 registers would be live through the S / dP phase,
    // the register peak of the kernel; they have the exponentials and the dV / dK products to land
    if (t + 1 < nqt) DKV_LOAD(t + 1);
    // ---- 256 P and 256 dS per (query, key); register 4 j + e of block qb is query 32 qb + 8 j + 4 h + e of the tile
    i32x8 pf, dsf;
    int ds_scale;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ql = qb * 32 + 8 * j + 4 * h;
        const float4 l4 = *reinterpret_cast<const float4*>(nls + ql);
        const float4 d4 = *reinterpret_cast<const float4*>(dls + ql);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
        float p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          p[e] = __builtin_amdgcn_exp2f(fmaf(s[qb][4 * j + e], c, -lv[e]));
          bool live = key_valid;
          if (MASK) live = live && (t * 64 + ql + e < g.S);
          if (!live) p[e] = 0.f;
          s[qb][4 * j + e] = p[e] * fmaf(dp[qb][4 * j + e], fdp, -dl[e]);      // s now holds 256 dS
        }
        int wv = 0;
        wv = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], wv, false);
        wv = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], wv, true);
        pf[qb * 4 + j] = wv;
      }
    mx_blocks(s, h, dsf, ds_scale);
    // ---- dV^T += dO8t P8, dK^T += Q8t dS8: the 64-query tile is one K = 64 step per 32-row d tile
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const i32x8 dot = frag32(base + 3 * TILE8 + v8_off(dt * 32 + r, 2 * h), base + 3 * TILE8 + v8_off(dt * 32 + r, 2 * h + 1));
      const i32x8 qt = frag32(base + 2 * TILE8 + v8_off(dt * 32 + r, 2 * h), base + 2 * TILE8 + v8_off(dt * 32 + r, 2 * h + 1));
      dv[dt] = MFMA_F8(dot, pf, dv[dt]);
      dk[dt] = MFMA_F8_SB(qt, dsf, dk[dt], ds_scale);
    }
    if (t + 1 < nqt) DKV_STORE(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  };
  const int nfull = g.S / 64;
  for (int t = 0; t < nfull; ++t) tile(t, std::false_type{});
  if (nfull < nqt) tile(nfull, std::true_type{});

  if (key_valid) {
    const float fv = dequant(ado) * (1.0f / 256.0f);                    // dO8 = dO 448 / ado, P8 = 256 P
    const float fk = g.scale * dequant(aq) * (1.0f / 256.0f);           // Q8 = Q 448 / aq, the block holds 256 dS
    bf16_raw* dkp = g.dK + (bhS + key0 + r) * HD;
    bf16_raw* dvp = g.dV + (bhS + key0 + r) * HD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const int d = dt * 32 + 8 * i4 + 4 * h;
        *reinterpret_cast<uint2*>(dkp + d) = make_uint2(pack_bf16(dk[dt][4 * i4] * fk, dk[dt][4 * i4 + 1] * fk),
                                                        pack_bf16(dk[dt][4 * i4 + 2] * fk, dk[dt][4 * i4 + 3] * fk));
        *reinterpret_cast<uint2*>(dvp + d) = make_uint2(pack_bf16(dv[dt][4 * i4] * fv, dv[dt][4 * i4 + 1] * fv),
                                                        pack_bf16(dv[dt][4 * i4 + 2] * fv, dv[dt][4 * i4 + 3] * fv));
      }
  }
}

// ------------------------------------------------------------------------------------------------ dQ
// LDS per 64-key tile: K8 [64][128] | V8 [64][128] | K8t [128][64]
constexpr int DQ_STAGE = 3 * TILE8;
__global__ void __launch_bounds__(256, 2) attn_bwd_fp8_dq_kernel(BwdF8Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  int one_e8m0 = 0x7F7F7F7F;
  asm volatile("" : "+v"(one_e8m0));

  const int nq = (g.S + 127) / 128;
  int bid = blockIdx.x;
  xcd_remap(bid, nq * g.H * g.B);
  const int qt = bid % nq, bh = bid / nq;
  const int BH = g.B * g.H;
  const float aq = g.amax[bh], ak = g.amax[BH + bh], av = g.amax[2 * BH + bh], ado = g.amax[3 * BH + bh];
  const float c = score_c(g.scale_log2e, aq, ak);
  const float fdp = dequant(ado) * dequant(av);

  const long bhS = (long)bh * g.S;
  const uint8_t* Kp = g.K8 + bhS * HD;
  const uint8_t* Vp = g.V8 + bhS * HD;
  const uint8_t* Ktp = g.K8t + (long)bh * HD * g.Sp;

  // own query: Q8 and dO8 rows as B operands of S^T = K Q^T and dP^T = V dO^T, lse and delta per lane
  const int q0 = qt * 128 + wid * 32;
  const bool q_valid = q0 + r < g.S;
  const int qrow = q_valid ? q0 + r : g.S - 1;
  i32x8 qf[2], dof[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const char* pq = reinterpret_cast<const char*>(g.Q8 + (bhS + qrow) * HD + ks * 64 + h * 32);
    const char* pd = reinterpret_cast<const char*>(g.dO8 + (bhS + qrow) * HD + ks * 64 + h * 32);
    qf[ks] = frag32(pq, pq + 16);
    dof[ks] = frag32(pd, pd + 16);
  }
  const float nl = g.lse[bhS + qrow] * LOG2E - 8.0f;
  const float dl = g.delta[bhS + qrow];
  f32x16 dq[4];   // dQ^T: rows d = 32 dt + ..., column = query r
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;

  uint4 sk0, sk1, sv0, sv1, skt0, skt1;
  const int ntiles = (g.S + 63) / 64;
#define DQ_LOAD1(t, j)                                                                                           \
  do {                                                                                                           \
    const int id = tid + 256 * (j);                                                                              \
    int ka = (t) * 64 + (id >> 3);                                                                               \
    if (ka >= g.S) ka = g.S - 1;                                                                                 \
    sk##j = *reinterpret_cast<const uint4*>(Kp + (long)ka * HD + (id & 7) * 16);                                 \
    sv##j = *reinterpret_cast<const uint4*>(Vp + (long)ka * HD + (id & 7) * 16);                                 \
    skt##j = *reinterpret_cast<const uint4*>(Ktp + (long)(id >> 2) * g.Sp + (t) * 64 + (id & 3) * 16);           \
  } while (0)
#define DQ_LOAD(t)                                                                                               \
  do {                                                                                                           \
    DQ_LOAD1(t, 0);                                                                                              \
    DQ_LOAD1(t, 1);                                                                                              \
  } while (0)
#define DQ_STORE1(buf, j)                                                                                        \
  do {                                                                                                           \
    char* base_ = smem + (buf) * DQ_STAGE;                                                                       \
    const int id = tid + 256 * (j);                                                                              \
    *reinterpret_cast<uint4*>(base_ + k8_off(id >> 3, id & 7)) = sk##j;                                          \
    *reinterpret_cast<uint4*>(base_ + TILE8 + k8_off(id >> 3, id & 7)) = sv##j;                                  \
    *reinterpret_cast<uint4*>(base_ + 2 * TILE8 + v8_off(id >> 2, id & 3)) = skt##j;                             \
  } while (0)
#define DQ_STORE(buf)                                                                                            \
  do {                                                                                                           \
    char* base_ = smem + (buf) * DQ_STAGE;                                                                       \
    DQ_STORE1(buf, 0);                                                                                           \
    DQ_STORE1(buf, 1);                                                                                           \
  } while (0)

  DQ_LOAD(0);
  DQ_STORE(0);
  __syncthreads();
  int cur = 0;
  auto tile = [&](int t, auto mask_tag) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_tag)::value;
    if (t + 1 < ntiles) DQ_LOAD(t + 1);
    const char* base = smem + cur * DQ_STAGE;
    // ---- S^T and dP^T blocks (32 keys x 32 queries) x 2; S^T exactly as attn_fwd_fp8_kernel forms it
    f32x16 s[2], dp[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      i32x8 ka[2], va[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        ka[ks] = frag32(base + k8_off(kb * 32 + r, 4 * ks + 2 * h), base + k8_off(kb * 32 + r, 4 * ks + 2 * h + 1));
        va[ks] = frag32(base + TILE8 + k8_off(kb * 32 + r, 4 * ks + 2 * h), base + TILE8 + k8_off(kb * 32 + r, 4 * ks + 2 * h + 1));
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = dp[kb][i] = 0.f;
      s[kb] = MFMA_F8(ka[0], qf[0], s[kb]);
      s[kb] = MFMA_F8(ka[1], qf[1], s[kb]);
      dp[kb] = MFMA_F8(va[0], dof[0], dp[kb]);
      dp[kb] = MFMA_F8(va[1], dof[1], dp[kb]);
    }
    // ---- 256 dS^T; register i of block kb is key 32 kb + 8 (i >> 2) + 4 h + (i & 3) of the tile
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float p = __builtin_amdgcn_exp2f(fmaf(s[kb][i], c, -nl));
        if (MASK && t * 64 + kb * 32 + 8 * (i >> 2) + 4 * h + (i & 3) >= g.S) p = 0.f;
        s[kb][i] = p * fmaf(dp[kb][i], fdp, -dl);
      }
    i32x8 dsf;
    int ds_scale;
    mx_blocks(s, h, dsf, ds_scale);
    // ---- dQ^T += K8t dS8^T
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const i32x8 ktf = frag32(base + 2 * TILE8 + v8_off(dt * 32 + r, 2 * h), base + 2 * TILE8 + v8_off(dt * 32 + r, 2 * h + 1));
      dq[dt] = MFMA_F8_SB(ktf, dsf, dq[dt], ds_scale);
    }
    if (t + 1 < ntiles) DQ_STORE(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  };
  const int nfull = g.S / 64;
  for (int t = 0; t < nfull; ++t) tile(t, std::false_type{});
  if (nfull < ntiles) tile(nfull, std::true_type{});

  if (q_valid) {
    const float fq = g.scale * dequant(ak) * (1.0f / 256.0f);           // K8 = K 448 / ak, the block holds 256 dS
    bf16_raw* dqp = g.dQ + (bhS + q0 + r) * HD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const int d = dt * 32 + 8 * i4 + 4 * h;
        *reinterpret_cast<uint2*>(dqp + d) = make_uint2(pack_bf16(dq[dt][4 * i4] * fq, dq[dt][4 * i4 + 1] * fq),
                                                        pack_bf16(dq[dt][4 * i4 + 2] * fq, dq[dt][4 * i4 + 3] * fq));
      }
  }
}

// Workspace sections, in this order: Q8, K8, V8, dO8 [B,H,S,128] (each rounded up to 256 bytes), Q8t, K8t, dO8t [B,H,128,Sp].
inline long rows_bytes(int B, int H, int S) { return ((long)B * H * S * HD + 255) / 256 * 256; }
inline long t_bytes(int B, int H, int Sp) { return (long)B * H * HD * Sp; }

}  // namespace

extern "C" long mgx_attn_bwd_fp8_workspace(int B, int H, int S, int Sp) {
  if (B <= 0 || H <= 0 || S <= 0 || Sp < S || Sp % 64 != 0) return -1;
  return 4 * rows_bytes(B, H, S) + 3 * t_bytes(B, H, Sp);
}

extern "C" int mgx_attn_bwd_fp8(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* Qt, const uint16_t* Kt,
                                const uint16_t* O, const uint16_t* dO, const float* lse, float* delta, uint16_t* dOt,
                                uint16_t* dQ, uint16_t* dK, uint16_t* dV, uint8_t* ws, float* amax, int B, int H, int S, int Sp,
                                long ldo, long o_bstride, float scale, long ws_bytes, void* stream) {
  MGX_REQUIRE(Q && K && V && Qt && Kt && O && dO && lse && delta && dOt && dQ && dK && dV && ws && amax, "null operand");
  MGX_REQUIRE(B > 0 && H > 0 && S > 0 && Sp >= S && Sp % 64 == 0, "bad sizes");
  MGX_REQUIRE(ldo % 8 == 0 && o_bstride % 8 == 0, "dO rows must be 16-byte aligned");
  MGX_REQUIRE(ldo >= (long)H * HD && o_bstride >= (long)(S - 1) * ldo + (long)H * HD, "dO strides do not hold the heads");
  MGX_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0 && ws_bytes >= mgx_attn_bwd_fp8_workspace(B, H, S, Sp),
              "workspace: 16-byte aligned, mgx_attn_bwd_fp8_workspace bytes");
  MGX_REQUIRE(scale >= 0.f, "the forward's score factor needs a non-negative scale");
  hipStream_t st = (hipStream_t)stream;
  const long rb = rows_bytes(B, H, S), tb = t_bytes(B, H, Sp);
  BwdF8Args g;
  uint8_t* Q8 = ws; uint8_t* K8 = ws + rb; uint8_t* V8 = ws + 2 * rb; uint8_t* dO8 = ws + 3 * rb;
  uint8_t* Q8t = ws + 4 * rb; uint8_t* K8t = Q8t + tb; uint8_t* dO8t = K8t + tb;
  g.Q8 = Q8; g.K8 = K8; g.V8 = V8; g.dO8 = dO8; g.Q8t = Q8t; g.K8t = K8t; g.dO8t = dO8t;
  g.amax = amax; g.lse = lse; g.delta = delta; g.dQ = dQ; g.dK = dK; g.dV = dV;
  g.B = B; g.H = H; g.S = S; g.Sp = Sp; g.scale = scale; g.scale_log2e = scale * LOG2E;

  mgx_f8::Srcs srcs = {};
  srcs.s[0] = mgx_f8::rows_src(Q, H, S, Q8);
  srcs.s[1] = mgx_f8::rows_src(K, H, S, K8);
  srcs.s[2] = mgx_f8::rows_src(V, H, S, V8);
  srcs.s[3] = {dO, o_bstride, (long)HD, ldo, S, HD, dO8};
  mgx_f8::amax_launch(srcs, 4, amax, B, H, st);
  mgx_f8::quant_rows_launch(srcs, 0, 4, amax, B, H, st);
  mgx_attn_bwd_prep_launch(O, dO, ldo, o_bstride, delta, dOt, B, H, S, Sp, st);
  const long rows = (long)B * H * S;
  fp8_delta_kernel<<<min(cdiv(rows, 4), 16384), 256, 0, st>>>(dO8, O, ldo, o_bstride, amax + 3L * B * H, delta, H, S, rows);
  mgx_f8::TSrcs ts = {};
  ts.s[0] = {Qt, Q8t, 0};
  ts.s[1] = {Kt, K8t, 1};
  ts.s[2] = {dOt, dO8t, 3};
  mgx_f8::quant_t_launch(ts, 3, amax, B * H, S, Sp, st);
  const int nb = cdiv(S, 128) * H * B;
  launch_lds<attn_bwd_fp8_dkv_kernel, 2 * DKV_STAGE>(nb, 256, st, g);
  launch_lds<attn_bwd_fp8_dq_kernel, 2 * DQ_STAGE>(nb, 256, st, g);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
