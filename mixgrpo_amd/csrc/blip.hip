// ImageReward scorer (fastvideo/models/reward_model/image_reward.py:24-40: `RM.load(...)`, `self.model.inference_rank(text,
// [image])` :38): a BLIP ViT image encoder, a BERT text encoder whose every layer cross-attends to the image tokens, and an MLP
// head.  Its Linears run on the GEMM kernels (gemm.hip), LayerNorm / GELU / embeddings on clip.hip and text.hip, both
// attentions on encoder_attn.hip (mgx_vit_attn_fwd, mgx_xattn_fwd); this file holds the one thing those cannot do.  Inference
// only.
//   mgx_linear_rows_f32   fp32 Linear of a few rows, for the score head
#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

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
