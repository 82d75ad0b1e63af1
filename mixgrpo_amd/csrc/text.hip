// Text encoders (the CLIP text tower of the reward networks, fastvideo/models/reward_model/{hps_score,pick_score,clip_score}.py,
// and the T5 + CLIP-L prompt encoders of fastvideo/data_preprocess/preprocess_flux_embedding.py): what sits around their
// Linears, which all run on the GEMM kernels (gemm.hip), and their attention (mgx_text_attn_fwd, encoder_attn.hip).  Inference only.
//   mgx_rms_norm_affine   T5LayerNorm
//   mgx_gated_act_rows    act(a) * b: T5 v1.1's gated GELU
//   mgx_token_embed       token-embedding gather + position embeddings
#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- RMS norm
// one wave per row, element lane + 64 i on lane (up to 64 per lane: D <= 4096): fp32 sum of squares, one rounding
__global__ void __launch_bounds__(256) rms_norm_affine_kernel(const bf16_raw* x, long ldx, const float* __restrict__ gamma,
                                                              bf16_raw* y, long ldy, long M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int n = D / 64;
  const bf16_raw* xr = x + row * ldx;
  float v[64];
  float qs = 0.f;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    v[i] = i < n ? bf2f(xr[i * 64 + lane]) : 0.f;
    qs += v[i] * v[i];
  }
  const float rstd = 1.f / sqrtf(wave_sum(qs) / (float)D + eps);
  bf16_raw* yr = y + row * ldy;
#pragma unroll
  for (int i = 0; i < 64; ++i)
    if (i < n) {
      const int col = i * 64 + lane;
      yr[col] = f2bf(v[i] * rstd * gamma[col]);
    }
}

// ------------------------------------------------------------------------------------------------------------ activations
// act 0 / 1 as act_rows_kernel (clip.hip).  act 2, the tanh GELU, with u = sqrt(2 / pi) (x + 0.044715 x^3) and e = exp(-2 |u|):
// 0.5 (1 + tanh u) is exactly 1 / (1 + e) for u >= 0 and e / (1 + e) for u < 0.  Neither form cancels where 1 + tanh u does
// (x < 0), and e only ever underflows, gradually: the results down to bf16's smallest subnormal keep their precision, where
// exp(+2 |u|) would overflow to inf (a zero result) from 2 |u| = 88.7 on.
__device__ __forceinline__ float act_value(float v, int act) {
  if (act == 0) return 0.5f * v * erfcf(-v * 0.70710678118654752f);
  if (act == 1) return v / (1.f + expf(-1.702f * v));
  const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
  const float e = expf(-2.f * fabsf(u));
  return u >= 0.f ? v / (1.f + e) : v * e / (1.f + e);
}

__global__ void __launch_bounds__(256) gated_act_rows_kernel(const bf16_raw* a, long lda, const bf16_raw* __restrict__ b, long ldb,
                                                             bf16_raw* y, long ldy, long M, int N, int act) {
  const long total = M * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / N;
    const int col = (int)(i - r * N);
    y[r * ldy + col] = f2bf(act_value(bf2f(a[r * lda + col]), act) * bf2f(b[r * ldb + col]));
  }
}

// ---------------------------------------------------------------------------------------------------------------- embed
// An id outside [0, V) breaks the contract (the Python wrapper refuses it on the host); the kernel then reads row 0, never
// memory outside the table.
__global__ void __launch_bounds__(256) token_embed_kernel(const int* __restrict__ ids, const bf16_raw* __restrict__ table,
                                                          const float* __restrict__ pos, bf16_raw* __restrict__ x, long M, int S,
                                                          int D, int V) {
  const long total = M * D;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / D;
    const int col = (int)(i - r * D);
    int id = ids[r];
    if ((unsigned)id >= (unsigned)V) id = 0;
    float v = bf2f(table[(long)id * D + col]);
    if (pos) v += pos[(r % S) * D + col];
    x[i] = f2bf(v);
  }
}

inline int ew_grid(long total) { return (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

}  // namespace

extern "C" int mgx_rms_norm_affine(const uint16_t* x, long ldx, const float* gamma, uint16_t* y, long ldy, long M, int D, float eps,
                                   void* stream) {
  MGX_REQUIRE(x && gamma && y && M > 0, "bad argument");
  MGX_REQUIRE(D > 0 && D % 64 == 0 && D <= 4096 && ldx >= D && ldy >= D, "D % 64 == 0, D <= 4096");
  MGX_REQUIRE((M + 3) / 4 < (1L << 31), "too many rows");
  rms_norm_affine_kernel<<<(int)((M + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, ldx, gamma, y, ldy, M, D, eps);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_gated_act_rows(const uint16_t* a, long lda, const uint16_t* b, long ldb, uint16_t* y, long ldy, long M, int N,
                                  int act, void* stream) {
  MGX_REQUIRE(a && b && y && M > 0 && N > 0 && lda >= N && ldb >= N && ldy >= N && act >= 0 && act <= 2, "bad argument");
  gated_act_rows_kernel<<<ew_grid(M * N), 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, y, ldy, M, N, act);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_token_embed(const int* ids, const uint16_t* table, const float* pos, uint16_t* x, long M, int S, int D, int V,
                               void* stream) {
  MGX_REQUIRE(ids && table && x && M > 0 && S > 0 && D > 0 && V > 0, "bad argument");
  token_embed_kernel<<<ew_grid(M * D), 256, 0, (hipStream_t)stream>>>(ids, table, pos, x, M, S, D, V);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
