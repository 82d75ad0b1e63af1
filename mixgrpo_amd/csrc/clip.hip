// CLIP ViT image tower (the reward networks of fastvideo/models/reward_model/{hps_score,pick_score,clip_score}.py): what sits
// around the tower's Linears, which all run on the GEMM kernels (gemm.hip), and its attention (mgx_vit_attn_fwd,
// encoder_attn.hip).  The tower is inference only.
//   mgx_clip_preprocess    decoded image -> normalised patch rows (the PIL resize + crop + normalise of the reference's processors)
//   mgx_vit_embed          class token + patch embeddings + position embeddings
//   mgx_layer_norm_affine  nn.LayerNorm with weight and bias
//   mgx_act_rows           exact GELU / QuickGELU
//   mgx_l2_normalize_rows, mgx_cosine_score   the scores' tail
#include "../../include/mixgrpo_hip.h"
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- LayerNorm
// one wave per row, element lane + 64 i on lane: fp32 mean, then the centred sum of squares (two passes over registers)
__global__ void __launch_bounds__(256) layer_norm_affine_kernel(const bf16_raw* x, long ldx, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, bf16_raw* y, long ldy, long M,
                                                                int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int n = D / 64;
  const bf16_raw* xr = x + row * ldx;
  float v[32];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    v[i] = i < n ? bf2f(xr[i * 64 + lane]) : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float qs = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const float dv = i < n ? v[i] - mean : 0.f;
    qs += dv * dv;
  }
  const float rstd = 1.f / sqrtf(wave_sum(qs) / (float)D + eps);
  bf16_raw* yr = y + row * ldy;
#pragma unroll
  for (int i = 0; i < 32; ++i)
    if (i < n) {
      const int col = i * 64 + lane;
      yr[col] = f2bf((v[i] - mean) * rstd * gamma[col] + beta[col]);
    }
}

// ------------------------------------------------------------------------------------------------------------ activations
// exact GELU as x/2 erfc(-x / sqrt 2): 1 + erf(x / sqrt 2) cancels for x < 0 and loses the result's relative precision
__global__ void __launch_bounds__(256) act_rows_kernel(const bf16_raw* x, long ldx, bf16_raw* y, long ldy, long M, int N, int act) {
  const long total = M * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / N;
    const int col = (int)(i - r * N);
    const float v = bf2f(x[r * ldx + col]);
    float o;
    if (act == 0)
      o = 0.5f * v * erfcf(-v * 0.70710678118654752f);
    else
      o = v / (1.f + expf(-1.702f * v));
    y[r * ldy + col] = f2bf(o);
  }
}

// ---------------------------------------------------------------------------------------------------------------- embed
__global__ void __launch_bounds__(256) vit_embed_kernel(const bf16_raw* __restrict__ patch_out, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, bf16_raw* __restrict__ x, long rows,
                                                        int S, int width) {
  const long total = rows * width;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / width;
    const int col = (int)(i - r * width);
    const long b = r / S;
    const int s = (int)(r - b * S);
    const float a = s == 0 ? cls[col] : bf2f(patch_out[(b * (S - 1) + s - 1) * width + col]);
    x[i] = f2bf(a + pos[(long)s * width + col]);
  }
}

// ----------------------------------------------------------------------------------------------------------- preprocess
// VaeImageProcessor.postprocess under bf16 (denormalise and clamp in bf16), then x 255 in fp32 and round half to even
__device__ __forceinline__ float image_level(bf16_raw raw) {
  float t = rbf(bf2f(raw) * 0.5f);
  t = rbf(t + 0.5f);
  t = fminf(fmaxf(t, 0.f), 1.f);
  return rintf(t * 255.f);
}

// Keys cubic, a = -1/2 (PIL's BICUBIC)
__device__ __forceinline__ double cubic_weight(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// PIL's precompute_coeffs for output index i: taps [k0, k1), the centre and 1 / max(scale, 1).  The weights themselves are
// evaluated in double where they are used: in fp32 the centre (i + 1/2) scale of a 1024-pixel side is uncertain by 6e-5 pixels,
// which moves a noisy image's result by several thousandths of a level.
struct Taps {
  int k0, k1;
  double center, ss;
};
__device__ __forceinline__ Taps resize_taps(int i, int in, int out) {
  const double scale = (double)in / (double)out;
  const double fs = scale > 1.0 ? scale : 1.0;
  const double support = 2.0 * fs;
  Taps t;
  t.center = (i + 0.5) * scale;
  t.ss = 1.0 / fs;
  t.k0 = (int)(t.center - support + 0.5);
  if (t.k0 < 0) t.k0 = 0;
  t.k1 = (int)(t.center + support + 0.5);
  if (t.k1 > in) t.k1 = in;
  return t;
}

// horizontal pass over the columns the crop keeps: tmp[c][y][j] = resize of row y at output column left + j
__global__ void __launch_bounds__(256) clip_hpass_kernel(const bf16_raw* __restrict__ img, float* __restrict__ tmp, int H, int W,
                                                         int ow, int left, int R) {
  const long total = 3L * H * R;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int j = (int)(i % R);
    const long cy = i / R;                                    // c * H + y
    const Taps t = resize_taps(left + j, W, ow);
    const bf16_raw* row = img + cy * W;
    double ww = 0.0, a = 0.0;
    for (int k = t.k0; k < t.k1; ++k) {
      const double w = cubic_weight((k - t.center + 0.5) * t.ss);
      ww += w;
      a += w * (double)image_level(row[k]);
    }
    tmp[i] = (float)(a / ww);
  }
}

// vertical pass, rounding to levels, normalisation and the patch layout
__global__ void __launch_bounds__(256) clip_vpass_kernel(const float* __restrict__ tmp, bf16_raw* __restrict__ patches,
                                                         uint8_t* __restrict__ levels, int H, int oh, int top, int R, int p, int Kp,
                                                         float m0, float m1, float m2, float s0, float s1, float s2) {
  const int np = R / p;
  const long total = (long)np * np * Kp;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int col = (int)(i % Kp);
    const int prow = (int)(i / Kp);
    if (col >= 3 * p * p) {
      patches[i] = 0;
      continue;
    }
    const int c = col / (p * p), dy = (col / p) % p, dx = col % p;
    const int y = (prow / np) * p + dy, x = (prow % np) * p + dx;
    const Taps t = resize_taps(top + y, H, oh);
    const float* colp = tmp + (long)c * H * R + x;
    double ww = 0.0, a = 0.0;
    for (int k = t.k0; k < t.k1; ++k) {
      const double w = cubic_weight((k - t.center + 0.5) * t.ss);
      ww += w;
      a += w * (double)colp[(long)k * R];
    }
    float lv = rintf((float)(a / ww));
    lv = fminf(fmaxf(lv, 0.f), 255.f);
    if (levels) levels[((long)c * R + y) * R + x] = (uint8_t)lv;
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    patches[i] = f2bf((lv / 255.f - mean) / sd);
  }
}

// ---------------------------------------------------------------------------------------------------------- score tail
template <typename T>
__device__ __forceinline__ float ldf(const T* p, long i);
template <>
__device__ __forceinline__ float ldf<float>(const float* p, long i) { return p[i]; }
template <>
__device__ __forceinline__ float ldf<bf16_raw>(const bf16_raw* p, long i) { return bf2f(p[i]); }

// sums over a 256-thread block, the result on every thread
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

template <typename TF, typename TT>
__global__ void __launch_bounds__(256) cosine_score_kernel(const TF* __restrict__ f, long ldf_, const TT* __restrict__ t, long ldt,
                                                           float* __restrict__ out, int n, float logit_scale, float mean, float std) {
  __shared__ float sh[4];
  const long b = blockIdx.x;
  float dot = 0.f, ff = 0.f, tt = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = ldf<TF>(f, b * ldf_ + i), c = ldf<TT>(t, b * ldt + i);
    dot += a * c;
    ff += a * a;
    tt += c * c;
  }
  dot = block_sum(dot, sh);
  ff = block_sum(ff, sh);
  tt = block_sum(tt, sh);
  if (threadIdx.x == 0) out[b] = (logit_scale * (dot / (sqrtf(ff) * sqrtf(tt))) - mean) / std;
}

__global__ void __launch_bounds__(256) l2_normalize_kernel(const bf16_raw* __restrict__ f, long ldf_, float* __restrict__ out, int n) {
  __shared__ float sh[4];
  const long b = blockIdx.x;
  float ff = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = bf2f(f[b * ldf_ + i]);
    ff += a * a;
  }
  const float nrm = sqrtf(block_sum(ff, sh));
  for (int i = threadIdx.x; i < n; i += 256) out[b * n + i] = bf2f(f[b * ldf_ + i]) / nrm;
}

inline int ew_grid(long total) { return (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

// output side of the resize of an H x W image whose shortest edge becomes R (the long side truncated, as
// transformers' get_resize_output_image_size and torchvision's Resize do)
inline void resized_hw(int H, int W, int R, int* oh, int* ow) {
  if (H <= W) {
    *oh = R;
    *ow = (int)((long)R * W / H);
  } else {
    *ow = R;
    *oh = (int)((long)R * H / W);
  }
}

}  // namespace

extern "C" int mgx_layer_norm_affine(const uint16_t* x, long ldx, const float* gamma, const float* beta, uint16_t* y, long ldy,
                                     long M, int D, float eps, void* stream) {
  MGX_REQUIRE(x && gamma && beta && y && M > 0, "bad argument");
  MGX_REQUIRE(D > 0 && D % 64 == 0 && D <= 2048 && ldx >= D && ldy >= D, "D % 64 == 0, D <= 2048");
  MGX_REQUIRE((M + 3) / 4 < (1L << 31), "too many rows");
  layer_norm_affine_kernel<<<(int)((M + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, ldx, gamma, beta, y, ldy, M, D, eps);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_act_rows(const uint16_t* x, long ldx, uint16_t* y, long ldy, long M, int N, int act, void* stream) {
  MGX_REQUIRE(x && y && M > 0 && N > 0 && ldx >= N && ldy >= N && (act == 0 || act == 1), "bad argument");
  act_rows_kernel<<<ew_grid(M * N), 256, 0, (hipStream_t)stream>>>(x, ldx, y, ldy, M, N, act);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_vit_embed(const uint16_t* patch_out, const float* cls, const float* pos, uint16_t* x, int B, int S, int width,
                             void* stream) {
  MGX_REQUIRE(patch_out && cls && pos && x && B > 0 && S >= 2 && width > 0, "bad argument");
  vit_embed_kernel<<<ew_grid((long)B * S * width), 256, 0, (hipStream_t)stream>>>(patch_out, cls, pos, x, (long)B * S, S, width);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" long mgx_clip_preprocess_workspace(int H, int W, int R) {
  if (H < 1 || W < 1 || R < 1) return -1;
  return 3L * H * R;
}

extern "C" int mgx_clip_preprocess(const uint16_t* image, int H, int W, int R, int p, const float* mean, const float* std,
                                   uint16_t* patches, int Kp, uint8_t* levels, float* workspace, long workspace_elems,
                                   void* stream) {
  MGX_REQUIRE(image && mean && std && patches && workspace && H >= 1 && W >= 1, "bad argument");
  MGX_REQUIRE(R >= 1 && p >= 1 && R % p == 0 && Kp >= 3 * p * p, "R % patch == 0, Kp >= 3 patch^2");
  MGX_REQUIRE(workspace_elems >= 3L * H * R, "workspace smaller than mgx_clip_preprocess_workspace");
  for (int c = 0; c < 3; ++c) MGX_REQUIRE(std[c] > 0.f, "std must be positive");
  int oh, ow;
  resized_hw(H, W, R, &oh, &ow);
  const int top = (oh - R) / 2, left = (ow - R) / 2;
  hipStream_t st = (hipStream_t)stream;
  clip_hpass_kernel<<<ew_grid(3L * H * R), 256, 0, st>>>(image, workspace, H, W, ow, left, R);
  MGX_CHECK_LAUNCH();
  clip_vpass_kernel<<<ew_grid((long)(R / p) * (R / p) * Kp), 256, 0, st>>>(workspace, patches, levels, H, oh, top, R, p, Kp, mean[0],
                                                                            mean[1], mean[2], std[0], std[1], std[2]);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_cosine_score(const void* f, int f_is_f32, long ldf_, const void* t, int t_is_f32, long ldt, float* out, int B,
                                int n, float logit_scale, float mean, float std, void* stream) {
  MGX_REQUIRE(f && t && out && B > 0 && n > 0 && ldf_ >= n && (ldt >= n || ldt == 0) && std != 0.f, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (f_is_f32 && t_is_f32)
    cosine_score_kernel<float, float><<<B, 256, 0, st>>>((const float*)f, ldf_, (const float*)t, ldt, out, n, logit_scale, mean, std);
  else if (f_is_f32)
    cosine_score_kernel<float, bf16_raw><<<B, 256, 0, st>>>((const float*)f, ldf_, (const bf16_raw*)t, ldt, out, n, logit_scale, mean, std);
  else if (t_is_f32)
    cosine_score_kernel<bf16_raw, float><<<B, 256, 0, st>>>((const bf16_raw*)f, ldf_, (const float*)t, ldt, out, n, logit_scale, mean, std);
  else
    cosine_score_kernel<bf16_raw, bf16_raw><<<B, 256, 0, st>>>((const bf16_raw*)f, ldf_, (const bf16_raw*)t, ldt, out, n, logit_scale, mean, std);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_l2_normalize_rows(const uint16_t* f, long ldf_, float* out, int B, int n, void* stream) {
  MGX_REQUIRE(f && out && B > 0 && n > 0 && ldf_ >= n, "bad argument");
  l2_normalize_kernel<<<B, 256, 0, (hipStream_t)stream>>>(f, ldf_, out, n);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
