// FLUX VAE decoder (diffusers AutoencoderKL, decoder half) -- the memory-bound kernels around the convolutions.
// The convolutions and the mid-block attention's projections / products run on the GEMM kernels (gemm.hip:
// mgx_conv3x3_nhwc, mgx_gemm); this file holds what sits between them.  Activations are NHWC bf16: "plain" = [H W][C]
// row-major, "padded" = [(H + 2)(W + 2)][C] with a zero border (the convolution's padding; only interiors are ever written).
//
// What it replaces: `vae.decode(latents)` of fastvideo/train_grpo_flux.py:279-289 (bf16 weights under bf16 autocast):
// GroupNorm(32 groups, eps 1e-6) runs in fp32 on the bf16 tensor and its fp32 result goes through SiLU in fp32 before the
// next convolution's input cast to bf16 -- one rounding, here at the store; nearest-neighbour upsampling is exact.
// The encoder half (`vae.encode`) adds the plain-to-padded copy in front of its stride-2 downsampler (mgx_conv3x3s2_nhwc) and
// the DiagonalGaussianDistribution of fastvideo/models/hunyuan/vae/vae.py:321-353,384 behind conv_out.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- GroupNorm statistics
// stage 1: per-channel sum / sum of squares of a slab of rows; stage 2: groups, in double.
// The variance is E[x^2] - mean^2, so for a group whose mean is large against its spread (mean 12, std 1/4: mean^2 / var =
// 2304) a relative error e of the sums is an error of 1152 e of rstd: they must be exact to fp32's last bit.  A thread
// therefore adds GN_CHAIN rows in fp32 -- bf16 values have 8 significant bits and their squares 16, so 64 squares of values
// of one binade (two binades of squares) add exactly in fp32's 24 -- and folds each chain into fp64, in which everything
// after it runs.  (One fp32 chain over the slab, 512 rows at C = 2048, and the fp32 sum over the 256 rows of a pass at C = 8
// lost the last bits of the squares' sum: tests/test_hip_vae_kernels.py.)  64 and not fewer: every chain's end exposes one
// load latency, which at C = 512 (128 rows per thread) was measured as 3 us of a 57 us launch with chains of 16.
constexpr int GN_ROWS = 512;   // rows per stage-1 block
constexpr int GN_CHAIN = 64;   // rows a thread adds in fp32 before it folds the sums into fp64

__global__ void __launch_bounds__(256) gn_partial_kernel(const bf16_raw* __restrict__ x, long ld, long M, int C,
                                                         double* __restrict__ part) {
  const int tpr = C / 8;                          // threads per row (8 channels = 16 bytes each)
  const int rpp = 256 / tpr;                      // rows per pass
  const int cx = threadIdx.x % tpr, ry = threadIdx.x / tpr;
  const long r0 = (long)blockIdx.x * GN_ROWS;
  const long r1 = r0 + GN_ROWS < M ? r0 + GN_ROWS : M;
  double sd[8], qd[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sd[e] = qd[e] = 0.0;
  if (ry < rpp)
    for (long rb = r0 + ry; rb < r1; rb += (long)GN_CHAIN * rpp) {
      const long re = rb + (long)GN_CHAIN * rpp < r1 ? rb + (long)GN_CHAIN * rpp : r1;
      float s[8], q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
      for (long r = rb; r < re; r += rpp) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + r * ld + cx * 8);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = bf2f(w[e] & 0xffff), b = bf2f(w[e] >> 16);
          s[2 * e] += a; q[2 * e] += a * a;
          s[2 * e + 1] += b; q[2 * e + 1] += b * b;
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { sd[e] += (double)s[e]; qd[e] += (double)q[e]; }
    }
  // rows of the block -> one value per channel (LDS: [ry][C] x 2, doubles.  One array used twice, to stay at the 16 KiB of the
  // fp32 arrays, was measured slower: 59.9 against 58.5 us at 128 x 128 x 512)
  extern __shared__ double sh[];
  double* ss = sh;
  double* qq = sh + (size_t)rpp * C;
  if (ry < rpp) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ss[ry * C + cx * 8 + e] = sd[e];
      qq[ry * C + cx * 8 + e] = qd[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double a = 0.0, b = 0.0;
    for (int r = 0; r < rpp; ++r) {
      a += ss[r * C + c];
      b += qq[r * C + c];
    }
    part[((long)blockIdx.x * 2 + 0) * C + c] = a;
    part[((long)blockIdx.x * 2 + 1) * C + c] = b;
  }
}

// stats[g] = (mean, rstd) of group g; one block per group
__global__ void __launch_bounds__(256) gn_finish_kernel(const double* __restrict__ part, float* __restrict__ stats, int nblk,
                                                        int C, int G, long M, float eps) {
  __shared__ double rs[4], rq[4];
  const int g = blockIdx.x, cpg = C / G;
  double s = 0.0, q = 0.0;
  for (long i = threadIdx.x; i < (long)nblk * cpg; i += 256) {
    const long b = i / cpg;
    const int c = g * cpg + (int)(i - b * cpg);
    s += part[(b * 2 + 0) * C + c];
    q += part[(b * 2 + 1) * C + c];
  }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { rs[w] = s; rq[w] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)M * cpg;
    const double mean = (rs[0] + rs[1] + rs[2] + rs[3]) / n;
    double var = (rq[0] + rq[1] + rq[2] + rq[3]) / n - mean * mean;   // biased, like torch.nn.functional.group_norm
    if (var < 0.0) var = 0.0;
    stats[2 * g] = (float)mean;
    stats[2 * g + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + __expf(-v)); }

// y = [silu]((x - mean) rstd w + b) -> bf16.  Output pixel (yy, xx) goes to out + (yy * out_row + xx) * out_px: a plain
// matrix (out_row = W * C, out_px = C) or the interior of a padded image (out_row = (W + 2) C, out pointing at pixel (1, 1)).
__global__ void __launch_bounds__(256) gn_apply_kernel(const bf16_raw* __restrict__ x, long ld, const float* __restrict__ stats,
                                                       const bf16_raw* __restrict__ gamma, const bf16_raw* __restrict__ beta,
                                                       bf16_raw* __restrict__ out, long out_row, long out_px, long M, int Wd,
                                                       int C, int G, int silu) {
  const int tpr = C / 8, cpg = C / G;
  const long total = M * tpr;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const long r = id / tpr;
    const int c0 = (int)(id - r * tpr) * 8;
    const uint4 u = *reinterpret_cast<const uint4*>(x + r * ld + c0);
    const uint4 gw = *reinterpret_cast<const uint4*>(gamma + c0), gb = *reinterpret_cast<const uint4*>(beta + c0);
    const uint32_t xw[4] = {u.x, u.y, u.z, u.w}, ww[4] = {gw.x, gw.y, gw.z, gw.w}, bw[4] = {gb.x, gb.y, gb.z, gb.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = c0 + 2 * e + h;
        const int g = c / cpg;
        const float xv = bf2f(h ? xw[e] >> 16 : xw[e] & 0xffff);
        const float wv = bf2f(h ? ww[e] >> 16 : ww[e] & 0xffff), bv = bf2f(h ? bw[e] >> 16 : bw[e] & 0xffff);
        float t = (xv - stats[2 * g]) * stats[2 * g + 1] * wv + bv;
        v[h] = silu ? silu_f(t) : t;
      }
      o[e] = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    }
    const long yy = r / Wd, xx = r - yy * Wd;
    *reinterpret_cast<uint4*>(out + yy * out_row + xx * out_px + c0) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// nearest-neighbour 2x: plain [H W][C] -> interior of a padded [(2H + 2)(2W + 2)][C] image (out points at pixel (1, 1))
__global__ void __launch_bounds__(256) upsample2x_pad_kernel(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ out, int H,
                                                             int Wd, int C) {
  const int tpr = C / 8;
  const long total = (long)4 * H * Wd * tpr;
  const long orow = (long)(2 * Wd + 2) * C;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const long p = id / tpr;
    const int c0 = (int)(id - p * tpr) * 8;
    const long oy = p / (2 * Wd), ox = p - oy * (2 * Wd);
    const uint4 u = *reinterpret_cast<const uint4*>(x + ((oy >> 1) * Wd + (ox >> 1)) * C + c0);
    *reinterpret_cast<uint4*>(out + oy * orow + ox * C + c0) = u;
  }
}

// plain [H W][ld] (first C channels) -> interior of a padded [(H + 2)(W + 2)][C] image (out points at pixel (1, 1))
__global__ void __launch_bounds__(256) pad_kernel(const bf16_raw* __restrict__ x, long ld, bf16_raw* __restrict__ out, int H,
                                                  int Wd, int C) {
  const int tpr = C / 8;
  const long total = (long)H * Wd * tpr;
  const long orow = (long)(Wd + 2) * C;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const long p = id / tpr;
    const int c0 = (int)(id - p * tpr) * 8;
    const long yy = p / Wd, xx = p - yy * Wd;
    *reinterpret_cast<uint4*>(out + yy * orow + xx * C + c0) = *reinterpret_cast<const uint4*>(x + p * ld + c0);
  }
}

// DiagonalGaussianDistribution on bf16 tensors: every torch op rounds its result to bf16.  moments plain [HW][ld]: channels
// [0, Cz) the mean, [Cz, 2 Cz) the logvar -> mean, std, sample [Cz][HW]
__global__ void __launch_bounds__(256) diag_gaussian_kernel(const bf16_raw* __restrict__ mom, long ld,
                                                            const bf16_raw* __restrict__ noise, bf16_raw* __restrict__ mean,
                                                            bf16_raw* __restrict__ stdv, bf16_raw* __restrict__ sample, int Cz,
                                                            long HW) {
  const long total = HW * Cz;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const int c = (int)(id / HW);
    const long p = id - (long)c * HW;
    const bf16_raw m = mom[p * ld + c];
    float lv = bf2f(mom[p * ld + Cz + c]);
    lv = lv < -30.0f ? -30.0f : (lv > 20.0f ? 20.0f : lv);                        // torch.clamp: exact in bf16, NaN stays NaN
    const bf16_raw s = f2bf(expf(bf2f(f2bf(0.5f * lv))));
    mean[id] = m;
    stdv[id] = s;
    sample[id] = noise ? f2bf(bf2f(m) + bf2f(f2bf(bf2f(s) * bf2f(noise[id])))) : m;
  }
}

// latents [Cin][H][W] fp32 -> bf16 interior of a padded NHWC image with C channels (channels >= Cin stay zero)
__global__ void __launch_bounds__(256) nchw_to_pad_kernel(const float* __restrict__ z, bf16_raw* __restrict__ out, int Cin, int H,
                                                          int Wd, int C) {
  const long total = (long)H * Wd * Cin;
  const long orow = (long)(Wd + 2) * C;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const int c = (int)(id % Cin);
    const long p = id / Cin;
    const long yy = p / Wd, xx = p - yy * Wd;
    out[yy * orow + xx * C + c] = f2bf(z[((long)c * H + yy) * Wd + xx]);
  }
}

// [H W][ld] bf16 (first Cout channels) -> image [Cout][H][W] bf16
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const bf16_raw* __restrict__ x, long ld, bf16_raw* __restrict__ img,
                                                           int Cout, long HW) {
  const long total = HW * Cout;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const int c = (int)(id / HW);
    const long p = id - (long)c * HW;
    img[id] = x[p * ld + c];
  }
}

// P[r, :] = bf16(softmax(scale * S[r, :])), S fp32 [M][ld]; one block per row, the row held in registers (n <= 256 * 64)
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* __restrict__ S, long lds_, bf16_raw* __restrict__ P,
                                                           long ldp, int n, float scale) {
  __shared__ float red[4];
  const float* row = S + (long)blockIdx.x * lds_;
  float v[64];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int c = i * 256 + threadIdx.x;
    v[i] = c < n ? row[c] * scale : -INFINITY;
    mx = fmaxf(mx, v[i]);
  }
  mx = wave_max(mx);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    v[i] = __expf(v[i] - mx);                      // exp(-inf) = 0 beyond the row
    sum += v[i];
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[w] = sum;
  __syncthreads();
  const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
  bf16_raw* prow = P + (long)blockIdx.x * ldp;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int c = i * 256 + threadIdx.x;
    if (c < n) prow[c] = f2bf(v[i] * inv);
  }
}

}  // namespace

// (fp32 elements: the stage-1 sums are doubles, two elements each, in front of the 2 G statistics)
extern "C" long mgx_group_norm_workspace(long M, int C, int G) { return (long)cdiv(M, GN_ROWS) * 4 * C + 2L * G; }

// y = [silu](GroupNorm(x)) for one image: x plain [M = H W][C] bf16 (leading dimension ld), G groups, affine gamma / beta [C]
// bf16; out: see gn_apply_kernel.  ws: fp32 scratch of mgx_group_norm_workspace(M, C, G) elements, 8-byte aligned.
extern "C" int mgx_group_norm_nhwc(const uint16_t* x, long ld, const uint16_t* gamma, const uint16_t* beta, uint16_t* out,
                                   long out_row, long out_px, float* ws, int H, int Wd, int C, int G, float eps, int silu,
                                   void* stream) {
  MGX_REQUIRE(x && gamma && beta && out && ws && H > 0 && Wd > 0, "bad argument");
  MGX_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0 && G > 0 && C % G == 0, "channels must be 8 .. 2048, a power of two times 8");
  MGX_REQUIRE(ld % 8 == 0 && out_row % 8 == 0 && out_px % 8 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0) &&
                  ((uintptr_t)gamma % 16 == 0) && ((uintptr_t)beta % 16 == 0), "16-byte addressable rows");
  MGX_REQUIRE((uintptr_t)ws % 8 == 0, "the workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)H * Wd;
  const int nblk = cdiv(M, GN_ROWS);
  double* part = reinterpret_cast<double*>(ws);
  float* stats = ws + (long)nblk * 4 * C;
  const int rpp = 256 / (C / 8);
  gn_partial_kernel<<<nblk, 256, (size_t)2 * rpp * C * sizeof(double), st>>>(x, ld, M, C, part);
  gn_finish_kernel<<<G, 256, 0, st>>>(part, stats, nblk, C, G, M, eps);
  const long total = M * (C / 8);
  const int grid = (int)((total + 255) / 256 < 256L * 16 ? (total + 255) / 256 : 256L * 16);
  gn_apply_kernel<<<grid, 256, 0, st>>>(x, ld, stats, gamma, beta, out, out_row, out_px, M, Wd, C, G, silu);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_upsample2x_pad_nhwc(const uint16_t* x, uint16_t* out, int H, int Wd, int C, void* stream) {
  MGX_REQUIRE(x && out && H > 0 && Wd > 0 && C % 8 == 0, "bad argument");
  MGX_REQUIRE(((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0), "16-byte aligned images");
  const long total = (long)4 * H * Wd * (C / 8);
  const int grid = (int)((total + 255) / 256 < 256L * 16 ? (total + 255) / 256 : 256L * 16);
  upsample2x_pad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, out, H, Wd, C);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_pad_nhwc(const uint16_t* x, long ld, uint16_t* out, int H, int Wd, int C, void* stream) {
  MGX_REQUIRE(x && out && H > 0 && Wd > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 8 == 0, "bad argument");
  MGX_REQUIRE(((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0), "16-byte aligned images");
  const long total = (long)H * Wd * (C / 8);
  const int grid = (int)((total + 255) / 256 < 256L * 16 ? (total + 255) / 256 : 256L * 16);
  pad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, ld, out, H, Wd, C);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_diag_gaussian_nhwc(const uint16_t* moments, long ld, const uint16_t* noise, uint16_t* mean, uint16_t* std,
                                      uint16_t* sample, int Cz, int H, int Wd, void* stream) {
  MGX_REQUIRE(moments && mean && std && sample && Cz > 0 && ld >= 2L * Cz && H > 0 && Wd > 0, "bad argument");
  const long total = (long)H * Wd * Cz;
  const int grid = (int)((total + 255) / 256 < 256L * 16 ? (total + 255) / 256 : 256L * 16);
  diag_gaussian_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(moments, ld, noise, mean, std, sample, Cz, (long)H * Wd);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_latents_to_pad_nhwc(const float* z, uint16_t* out, int Cin, int H, int Wd, int C, void* stream) {
  MGX_REQUIRE(z && out && Cin > 0 && Cin <= C && H > 0 && Wd > 0, "bad argument");
  const long total = (long)H * Wd * Cin;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  nchw_to_pad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(z, out, Cin, H, Wd, C);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_nhwc_to_image(const uint16_t* x, long ld, uint16_t* img, int Cout, int H, int Wd, void* stream) {
  MGX_REQUIRE(x && img && Cout > 0 && ld >= Cout && H > 0 && Wd > 0, "bad argument");
  const long total = (long)H * Wd * Cout;
  const int grid = (int)((total + 255) / 256 < 256L * 16 ? (total + 255) / 256 : 256L * 16);
  nhwc_to_nchw_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, ld, img, Cout, (long)H * Wd);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int mgx_softmax_rows_f32(const float* S, long lds_, uint16_t* P, long ldp, int M, int n, float scale, void* stream) {
  MGX_REQUIRE(S && P && M > 0 && n > 0 && n <= 256 * 64 && lds_ >= n && ldp >= n, "row length must be <= 16384");
  softmax_rows_kernel<<<M, 256, 0, (hipStream_t)stream>>>(S, lds_, P, ldp, n, scale);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
