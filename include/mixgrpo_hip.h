/*
 * libmixgrpo_hip.so -- C ABI of the MI355X-native MixGRPO rollout-and-update hot path.
 *
 * The reference (zqqqqz2000/MixGRPO) is pure Python and has no FFI layer; its boundary for this path is
 * the function surface of fastvideo/utils/sampling_utils.py and fastvideo/train_grpo_flux.py, which calls
 * PyTorch eager ops.  Every entry point below replaces the eager-op sequence of one reference function
 * (cited per function, paths relative to the reference root).  The Python mirror in mixgrpo_amd/ binds
 * them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: plain pointers to DEVICE memory unless a parameter says "host"; sizes as int/long; scalars
 * by value; `stream` is a hipStream_t passed as void*.  No allocation, no host sync, no global mutable
 * state except the thread-local last-error string.  Returns 0 (MGX_OK) or a negative error code; the
 * message is available from mgx_last_error().  bf16 tensors are passed as uint16_t*.
 */
#ifndef MIXGRPO_HIP_H
#define MIXGRPO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int mgx_version(void);
const char* mgx_last_error(void);

/* ------------------------------------------------------------------------------------------------ solver
 * Host-computed per-step scalars.  They are produced on the host (mixgrpo_amd/sampling_utils.py) in the
 * reference's own fp32 operation order, including which scalars PyTorch rounds to bf16 before multiplying
 * a bf16 tensor (oracle/solver.py header), so the kernels only apply them.
 */
typedef struct {
  float sigma_x0; /* x0   = x - bf16(v * sigma_x0)                       sampling_utils.py:175 */
  float c_x;      /* mean = x * c_x + bf16(bf16(v * c_v) * dt_mean)      sampling_utils.py:186 */
  float c_v;
  float dt_mean;
  float sd_noise; /* prev = mean + bf16(noise * sd_noise)                sampling_utils.py:195 */
  float dt_det;   /* deterministic: prev = x + bf16(v * dt_det)          sampling_utils.py:199 */
  float den;      /* 2*sd^2                                              sampling_utils.py:202 */
  float log_sd;   /* log(sd)                                             sampling_utils.py:203 */
  float log_c;    /* log(sqrt(2*pi))                                     sampling_utils.py:204 */
} mgx_flow_coeffs;

/* Elements of `ws` (double) the log-prob reduction needs for a [B, n] problem. */
long mgx_logp_workspace_elems(int B, long n);

/* flow_grpo_step forward (sampling_utils.py:157-210).  x fp32 [B,n]; v bf16 [B,n].
 * Rollout: noise bf16 [B,n] given, prev_in NULL -> writes prev_out.  Replay (training, :149-157 of
 * train_grpo_flux.py): prev_in fp32 given, noise NULL, prev_out may be NULL.  deterministic!=0 applies the
 * ODE override (:198-199) after the draw.  x0_out / mean_out are optional (NULL to skip).
 * logp fp32 [B] = mean over n of the Gaussian log-density (:201-208). */
int mgx_flow_step_fwd(const float* x, const uint16_t* v, const uint16_t* noise, const float* prev_in,
                      float* prev_out, float* x0_out, float* mean_out, float* logp, double* ws, int B, long n,
                      const mgx_flow_coeffs* k /*host*/, int deterministic, void* stream);

/* d logp / d v for the replay path (autograd of sampling_utils.py:186,201-208): dv bf16 [B,n],
 * g_logp fp32 [B] is dLoss/dlogp. */
int mgx_flow_step_bwd(const float* x, const uint16_t* v, const float* prev, const float* g_logp, uint16_t* dv,
                      int B, long n, const mgx_flow_coeffs* k /*host*/, void* stream);

/* KL penalty of a replayed Flow-GRPO step to a frozen reference policy (trainer flag --kl_ref_coeff; LoRA runs, where
 * the adapter-free base is the reference).  NOT in the reference trainer, whose --kl_coeff term 0.5 (lp_new - lp_old)^2
 * is taken to the rollout policy of the same step.  v_ref bf16 [B,n] is the reference policy's model output on the
 * same inputs and carries no gradient.  With mean(u) = x * c_x + bf16(bf16(u * c_v) * dt_mean), the mean_out of
 * mgx_flow_step_fwd:
 *   kl[b] = mean over n of (mean(v) - mean(v_ref))^2 / den          (den = 2 sd^2: the closed-form KL of two
 *                                                                    Gaussians of equal sd, averaged like logp)
 * ws as for mgx_flow_step_fwd (mgx_logp_workspace_elems doubles; per-block partials, fixed-order finalize, no
 * atomics).  Streams 8 bytes per element. */
int mgx_flow_kl_fwd(const float* x, const uint16_t* v, const uint16_t* v_ref, float* kl_out, double* ws, int B, long n,
                    const mgx_flow_coeffs* k /*host*/, void* stream);

/* mgx_flow_step_bwd with that term: g_kl fp32 [B] is dLoss/dkl.  Both gradients meet at the fp32 mean, as under
 * autograd, before the bf16 chain to dv:
 *   gm = (g_logp / n / den) * 2 (prev - mean(v)) + (g_kl / n / den) * 2 (mean(v) - mean(v_ref))
 * With g_kl zero or v_ref == v the result is mgx_flow_step_bwd's bit for bit.  14 bytes per element. */
int mgx_flow_step_kl_bwd(const float* x, const uint16_t* v, const uint16_t* v_ref, const float* prev,
                         const float* g_logp, const float* g_kl, uint16_t* dv, int B, long n,
                         const mgx_flow_coeffs* k /*host*/, void* stream);

typedef struct {
  float ds_r;    /* mean0 = x + bf16(v * ds_r)        sampling_utils.py:224 (scalar rounded to bf16) */
  float s_r;      /* x0    = x - bf16(v * s_r)         sampling_utils.py:226 */
  float ds;       /* unrounded sigma_next - sigma (score-correction term :234) */
  float ds_b;     /* scalar autograd uses for d(ds*v)/dv (unrounded on CPU semantics) */
  float s_b;      /* scalar autograd uses for d(s*v)/dv */
  float one_m_s;  /* 1 - sigma                         sampling_utils.py:232 */
  float s_sq;     /* sigma^2 */
  float half_eta2;/* -0.5*eta^2 as fp32                sampling_utils.py:233 */
  float sd;       /* eta*sqrt(sigma - sigma_next) as fp32 :229 */
  float den;      /* 2*sd^2 as fp32                    :245 */
} mgx_dance_coeffs;

/* dance_grpo_step forward with grpo=True (sampling_utils.py:212-253).  noise fp32 [B,n] (SDE rollout) or
 * NULL; prev_in fp32 (replay) or NULL; sde!=0 adds the score correction (:231-234). */
int mgx_dance_step_fwd(const float* x, const uint16_t* v, const float* noise, const float* prev_in,
                       float* prev_out, float* x0_out, float* logp, double* ws, int B, long n,
                       const mgx_dance_coeffs* k /*host*/, int sde, void* stream);
int mgx_dance_step_bwd(const float* x, const uint16_t* v, const float* prev, const float* g_logp, uint16_t* dv,
                       int B, long n, const mgx_dance_coeffs* k /*host*/, int sde, void* stream);

typedef struct {
  int order;        /* 1..3: which multistep update (sampling_utils.py:327-357) */
  int sde;          /* x = mean + sd_noise*noise instead of the ODE combination */
  float sigma_x0;   /* x0 = sample - bf16(v*sigma_x0)            :387-396 */
  float inv_r0;     /* D1_0 = inv_r0*(m0-m1)                     :490,608 */
  float inv_r1;     /* D1_1 = inv_r1*(m1-m2)                     :608 */
  float c_r;        /* D1 = D1_0 + c_r*(D1_0-D1_1)               :609 */
  float inv_r01;    /* D2 = inv_r01*(D1_0-D1_1)                  :610 */
  float cm[4];      /* mean = cm0*sample + cm1*D0 + cm2*D1 + cm3*D2 (signed, summed left to right) */
  float cx[4];      /* x    = cx0*sample + cx1*D0 + cx2*D1 + cx3*D2 */
  float sd_noise;   /* std*dt_sqrt */
  float den;        /* 2*(std*dt_sqrt)^2 */
  float log_sd;
  float log_c;
} mgx_dpm_coeffs;

/* dpm_step (sampling_utils.py:273-385) for DPM-Solver / DPM-Solver++ orders 1-3.  m1/m2 are the previous
 * x0 predictions (fp32, NULL when order is lower); x0_out receives this step's x0 (the new m0). */
int mgx_dpm_step_fwd(const float* sample, const uint16_t* v, const float* m1, const float* m2, const float* noise,
                     float* x_out, float* x0_out, float* logp, double* ws, int B, long n,
                     const mgx_dpm_coeffs* k /*host*/, void* stream);

/* d log_prob / d model_output of a first-order SDE dpm_step whose sample x_t is held fixed: the training replay under
 * dpm_apply_strategy="all" (train_grpo_flux.py:170-180 calls dpm_step with dpm_state=None; the log-prob's gradient runs
 * through prev_sample_mean, sampling_utils.py:376-383).  sigma_b: the scalar autograd multiplies by in d(sigma*v)/dv. */
int mgx_dpm_step_bwd(const float* sample, const uint16_t* v, const float* x_t, const float* g_logp, uint16_t* dv, int B,
                     long n, const mgx_dpm_coeffs* k /*host, order 1*/, float sigma_b, void* stream);

/* convert_model_output alone (sampling_utils.py:387-396; used at :116 to feed DPMState inside the window) */
int mgx_x0_pred(const float* sample, const uint16_t* v, float* x0_out, long total, float sigma_x0, void* stream);

/* pack_latents / unpack_latents (train_grpo_flux.py:94-115): [B,C,H,W] <-> [B,(H/2)(W/2),4C]; elem_size 2|4 */
int mgx_pack_latents(const void* in, void* out, int B, int C, int H, int W, int elem_size, void* stream);
int mgx_unpack_latents(const void* in, void* out, int B, int C, int H, int W, int elem_size, void* stream);

/* ------------------------------------------------------------------------------------------------ GRPO
 * Group-relative advantage (train_grpo_flux.py:440-491): per group of G consecutive rewards,
 * (r-mean)/(unbiased std+1e-8).  trim < 0: statistics over the whole group in its own order (trimmed_ratio <= 0);
 * trim >= 0: over the sorted group without its `trim` smallest rewards, also for trim == 0.  The caller forms
 * trim = min(int(G * trimmed_ratio), G - 1) in DOUBLE, as the reference does (:454; a float product differs from it
 * for 107 of the (G <= 1024, ratio k/100) pairs); trim >= G is refused.
 * out[i] (+)= weight * advantage (accumulate!=0 implements the multi-reward sum of :465-467). */
int mgx_group_advantage(const float* rewards, float* out, int n, int G, int trim, float weight, int accumulate,
                        void* stream);
/* Global normalisation for use_group=False (:498): (r - mean(all))/(std(all)+1e-8); all = gathered rewards */
int mgx_global_advantage(const float* rewards, const float* gathered, float* out, int n, int n_all, void* stream);

/* PPO-clip GRPO loss per replayed transition (train_grpo_flux.py:560-583), batch of B independent
 * (sample, step) pairs: loss/policy/kl/clip_frac per element and g_logp = dloss/dnew_logp. */
int mgx_grpo_loss(const float* new_logp, const float* old_logp, const float* adv, int B, float clip_range,
                  float adv_clip_max, float kl_coeff, float denom, float* loss, float* policy, float* kl,
                  float* clip_frac, float* g_logp, void* stream);

/* ------------------------------------------------------------------------------------------------ MMDiT
 * The FLUX MMDiT is third-party code for the reference (diffusers 0.32.2 FluxTransformer2DModel, call sites
 * fastvideo/utils/sampling_utils.py:68-82 and fastvideo/train_grpo_flux.py:134-144); each entry point below
 * replaces the torch/cuBLAS/SDPA kernels that module launches under autocast(bf16).
 *
 * Row-batched matrices: row m lives at base + (m / rpb) * bstride + (m % rpb) * ld (elements).  A plain
 * matrix has rpb >= M.  This lets the text rows and image rows of the joint [B, S, d] stream be operands
 * without a concat/split copy.
 */
enum { MGX_EPI_BIAS = 0, MGX_EPI_BIAS_GELU = 1, MGX_EPI_BIAS_GATE_RES = 2, MGX_EPI_F32_ACC = 3, MGX_EPI_DGELU = 4 };

/* C[M,N] = epi(A[M,K] @ W[N,K]^T + bias[N]); bf16 in, fp32 accumulate (MFMA), one rounding to bf16
 * (nn.Linear under autocast).  Epilogues:
 *   MGX_EPI_BIAS          C = bf16(acc + bias)
 *   MGX_EPI_BIAS_GELU     C = bf16(gelu_tanh(bf16(acc + bias)));  aux (optional) receives the pre-activation
 *   MGX_EPI_BIAS_GATE_RES C = bf16(C + bf16(gate[m/c_rpb, n] * bf16(acc + bias)));  aux (optional) <- pre-gate
 *   MGX_EPI_F32_ACC       C(fp32) = beta * C + acc                  (weight gradients)
 *   MGX_EPI_DGELU         C = bf16(bf16(acc) * gelu_tanh'(aux))     (input gradient through GELU)
 * aux is a plain [M, ldaux] matrix.  K % 64 == 0, N % 4 == 0; M, N tails are masked. */
int mgx_gemm_bf16(const uint16_t* A, const uint16_t* W, const uint16_t* bias, void* C, const uint16_t* gate,
                  uint16_t* aux, long ldaux, int M, int N, int K, long lda, long a_rpb, long a_bstride, long ldw, long ldc,
                  long c_rpb, long c_bstride, long gate_ld, int epilogue, float beta, void* stream);
/* The same GEMM with a caller-owned fp32 workspace of mgx_gemm_sk_workspace_elems() floats (one per stream in use): the
 * persistent kernel may then share the tiles of its last, partial round out along K ("stream-K tail": partial sums through
 * the workspace, added in K order by a second launch -- deterministic, and a given shape is always split the same way).
 * Results can differ from mgx_gemm_bf16's in the last bit of the fp32 sum.  sk_workspace == NULL: identical to mgx_gemm_bf16.
 * Replaces the same torch/cuBLAS nn.Linear launches (fastvideo/utils/sampling_utils.py:68-82, train_grpo_flux.py:134-144,600). */
long mgx_gemm_sk_workspace_elems(void);
int mgx_gemm_bf16_sk(const uint16_t* A, const uint16_t* W, const uint16_t* bias, void* C, const uint16_t* gate,
                     uint16_t* aux, long ldaux, int M, int N, int K, long lda, long a_rpb, long a_bstride, long ldw, long ldc,
                     long c_rpb, long c_bstride, long gate_ld, int epilogue, float beta, float* sk_workspace,
                     long sk_workspace_elems, void* stream);
/* The q | k projection of an attention layer with mgx_qk_norm_rope_fwd_qs applied in the GEMM's epilogue, on the tile while
 * it is in registers: X [B * rows_per_batch, K] (plain), Wqk [2 * H * 128, K] (to_q rows, then to_k rows), bias [2 * H * 128]
 * -> Q, K [B, H, S, 128] at sequence positions s0 .. s0 + rows_per_batch - 1, Q times q_scale.  The [tokens, 2 H 128]
 * projection output is neither written nor re-read.  Same bits as mgx_gemm_bf16 followed by mgx_qk_norm_rope_fwd_qs
 * (diffusers' to_q / to_k Linears + norm_q / norm_k + apply_rotary_emb; call sites fastvideo/utils/sampling_utils.py:68-82).
 * cos_sin_pairs (optional): [S, 64, 2] fp32 = (cos[s][2i], sin[s][2i]) for tables whose two entries of a rotation pair are
 * equal (diffusers' FluxPosEmbed repeat_interleaves them) -- the caller's promise; the epilogue then reads half the table
 * bytes, which are what it costs (profiles/r04_qknorm_epilogue_prices.log).
 * Returns 1 -- nothing launched -- when the persistent kernel cannot take the problem (fewer than 128 output tiles of
 * 256 x 256, H odd, rows_per_batch % 128 != 0, alignments below 16 bytes, MGX_GEMM_QKNORM=0): keep the two-pass form. */
int mgx_linear_qk_norm_rope(const uint16_t* X, const uint16_t* Wqk, const uint16_t* bias, const float* wq, const float* wk,
                            const float* cos, const float* sin, const float* cos_sin_pairs /* optional, see above */,
                            uint16_t* Q, uint16_t* K, int B, int H, int S, int rows_per_batch, int s0, int Kdim, long ldx,
                            long ldw, float q_scale, void* stream);

/* A Linear whose output leaves TRANSPOSED: Ct[b][f][t] = bf16(X[b * tok_rpb + t, :] . W[f, :] + bias[f]), ld_ct elements
 * between feature rows, ct_bstride between token batches -- the V^T [B, H, 128, Sp] operand of mgx_attn_fwd* straight from
 * the value projection (the nn.Linear to_v / add_v_proj of diffusers' FluxAttnProcessor2_0 followed by the transpose SDPA's
 * kernels do internally; call sites fastvideo/utils/sampling_utils.py:68-82), mgx_qk_norm_rope_fwd* then called with Vt = NULL.
 * Same persistent kernel with the operand roles swapped.  Returns 1 -- nothing launched -- for shapes that kernel cannot take
 * (fewer than 128 output tiles of 256 x 256, tok_rpb % 64 != 0 with several batches, alignments below 16 bytes): the caller
 * then keeps the plain projection + mgx_qk_norm_rope_fwd's transposing pass. */
int mgx_linear_bf16_t(const uint16_t* X, const uint16_t* W, const uint16_t* bias, uint16_t* Ct, int tokens, int F, int K,
                      long ldx, long ldw, long ld_ct, long tok_rpb, long ct_bstride, float* sk_workspace,
                      long sk_workspace_elems, void* stream);

/* What mgx_gemm_bf16_sk launches for dense operands (lda = ldw = K) of this shape, with (stream_k != 0) or without a
 * workspace: the plan the kernels themselves walk (csrc/gemm_plan.h), for tests and tools.  No GPU needed.
 * mgx_gemm_plan: out[0..5] = kernel family (0: 128x128 tiles, 1: persistent 256x256), grid, band, sk_minparts, fix-up
 * blocks (0: nothing is split), XCDs that split their tail (bit x: XCD x); returns 6.
 * mgx_gemm_plan_units, fixup == 0: workgroup `index` of the main kernel; returns its number of units, unit i =
 * out[5 i .. 5 i + 4] = (m0, n0, first K-tile, end K-tile, partial: 1 = its sums go to workspace slot `index`).
 * fixup != 0: fix-up block `index`; returns the number of workspace slots it adds (0: the block is idle), out[0..1] = (m0, n0)
 * of the tile it finishes, out[2 ..] = the slots in the order it adds them.  Both return -1 on a bad argument. */
int mgx_gemm_plan(int M, int N, int K, int stream_k, int* out, int cap);
int mgx_gemm_plan_units(int M, int N, int K, int stream_k, int fixup, int index, int* out, int cap);

/* out[N, ld_out] = in[M, N]^T (bf16; columns M..ld_out-1 are zero-filled) and, optionally, fp32 column sums
 * colsum_out[n] = beta*colsum_out[n] + sum_m in[m, n] (bias gradients) via a deterministic two-stage reduction;
 * colsum_partial needs mgx_transpose_partial_elems(M, N) floats. */
long mgx_transpose_partial_elems(int M, int N);
int mgx_transpose_bf16(const uint16_t* in, uint16_t* out, float* colsum_partial, float* colsum_out, float colsum_beta,
                       int M, int N, long ld_in, long in_rpb, long in_bstride, long ld_out, void* stream);

/* y[M, D] = bf16( LayerNorm(x[m,:]; eps 1e-6, no affine) * bf16(1 + scale[b,:]) + shift[b,:] ), b = m / x_rpb
 * (AdaLayerNormZero / ...Single / ...Continuous normalisation).  shift/scale point at their chunk inside the
 * modulation vector [B, mod_ld].  stats (optional) receives (mean, rstd) per row.  D % 512 == 0, D <= 4096. */
int mgx_ln_modulate_fwd(const uint16_t* x, long ldx, long x_rpb, long x_bstride, const uint16_t* shift,
                        const uint16_t* scale, long mod_ld, uint16_t* y, long ldy, float* stats, long M, int D,
                        void* stream);
/* Backward of the above: dx = bf16(dLN), or with `accumulate` dx = bf16(dx + dLN) (ONE rounding of the fp32 sum of the old
 * bf16 value and dLN); dshift/dscale (bf16, [B, mod_ld] chunks) are written (not accumulated) with per-batch column sums. */
long mgx_ln_modulate_bwd_workspace(long M, long rpb, int D);
int mgx_ln_modulate_bwd(const uint16_t* dy, long lddy, const uint16_t* x, long ldx, long x_rpb, long x_bstride,
                        const uint16_t* scale, long mod_ld, uint16_t* dx, long lddx, long dx_rpb, long dx_bstride,
                        int accumulate, uint16_t* dshift, uint16_t* dscale, float* ws, long M, int D, void* stream);

/* Per-head RMSNorm(eps 1e-6, fp32 weight[128]) on q,k + interleaved-pair RoPE (fp32 cos/sin [S,128]) + head
 * split: qkv [B*rows_per_batch, 3*H*128] -> Q,K [B,H,S,128] (rounded once to bf16), Vt [B,H,128,Sp], written
 * at sequence positions s0 .. s0+rows_per_batch-1 of the joint sequence (diffusers FluxAttnProcessor2_0). */
/* V, Qt, Kt (all or none): extra layouts the attention backward consumes -- V row-major [B,H,S,128] and
 * Q^T, K^T [B,H,128,Sp] (padding must be finite: allocate zeroed).  Vt = NULL (without the extras): the v columns are not
 * read and V^T is not written (mgx_linear_bf16_t wrote it). */
int mgx_qk_norm_rope_fwd(const uint16_t* qkv, long ld, const float* wq, const float* wk, const float* cos,
                         const float* sin, uint16_t* Q, uint16_t* K, uint16_t* Vt, uint16_t* V, uint16_t* Qt,
                         uint16_t* Kt, int B, int H, int S, int Sp, int rows_per_batch, int s0, void* stream);
/* ..._qs: Q (and Qt) leave as bf16(q * q_scale) -- one rounding, of the scaled value.  With q_scale = softmax scale * log2(e)
 * the scores Q K^T are exponents of two: what mgx_attn_fwd_log2 consumes; every other consumer of that Q takes `scale` = ln 2
 * (mgx_attn_bwd, mgx_attn_fwd_fp8), and mgx_qk_norm_rope_bwd_qs multiplies the incoming dQ by the same q_scale. */
int mgx_qk_norm_rope_fwd_qs(const uint16_t* qkv, long ld, const float* wq, const float* wk, const float* cos,
                            const float* sin, uint16_t* Q, uint16_t* K, uint16_t* Vt, uint16_t* V, uint16_t* Qt,
                            uint16_t* Kt, int B, int H, int S, int Sp, int rows_per_batch, int s0, float q_scale,
                            void* stream);
long mgx_qk_norm_rope_bwd_workspace(int B, int H, int rows_per_batch);
int mgx_qk_norm_rope_bwd(const uint16_t* qkv, long ld, const float* wq, const float* wk, const float* cos,
                         const float* sin, const uint16_t* dQ, const uint16_t* dK, const uint16_t* dV, uint16_t* dqkv,
                         long ld_dqkv /* elements between rows of dqkv, >= ld */, float* gwq, float* gwk, float* ws, int B,
                         int H, int S, int Sp, int rows_per_batch, int s0, void* stream);

int mgx_qk_norm_rope_bwd_qs(const uint16_t* qkv, long ld, const float* wq, const float* wk, const float* cos,
                            const float* sin, const uint16_t* dQ, const uint16_t* dK, const uint16_t* dV, uint16_t* dqkv,
                            long ld_dqkv, float* gwq, float* gwk, float* ws, int B, int H, int S, int Sp,
                            int rows_per_batch, int s0, float q_scale, void* stream);

/* O = softmax(scale * Q K^T) V, non-causal, head_dim 128 (F.scaled_dot_product_attention under autocast):
 * Q,K [B,H,S,128], Vt [B,H,128,Sp], O [B,S,ldo] at column h*128 (columns outside the head blocks and the gap between
 * batches when o_bstride > S * ldo are not written), lse [B,H,S] (optional, natural log) for the backward pass.
 * Sp: any multiple of 64 that is >= S.  The padding columns s >= S of Vt (and of Qt, Kt, below) are read and multiplied by
 * probabilities that are exactly zero, so they may hold ANY FINITE values (not NaN / inf: 0 * inf); they are never written.
 * Sp > S with S % 256 == 0 (more padding than S rounded up to 64 needs) is accepted but costs the generated 64-wide kernels:
 * those take Sp == S only, the 8-wave kernels run instead (mgx_attn_fwd_path / mgx_attn_bwd_path tell). */
int mgx_attn_fwd(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, uint16_t* O, float* lse, int B, int H, int S,
                 int Sp, long ldo, long o_bstride, float scale, void* stream);

/* The same with Q2 = Q * scale * log2(e) (mgx_qk_norm_rope_fwd_qs): P = 2^(Q2 K^T - m), lse still the natural logarithm.
 * On the 64-query kernel (S % 256 == 0) the running maximum is subtracted by the matrix pipe -- a score tile's accumulator
 * starts at -m -- and the per-score multiply-add of the softmax is gone (csrc/gen/attn_fwd64.py, ACC). */
int mgx_attn_fwd_log2(const uint16_t* Q2, const uint16_t* K, const uint16_t* Vt, uint16_t* O, float* lse, int B, int H,
                      int S, int Sp, long ldo, long o_bstride, void* stream);

/* Which kernels mgx_attn_fwd / mgx_attn_fwd_log2 and mgx_attn_bwd launch for a problem: 0 = the 8-wave kernels, 1 = the
 * generated 64-wide ones (S % 256 == 0, Sp == S, offsets within their 32-bit / 24-bit fields; the forward also needs the
 * persistent walk's stride / (S / 256) < H, csrc/attention.hip), negative = the sizes are refused.  The launchers call the
 * same predicate; MGX_ATTN_W64=0 (read per call) forces 0.  Launches nothing. */
int mgx_attn_fwd_path(int B, int H, int S, int Sp, long ldo, long o_bstride);
int mgx_attn_bwd_path(int B, int H, int S, int Sp, long ldo, long o_bstride);

/* mgx_attn_fwd_log2 with a masked key tail, for a sequence padded to a multiple of 256 so that the 64-query kernel (and the
 * fused projections in front of it) apply: the no-grad F.scaled_dot_product_attention of the rollout,
 * fastvideo/utils/sampling_utils.py:68-82, at resolutions whose token count is off 256 (720 x 720: 512 + 2025 = 2537 -> 2560).
 * Everything is allocated at Sa, Sa % 256 == 0: Q2, K [B,H,Sa,128], Vt [B,H,128,Sa], O with Sa rows per batch
 * (o_bstride >= Sa * ldo), lse [B,H,Sa] (optional).  Sa - 256 < kv_len <= Sa.  Rows of Q2 / K and columns of Vt >= kv_len may
 * hold ANY FINITE values: such keys get probability exactly 0 (their score is replaced by -inf before the softmax), and the
 * padding rows of Q2 are not read at all.  Queries are not masked: rows < kv_len of O and lse are softmax attention over the
 * keys 0 .. kv_len - 1 only (lse the natural logarithm over those keys) and do not depend on the padding by a bit; rows
 * >= kv_len are written with unspecified finite values (today: those of row kv_len - 1).  kv_len == Sa gives the bits of
 * mgx_attn_fwd_log2.  Its backward is mgx_attn_bwd_kv.
 * Returns 1 and launches NOTHING when the 64-query kernel cannot take the problem -- mgx_attn_fwd_path(B, H, Sa, Sa, ..) is 0
 * (the persistent walk, Sa % 256, the offset fields, MGX_ATTN_W64=0) or kv_len is out of range: the caller keeps its unpadded
 * path, as with mgx_linear_qk_norm_rope.  mgx_attn_fwd_kv_path is that predicate (1 = taken, 0 = refused), launches nothing. */
int mgx_attn_fwd_log2_kv(const uint16_t* Q2, const uint16_t* K, const uint16_t* Vt, uint16_t* O, float* lse, int B, int H,
                         int Sa, int kv_len, long ldo, long o_bstride, void* stream);
int mgx_attn_fwd_kv_path(int B, int H, int Sa, int kv_len, long ldo, long o_bstride);

/* fp8 (OCP e4m3) variant of mgx_attn_fwd: the "fp8 MFMA attention path" of BASELINE.json configs[4].  The reference
 * has no fp8 attention; the entry points serve the same SDPA call sites (fastvideo/utils/sampling_utils.py:68-82,
 * train_grpo_flux.py:134-144).
 * mgx_attn_fp8_quantize: amax [3][B*H] fp32 (|max| of Q, K, V per batch-head, V over the S valid keys), Q8/K8
 * [B,H,S,128] = e4m3(x * 448 / amax), V8t [B,H,128,Sp] likewise with the keys of every 64-key block in the order
 * p = 32h + 16kb + i  <-  key 32kb + 8(i>>2) + 4h + (i&3)  (the order the kernel's P^T fragment holds them).
 * mgx_attn_fwd_fp8: O, lse as mgx_attn_fwd from the quantised operands (both contractions on e4m3 MFMA, P in e4m3,
 * fp32 statistics / accumulators).  The backward is mgx_attn_bwd on the bf16 operands with this O / lse, or mgx_attn_bwd_fp8. */
int mgx_attn_fp8_quantize(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, uint8_t* Q8, uint8_t* K8,
                          uint8_t* V8t, float* amax, int B, int H, int S, int Sp, void* stream);
int mgx_attn_fwd_fp8(const uint8_t* Q8, const uint8_t* K8, const uint8_t* V8t, const float* amax, uint16_t* O,
                     float* lse, int B, int H, int S, int Sp, long ldo, long o_bstride, float scale, void* stream);

/* Backward of mgx_attn_fwd (P recomputed from lse): dQ, dK, dV [B,H,S,128].  Inputs Q,K,V row-major, Qt,Kt
 * [B,H,128,Sp] (mgx_qk_norm_rope_fwd extras; padding columns s >= S finite, see mgx_attn_fwd), O and dO [B,S,ldo] at
 * column h*128.  delta [B,H,S] fp32 and dOt [B,H,128,Sp] bf16 are caller-provided scratch that the internal prep kernel
 * fills completely: delta[b,h,s] = sum_d dO * O in fp32 from the bf16 O passed in (the forward's rounded output, not its
 * fp32 accumulator), dOt = the head's dO columns transposed, zero in the padding columns s >= S (nothing beyond Sp). */
int mgx_attn_bwd(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* Qt, const uint16_t* Kt,
                 const uint16_t* O, const uint16_t* dO, const float* lse, float* delta, uint16_t* dOt, uint16_t* dQ,
                 uint16_t* dK, uint16_t* dV, int B, int H, int S, int Sp, long ldo, long o_bstride, float scale,
                 void* stream);

/* Opt-in e4m3 backward of mgx_attn_fwd_fp8 (csrc/attention_fp8_bwd.hip): the straight-through gradient of the quantised
 * forward.  The argument list and the meaning of `scale` are mgx_attn_bwd's (O, lse: what mgx_attn_fwd_fp8 wrote); dOt is
 * filled by the same prep kernel, delta leaves as sum_d dO8 * O on the dequantised e4m3 dO (the dO that dP is formed from).  Q8, K8, V8 are requantised from the bf16 Q, K, V handed in (the forward's quantiser:
 * same inputs, same bits), dO per (batch, head) like them; S is recomputed with the forward's instruction, so
 * P = exp(S - lse) is the forward's probability.  All five products run on the scaled e4m3 MFMA: P enters dV as e4m3(256 P),
 * dS = P (dP - delta) enters dK and dQ as MX blocks (32 contiguous values along the contraction dimension share a power-of-two
 * scale).
 * Any S >= 1; only rows < S of dQ, dK, dV [B,H,S,128] are written; the padding columns of Qt, Kt may hold anything.
 * amax: float [4][B*H], written (Q, K, V, dO).  ws: mgx_attn_bwd_fp8_workspace(B, H, S, Sp) bytes, 16-byte aligned, ws_bytes its
 * size; sections in order Q8, K8, V8, dO8 [B,H,S,128] e4m3 (each rounded up to a multiple of 256 bytes), then Q8t, K8t, dO8t
 * [B,H,128,Sp]: transposed, zero from column S on, the columns of every 64-block in the order of V8t (mgx_attn_fp8_quantize).
 * mgx_attn_bwd_fp8_workspace is host code (needs no GPU); -1 for sizes mgx_attn_bwd_fp8 refuses. */
long mgx_attn_bwd_fp8_workspace(int B, int H, int S, int Sp);
int mgx_attn_bwd_fp8(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* Qt, const uint16_t* Kt,
                     const uint16_t* O, const uint16_t* dO, const float* lse, float* delta, uint16_t* dOt, uint16_t* dQ,
                     uint16_t* dK, uint16_t* dV, uint8_t* ws, float* amax, int B, int H, int S, int Sp, long ldo,
                     long o_bstride, float scale, long ws_bytes, void* stream);

/* mgx_attn_bwd with a masked tail: the backward of mgx_attn_fwd_log2_kv (autograd of F.scaled_dot_product_attention,
 * fastvideo/train_grpo_flux.py:134-144, at a token count off 256), on the generated 64-wide pair and nothing else.
 * Everything is allocated at Sa, Sa % 256 == 0: Q, K, V, dQ, dK, dV [B,H,Sa,128], Qt, Kt, dOt [B,H,128,Sa], lse, delta
 * [B,H,Sa], O and dO with Sa rows per batch (o_bstride >= Sa * ldo).  Sa - 256 < kv_len <= Sa; keys AND queries >= kv_len are
 * padding.  Rows >= kv_len of Q, K, V, O, dO, lse and columns >= kv_len of Qt, Kt may hold ANY FINITE values -- no bound on
 * their magnitude: what they make of a score or a dP is replaced by a select, never multiplied away, the padding rows of Q, dO,
 * lse (dQ kernel) and of K, V (dK / dV kernel) are not read at all, and the padding rows of O and dO are not read by the prep.
 * Rows < kv_len of dQ, dK, dV, and of delta / columns < kv_len of dOt, are the backward of attention over the keys and
 * queries 0 .. kv_len - 1 only and do not depend on the padding by a bit.  Rows >= kv_len of dQ, dK, dV and of delta, and
 * columns >= kv_len of dOt, are written as ZERO (dQ / dK / dV possibly -0): the layers behind the attention take nothing from
 * the padding tokens.  kv_len == Sa gives the bits of mgx_attn_bwd at S = Sp = Sa.  `scale` as mgx_attn_bwd (for the log2
 * forward: ln 2 on Q2).
 * Returns 1 and launches NOTHING when the problem cannot be taken -- mgx_attn_bwd_path(B, H, Sa, Sa, ..) is 0 (Sa % 256, the
 * offset fields, MGX_ATTN_W64=0), kv_len is out of range or o_bstride < Sa * ldo: there is no other kernel behind this entry
 * point, the caller keeps its unpadded path.  mgx_attn_bwd_kv_path is that predicate (1 = taken, 0 = refused), launches
 * nothing. */
int mgx_attn_bwd_kv(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* Qt, const uint16_t* Kt,
                    const uint16_t* O, const uint16_t* dO, const float* lse, float* delta, uint16_t* dOt, uint16_t* dQ,
                    uint16_t* dK, uint16_t* dV, int B, int H, int Sa, int kv_len, long ldo, long o_bstride, float scale,
                    void* stream);
int mgx_attn_bwd_kv_path(int B, int H, int Sa, int kv_len, long ldo, long o_bstride);

/* The launch operands that the masked 64-wide kernels derive from kv_len (csrc/attn_operands.h, the one derivation the
 * kernels call), for the CPU tests that hold them equal to the generators' kv_operands.  stream: 0 = mgx_attn_fwd_log2_kv
 * (nloop, kmax, vmax, kt, kvm1), 1 = dQ (nloop, seq, kt0, kt1, qlast), 2 = dK / dV (nloop, qmax, cmax, qk, klast), the last two
 * of mgx_attn_bwd_kv; block = the workgroup's 256-row block (streams 1 and 2).  Writes the values to out[0 .. cap) in that
 * order and returns their count (5); MGX_ERR_ARG for another stream, kv_len < 1, a null out or cap too small.  Host code
 * only: needs no GPU. */
int mgx_attn_kv_operands(int stream, int kv_len, int block, int* out, int cap);

/* out[b, :] = bf16(x[b, :] @ W[N,K]^T + bias), 1 <= Bn <= 16 rows (temb MLPs, AdaLN modulation linears) */
int mgx_skinny_linear(const uint16_t* x, long ldx, const uint16_t* W, long ldw, const uint16_t* bias, uint16_t* out,
                      long ldo, int Bn, int N, int K, void* stream);
/* dW[N,K] (fp32) += dout[Bn,N]^T x[Bn,K]; dbias[N] (fp32, optional) += column sums of dout */
int mgx_skinny_wgrad(const uint16_t* dout, long ldd, const uint16_t* x, long ldx, float* dW, long ldw, float* dbias,
                     int Bn, int N, int K, void* stream);
/* dx[Bn,K] (bf16; += when accumulate) = bf16(dout[Bn,N] W[N,K]), 1 <= Bn <= 8: the input gradient of the same skinny linears
 * (autograd of diffusers' AdaLayerNormZero(.Single).linear / AdaLayerNormContinuous.linear, called from
 * train_grpo_flux.py:600 `loss.backward()`), read straight from the row-major weight.  ws: fp32 scratch of
 * mgx_skinny_dgrad_workspace(Bn, K) elements. */
long mgx_skinny_dgrad_workspace(int Bn, int K);
int mgx_skinny_dgrad(const uint16_t* dout, long ldd, const uint16_t* W, long ldw, uint16_t* dx, long lddx, float* ws,
                     int Bn, int N, int K, int accumulate, void* stream);
/* bf16 elementwise: op 0 y=silu(a) | 1 y=b*silu'(a) | 2 y=a+b | 3 y+=a */
int mgx_ew_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, long n, int op, void* stream);
/* diffusers Timesteps(256, flip_sin_to_cos=True, shift 0): out[b] = bf16([cos(t_b f) | sin(t_b f)]) */
int mgx_sincos_embed(const float* t, uint16_t* out, int Bn, void* stream);
int mgx_cast_f32_bf16(const float* x, uint16_t* y, long n, void* stream);
/* y = scale * float(x) (n % 8 == 0).  With mgx_cast_f32_bf16: the bf16 gradient buckets of the data-parallel all-reduce
 * (the reference's FSDP reduce-scatters its gradients per wrapped block, fastvideo/utils/fsdp_util.py:56-66) */
int mgx_cast_bf16_f32(const uint16_t* x, float* y, long n, float scale, void* stream);
/* out[N, ld_out] = (bf16(gelu_tanh(float(in[M, N]))))^T, columns M..ld_out-1 zero-filled: the weight-gradient operand of
 * ff.net.2 / proj_out formed straight from a KEPT pre-activation (the values mgx_gelu_bf16 would write, transposed; autograd of
 * diffusers' FeedForward / FLUX single-block act_mlp under train_grpo_flux.py:600 `loss.backward()`).  N, ld_in, ld_out % 8 == 0. */
int mgx_transpose_gelu_bf16(const uint16_t* in, uint16_t* out, int M, int N, long ld_in, long ld_out, void* stream);
/* y[m][0..N) = bf16(gelu_tanh(float(x[m][0..N)))), rows ldx / ldy elements apart (N, ldx, ldy % 8 == 0, 16-byte aligned):
 * the activation of diffusers' FeedForward(activation_fn="gelu-approximate") / FLUX single block `act_mlp` re-created from a
 * KEPT pre-activation, bit-identical to what mgx_gemm_bf16's bias+GELU epilogue writes (it applies GELU to the bf16-rounded
 * Linear output); used by the activation-recompute pass the reference gets from torch.utils.checkpoint
 * (fastvideo/utils/fsdp_util.py:26-66) to skip a GEMM whose input it kept. */
int mgx_gelu_bf16(const uint16_t* x, long ldx, uint16_t* y, long ldy, long M, int N, void* stream);
/* Backward of x + gate*y: dy = bf16(gate[b]*dout), dgate[b,:] = sum_rows dout*y (bf16) */
long mgx_gate_bwd_workspace(long batches, long rows_per_batch, int D);
int mgx_gate_bwd(const uint16_t* dout, long ldd, long d_bstride, const uint16_t* y, long ldy, const uint16_t* gate,
                 long gate_ld, uint16_t* dy, long lddy, uint16_t* dgate, float* ws, int batches, long rows_per_batch,
                 int D, void* stream);

/* ------------------------------------------------------------------------------------------------ optimizer
 * out[0] = beta*out[0] + sum g^2 (fp64 two-stage reduction; ws >= mgx_sqnorm_workspace() doubles):
 * the global grad norm of transformer.clip_grad_norm_ (train_grpo_flux.py:606). */
long mgx_sqnorm_workspace(void);
int mgx_sqnorm_f32(const float* g, long n, double* ws, float* out, float beta, void* stream);
/* torch.optim.AdamW step (train_grpo_flux.py:715-721,607) on flat fp32 master weights, fused with the
 * clip-by-global-norm scaling (gnorm_sq: device pointer to sum g^2 of the UNSCALED grads, or NULL for no
 * clipping; grad_scale multiplies every gradient first, e.g. 1/world_size) and the bf16 compute-copy refresh. */
/* lr, betas, eps and weight decay are DOUBLES, as the Python floats torch.optim.AdamW holds them: every derived coefficient
 * (1 - beta2, lr / (1 - beta1^step), ...) is formed in double and rounded to fp32 once, like torch's foreach step does. */
int mgx_adamw_step(float* w, uint16_t* w16, const float* g, float* m, float* v, long n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int step, const float* gnorm_sq, float max_norm,
                   float grad_scale, void* stream);
int mgx_scale_f32(float* x, long n, float s, void* stream);


/* ------------------------------------------------------------------------------------------------ VAE decode
 * `vae.decode(latents)` of fastvideo/train_grpo_flux.py:279-289: diffusers' AutoencoderKL decoder (bf16 weights, bf16 autocast;
 * its block structure is the 2-D original of the reference's vendored fastvideo/models/hunyuan/vae/unet_causal_3d_blocks.py
 * :404-462 ResnetBlock, :667-693 mid block, :148-206 upsample, and of vae.py:251-312 Decoder.forward).  Activations are NHWC
 * bf16 for one image: "plain" = [H W][C], "padded" = [(H + 2)(W + 2)][C] with a zero border that is the convolution's padding.
 *
 * 3x3 convolution, stride 1, padding 1, as an implicit GEMM on the MFMA GEMM kernels (K = 9 taps x C channels, no im2col):
 * x padded NHWC, C in {64, 128, 256, 512}; Wt [Cout][3][3][C] bf16 (tap-major); out plain [H W][ld_out], Cout % 4 == 0.
 * residual != 0: out = bf16(out + bf16(conv + bias)) (`input_tensor + hidden_states` of a ResnetBlock2D); `ones` = Cout bf16 ones. */
int mgx_conv3x3_nhwc(const uint16_t* x, const uint16_t* Wt, const uint16_t* bias, uint16_t* out, long ld_out,
                     const uint16_t* ones, int H, int W, int C, int Cout, int residual, void* stream);
/* y = [silu](GroupNorm(x; G groups, eps, affine gamma / beta [C] bf16)) in fp32 on a plain bf16 image x [H W][ld], one rounding
 * to bf16 at the store.  Output pixel (y, x) goes to out + y * out_row + x * out_px (elements): a plain matrix or the interior of
 * a padded image.  The group statistics (E[x^2] - mean^2) are summed in fp64 from fp32 chains of 64 rows, which are exact for
 * bf16 data.  ws: fp32 scratch of mgx_group_norm_workspace(H W, C, G) elements, 8-byte aligned. */
long mgx_group_norm_workspace(long M, int C, int G);
int mgx_group_norm_nhwc(const uint16_t* x, long ld, const uint16_t* gamma, const uint16_t* beta, uint16_t* out, long out_row,
                        long out_px, float* ws, int H, int W, int C, int G, float eps, int silu, void* stream);
/* nearest-neighbour 2x (F.interpolate(scale_factor=2, mode="nearest")): plain [H W][C] -> interior of a padded
 * [(2H + 2)(2W + 2)][C] image; `out` points at its pixel (1, 1) */
int mgx_upsample2x_pad_nhwc(const uint16_t* x, uint16_t* out, int H, int W, int C, void* stream);
/* latents [Cin][H][W] fp32 -> bf16 interior of a padded NHWC image of C >= Cin channels (`out` at pixel (1, 1)) */
int mgx_latents_to_pad_nhwc(const float* z, uint16_t* out, int Cin, int H, int W, int C, void* stream);
/* first Cout channels of a plain NHWC image -> [Cout][H][W] bf16 */
int mgx_nhwc_to_image(const uint16_t* x, long ld, uint16_t* img, int Cout, int H, int W, void* stream);
/* P[r, :n] = bf16(softmax(scale * S[r, :n])), S fp32 (the mid block's single-head attention over H W <= 16384 tokens) */
int mgx_softmax_rows_f32(const float* S, long lds, uint16_t* P, long ldp, int M, int n, float scale, void* stream);

/* ---- VAE encode: the encoder half of the same AutoencoderKL (`vae.encode(x).latent_dist`), on the kernels above plus these.
 * The encoder's downsampler, diffusers' Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then Conv2d(3, stride=2) -- semantics
 * recollected, PARITY UNPINNED (diffusers is not vendored by the reference; its fastvideo/models/hunyuan/vae/
 * unet_causal_3d_blocks.py:208 DownsampleCausal3D witnesses the structure only, its padding differs).
 * x: padded NHWC image of an H x W activation, H and W even, C in {64, 128, 256, 512}; out plain [(H/2)(W/2)][ld_out]:
 * out(y, x) = bias + sum_{ky,kx} w[ky][kx] . in(2y + ky, 2x + kx), `in` zero outside the activation (the bottom / right border of
 * x; its top / left border is never read).  Wt, bias, Cout, alignments as for mgx_conv3x3_nhwc; no residual form. */
int mgx_conv3x3s2_nhwc(const uint16_t* x, const uint16_t* Wt, const uint16_t* bias, uint16_t* out, long ld_out, int H, int W,
                       int C, int Cout, void* stream);
/* first C channels of a plain [H W][ld] image -> interior of a padded [(H + 2)(W + 2)][C] image (`out` at pixel (1, 1)); 16-byte
 * copies: C % 8 == 0, ld % 8 == 0.  The downsampler's input: a ResnetBlock's output (unet_causal_3d_blocks.py:404-462) is plain. */
int mgx_pad_nhwc(const uint16_t* x, long ld, uint16_t* out, int H, int W, int C, void* stream);
/* DiagonalGaussianDistribution (fastvideo/models/hunyuan/vae/vae.py:321-353, .mode() :384) as torch evaluates it on bf16 tensors,
 * every op rounding to bf16: moments plain NHWC [H W][ld], channels [0, Cz) the mean, [Cz, 2 Cz) the logvar (chunk, :331) ->
 * [Cz][H][W] bf16 each: mean; std = bf16(exp(bf16(0.5 * clamp(logvar, -30, 20)))) (:332,334);
 * sample = bf16(mean + bf16(std * noise)) (:352), noise [Cz][H][W] bf16; noise == NULL: sample = mean (.mode()). */
int mgx_diag_gaussian_nhwc(const uint16_t* moments, long ld, const uint16_t* noise, uint16_t* mean, uint16_t* std,
                           uint16_t* sample, int Cz, int H, int W, void* stream);

/* ---- low-rank adapters (csrc/lora.hip).  A target Linear y = x (W0 + s B A)^T + b with A [r, K], B [N, r]; B is held
 * transposed (Bt [r, N]) so that both adapter halves are "r rows x wide" and each kernel serves both.  r in {16, 32, 64, 128},
 * Kin % 64 == 0, any M >= 1; everything else is refused.  No atomics: every result is bit-reproducible.
 *
 * Out[M, r] = bf16(scale * In[M, Kin] P[r, Kin]^T): bf16 MFMA, fp32 accumulation, ONE rounding.  Row m of In sits at
 * (m / in_rpb) * in_bstride + (m % in_rpb) * ld_in elements (as in mgx_transpose_bf16); Out and P are plain matrices. */
int mgx_lora_proj(const uint16_t* in, const uint16_t* P, uint16_t* out, long M, int Kin, int r, long ld_in, long in_rpb,
                  long in_bstride, float scale, void* stream);
/* G[r, Kin] = beta * G + Small[M, r]^T Big[M, Kin], fp32 (beta == 0: G is not read).  Small is a plain [M, r] matrix, Big is
 * addressed like In above.  The rows are split over workgroups whose partial sums go to `workspace` (fp32,
 * mgx_lora_wgrad_workspace(M, Kin, r) elements; -1 for sizes the kernel refuses) and are added in a fixed order. */
long mgx_lora_wgrad_workspace(long M, int Kin, int r);
int mgx_lora_wgrad(const uint16_t* small, const uint16_t* big, float* G, float* workspace, long workspace_elems, long M, int Kin,
                   int r, long ld_big, long big_rpb, long big_bstride, float beta, void* stream);
/* W16[n, k] = bf16(W0[n, k] + s * sum_j Bt[j, n] A[j, k]): fp32 masters in, products and sums in fp64 (j ascending), ONE
 * rounding to bf16 (an fp32 sum misses bf16(exact) by several ulps where W0 and s B A cancel). */
int mgx_lora_merge(const float* W0, const float* Bt, const float* A, uint16_t* W16, int N, int K, int r, float s, void* stream);

/* ---- CLIP ViT image tower (csrc/clip.hip): the network behind the reference's HPSClipRewardModel, PickScoreRewardModel and
 * CLIPScoreRewardModel (fastvideo/models/reward_model/{hps_score,pick_score,clip_score}.py), inference only.  Its Linears are
 * mgx_gemm_bf16 launches; these entry points are what sits between them.
 *
 * Decoded image -> normalised patch rows: what `self.img_processor(image)` (hps_score.py:68), `self.processor(images=[image])`
 * (pick_score.py:55-61) and `self.preprocess(image)` (clip_score.py:57) do on a PIL image on the host.
 *   image [3][H][W] bf16 in about [-1, 1] (AutoencoderKL.decode's output);
 *   1. levels 0..255 as VaeImageProcessor.postprocess gives them under bf16: bf16(bf16(x / 2) + 0.5) clamped to [0, 1], times 255
 *      in fp32, rounded half to even;
 *   2. antialiased bicubic resize (PIL's BICUBIC: Keys a = -1/2, support 2 max(in / out, 1)) of the shortest edge to R, the long
 *      edge to floor(R long / short); horizontal then vertical pass with no rounding in between (PIL rounds to uint8 there),
 *      weights in fp64, the intermediate image in fp32; rounded to the nearest level and clamped to 0..255;
 *   3. centre crop R x R (top / left = floor of half the excess);  4. bf16((q / 255 - mean[c]) / std[c]), evaluated in fp32;
 *   5. patches[py (R / p) + px][c p p + dy p + dx], Kp >= 3 p p columns per row, the columns from 3 p p on written as zero.
 * mean, std: three floats each in HOST memory.  levels (optional, device): receives the R x R levels [3][R][R] as bytes.
 * workspace: fp32, mgx_clip_preprocess_workspace(H, W, R) elements (-1 for sizes below 1).  H, W >= 1, R % p == 0. */
long mgx_clip_preprocess_workspace(int H, int W, int R);
int mgx_clip_preprocess(const uint16_t* image, int H, int W, int R, int p, const float* mean, const float* std,
                        uint16_t* patches, int Kp, uint8_t* levels, float* workspace, long workspace_elems, void* stream);
/* x[b][0] = bf16(cls + pos[0]), x[b][1 + i] = bf16(patch_out[b][i] + pos[1 + i]): the class token, the patch embeddings
 * [B (S - 1)][width] bf16 and the position embeddings [S][width] (cls, pos fp32) -- CLIPVisionEmbeddings.forward / open_clip's
 * VisionTransformer.forward up to ln_pre, inside `self.reward_model(image, text)` (hps_score.py:71). */
int mgx_vit_embed(const uint16_t* patch_out, const float* cls, const float* pos, uint16_t* x, int B, int S, int width,
                  void* stream);
/* y[m][0..D) = bf16(LayerNorm(x[m][0..D); eps) * gamma + beta), rows ldx / ldy elements apart (y may be x): the nn.LayerNorm
 * layers of the tower (ln_pre, ln_1, ln_2, ln_post; same call sites).  fp32 statistics, the variance from centred values;
 * gamma, beta fp32 [D].  D % 64 == 0, D <= 2048. */
int mgx_layer_norm_affine(const uint16_t* x, long ldx, const float* gamma, const float* beta, uint16_t* y, long ldy, long M, int D,
                          float eps, void* stream);
/* Non-causal multi-head attention of the tower's nn.MultiheadAttention / CLIPAttention (same call sites), straight from the
 * packed projection: row b S + s of qkv [B S][ld_qkv] holds q | k | v, head h in the columns h d, width + h d and 2 width + h d
 * (width = H d); O[b S + s][h d ..] = bf16(softmax(scale q k^T) v), ldo elements between rows.  bf16 MFMA, fp32 scores and
 * accumulation, one rounding of O; no lse.  d % 16 == 0, d <= 128; any S >= 1, tail queries and keys masked in the kernel:
 * nothing outside the rows [0, B S) and the head columns is read or written.  ld_qkv % 8 == 0, ldo % 4 == 0, both pointers
 * 16-byte aligned.  Returns 1 -- nothing launched -- for S > 4096. */
int mgx_vit_attn_fwd(const uint16_t* qkv, long ld_qkv, uint16_t* O, long ldo, int B, int H, int S, int d, float scale,
                     void* stream);
/* y[m][0..N) = bf16(act(x[m][0..N))), y may be x.  act 0: exact GELU x Phi(x) (nn.GELU(): open_clip ViT-H, HF hidden_act "gelu"),
 * act 1: QuickGELU x sigmoid(1.702 x) (OpenAI weights) -- the tower's MLP activation (same call sites); mgx_gemm_bf16's GELU
 * epilogue is the tanh form, which these networks do not use. */
int mgx_act_rows(const uint16_t* x, long ldx, uint16_t* y, long ldy, long M, int N, int act, void* stream);
/* out[b][0..n) (fp32) = f[b] / |f[b]|, f bf16: `image_embs / torch.norm(image_embs, dim=-1, keepdim=True)` (pick_score.py:75),
 * F.normalize (clip_score.py:65). */
int mgx_l2_normalize_rows(const uint16_t* f, long ldf, float* out, int B, int n, void* stream);
/* out[b] = (logit_scale <f[b], t[b]> / (|f[b]| |t[b]|) - mean) / std, fp32 sums; f and t rows of bf16 or fp32 (`*_is_f32`), ldt
 * may be 0 (one text row for every image).  The score of pick_score.py:73-82 (logit_scale = exp(model.logit_scale)), and with
 * logit_scale 1, mean 0, std 1 the cosine of hps_score.py:70-77 and clip_score.py:63-70. */
int mgx_cosine_score(const void* f, int f_is_f32, long ldf, const void* t, int t_is_f32, long ldt, float* out, int B, int n,
                     float logit_scale, float mean, float std, void* stream);

/* ---- Text encoders (csrc/text.hip): the CLIP text tower inside `self.reward_model(image, text)` (hps_score.py:69-72),
 * `self.model.get_text_features` (pick_score.py:64-77) and `encode_text` (clip_score.py), and the T5-XXL + CLIP-L prompt
 * encoders behind `pipe.encode_prompt` (fastvideo/data_preprocess/preprocess_flux_embedding.py:89).  Inference only; the Linears
 * are mgx_gemm_bf16 launches.
 *
 * mgx_vit_attn_fwd's contract and kernel (csrc/encoder_attn.hip: packed q | k | v rows, bf16 MFMA, fp32 scores and sums, one
 * rounding of O, nothing read or written outside the rows and the head columns, d % 16 == 0, d <= 128, returns 1 for S > 4096),
 * plus:
 *   causal != 0: key k contributes to query q only if k <= q (CLIPTextTransformer's causal mask / open_clip's attn_mask); key
 *                blocks wholly above a workgroup's last query are neither loaded nor multiplied;
 *   rel_bias (device fp32 [H][2 S - 1], or NULL): rel_bias[h][k - q + S - 1] is added to scale * q.k in fp32 before the maximum
 *                is taken -- T5Attention's position_bias, which depends on (h, k - q) only, as a compact table.
 * T5 calls it with scale 1, causal 0 and a table, CLIP text with scale d^-0.5, causal 1 and NULL.  With causal 0 and NULL the
 * result equals mgx_vit_attn_fwd's bit for bit. */
int mgx_text_attn_fwd(const uint16_t* qkv, long ld_qkv, uint16_t* O, long ldo, int B, int H, int S, int d, float scale, int causal,
                      const float* rel_bias, void* stream);
/* T5LayerNorm (transformers modeling_t5.py, every layer_norm / final_layer_norm under `pipe.encode_prompt`):
 * y[m][0..D) = bf16(x * rsqrt(mean(x^2) + eps) * gamma), no mean subtraction, no bias; fp32 statistics, gamma fp32 [D], ONE
 * rounding.  STATED DEVIATION: transformers under bf16 rounds twice, once after the normalisation (the cast back to the
 * weight's dtype) and once after the weight.  D % 64 == 0, D <= 4096; rows ldx / ldy elements apart, y may be x. */
int mgx_rms_norm_affine(const uint16_t* x, long ldx, const float* gamma, uint16_t* y, long ldy, long M, int D, float eps,
                        void* stream);
/* y[m][0..N) = bf16(act(a[m][0..N)) * b[m][0..N)), y may be a: T5DenseGatedActDense's `self.act(self.wi_0(x)) * self.wi_1(x)`
 * (same call site); a and b are the two column halves of the fused wi_0 | wi_1 GEMM's output.  act 0, 1: as mgx_act_rows;
 * act 2: the tanh GELU 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) -- `gelu_new`, what feed_forward_proj "gated-gelu"
 * resolves to -- evaluated through exp(-2 |u|), which neither cancels for negative x nor overflows. */
int mgx_gated_act_rows(const uint16_t* a, long lda, const uint16_t* b, long ldb, uint16_t* y, long ldy, long M, int N, int act,
                       void* stream);
/* x[m][0..D) = bf16(table[ids[m]] + pos[m % S]): nn.Embedding of the token ids plus the position embeddings
 * (CLIPTextEmbeddings.forward; T5Stack's embed_tokens with pos == NULL; same call sites).  ids int32 [M] on the device, table
 * bf16 [V][D], pos fp32 [S][D] or NULL.  Contract: 0 <= ids[m] < V (the Python wrapper checks it on the host before the copy;
 * the kernel reads row 0 for an id outside, never memory outside the table). */
int mgx_token_embed(const int* ids, const uint16_t* table, const float* pos, uint16_t* x, long M, int S, int D, int V,
                    void* stream);

/* ---- ImageReward scorer (csrc/blip.hip): the network behind the reference's ImageRewardModel
 * (fastvideo/models/reward_model/image_reward.py:24-40; `self.model.inference_rank(text, [image])` :38): a BLIP ViT image
 * encoder, a BERT text encoder whose layers cross-attend to the image tokens, an MLP head.  Inference only; the Linears are
 * mgx_gemm_bf16 launches, LayerNorm, GELU and the embeddings the entry points above.
 *
 * Attention with separate operands and a key length per sample (image_reward.py:38: BertSelfAttention inside inference_rank,
 * once over the padded prompt with its attention_mask, once over the image tokens as encoder_hidden_states).  Row b Sq + s of
 * q [B Sq][ldq] holds head h in the columns h d, rows b Skv + t of k [B Skv][ldk] and v [B Skv][ldv] likewise;
 * O[b Sq + s][h d ..] = bf16(softmax(scale q k^T over the keys t < kv_len[b]) v), ldo elements between rows.  kv_len: device
 * int32 [B], or NULL: all Skv keys count.  mgx_vit_attn_fwd's kernel (csrc/encoder_attn.hip) and arithmetic: bf16 MFMA, fp32
 * scores and sums, one rounding of O, no lse.  Excluded keys are excluded exactly (BERT's additive -10000 / finfo.min gives them a weight that underflows to 0):
 * the k and v rows at or beyond kv_len[b] may hold anything, inf and NaN included -- they are not read, and key blocks wholly
 * beyond kv_len[b] are neither loaded nor multiplied.  Contract: 1 <= kv_len[b] <= Skv (the Python wrapper checks it on the
 * host before the copy); the kernel clamps into that range, so it never reads outside the rows [0, B Skv) and no query meets an
 * empty key set.  d % 16 == 0, d <= 128; any Sq, Skv >= 1; every row stride a multiple of 8 elements, all four pointers 16-byte
 * aligned; nothing outside the B Sq rows and the head columns of O is written.  q, k and v may point into one packed buffer.
 * Returns 1 -- nothing launched -- for Sq > 4096 or Skv > 4096. */
int mgx_xattn_fwd(const uint16_t* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv, uint16_t* O, long ldo,
                  int B, int H, int Sq, int Skv, int d, float scale, const int* kv_len, void* stream);
/* out[m][0..N) (fp32) = x[m][0..K) W[N][K]^T + bias, then, if affine != 0, (. - shift) / scale: the Linears of ImageReward's
 * score head `self.mlp` and its `(rewards - self.mean) / self.std` (inside inference_rank, image_reward.py:38), applied layer by
 * layer with fp32 intermediates.  x rows of bf16 or fp32 (`x_is_f32`), ldx elements apart (ldx % 4 == 0); W, bias (or NULL) and
 * out fp32, out rows ldo apart.  fp32 products and sums.  Any M, N >= 1; K % 4 == 0. */
int mgx_linear_rows_f32(const void* x, int x_is_f32, long ldx, const float* W, const float* bias, float* out, long ldo, int M,
                        int N, int K, int affine, float shift, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
