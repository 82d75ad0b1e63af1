"""Plain fp64 references of the VAE kernels (csrc/vae.hip, the implicit convolution of csrc/gemm.hip) and of the mid-block
attention that mixgrpo_amd/vae.py sequences from them.  Device-agnostic torch: tests/test_vae_refs.py checks them on the CPU
against torch's own operators, tests/test_hip_vae_kernels.py holds the kernels to them on the GPU.  Nothing here calls the
library."""
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def ulp_bf16(v):
    """Spacing of the bf16 values around |v| (fp64 tensor): 2^(floor(log2 |v|) - 7), from the smallest normal binade on."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def ordinal(t):
    """bf16 tensor -> integers in which neighbouring bf16 values differ by one (+0 and -0 both 0)"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def random_bits(shape, gen, device="cpu"):
    """Uniformly random 16-bit patterns as bf16 (NaN payloads, +-0, denormals), as tests/test_hip_wgrad_operands.py uses
    them: a copy kernel must move each of them unchanged.  Compare such tensors through `.view(torch.int16)`."""
    i = torch.randint(0, 1 << 16, shape, generator=gen) - (1 << 15)
    return i.to(torch.int16).view(BF16).to(device)


# ------------------------------------------------------------------------------------------------------------ convolution
def im2col_rows(xpad, H, W, stride, y0, y1):
    """Rows y0 .. y1 of the output image as GEMM rows [(y1 - y0) Wo, 9 C]: nine shifted slices of the zero-bordered NHWC image
    xpad [(H + 2), (W + 2), C], tap-major, channels contiguous (the layout of the weight [Cout, 3, 3, C]).
    stride 1: output pixel (y, x) reads padded pixels (y + ky, x + kx) -- zero padding 1.
    stride 2: output pixel (y, x) reads padded pixels (1 + 2 y + ky, 1 + 2 x + kx) -- F.pad(x, (0, 1, 0, 1)), no padding."""
    C = xpad.shape[-1]
    if stride == 1:
        taps = [xpad[ky + y0:ky + y1, kx:kx + W] for ky in range(3) for kx in range(3)]
    else:
        assert stride == 2 and H % 2 == 0 and W % 2 == 0
        taps = [xpad[1 + ky + 2 * y0:1 + ky + 2 * y1:2, 1 + kx:1 + kx + W:2] for ky in range(3) for kx in range(3)]
    return torch.cat([t.reshape(-1, C) for t in taps], dim=1)


def conv3x3_ref(xpad, wt, bias, H, W, stride=1, chunk_rows=8192):
    """fp64 [Ho Wo, Cout] = im2col(xpad) @ wt[Cout, 9 C]^T + bias, by an fp64 matmul on xpad's device in chunks of image rows.
    (Not F.conv2d on the GPU: a Winograd or FFT path does not add the products it is given.)"""
    Cout = wt.shape[0]
    Ho, Wo = (H, W) if stride == 1 else (H // 2, W // 2)
    w64 = wt.reshape(Cout, -1).to(F64).t().contiguous()
    out = torch.empty(Ho * Wo, Cout, dtype=F64, device=xpad.device)
    step = max(1, chunk_rows // Wo)
    for y0 in range(0, Ho, step):
        y1 = min(Ho, y0 + step)
        out[y0 * Wo:y1 * Wo] = im2col_rows(xpad, H, W, stride, y0, y1).to(F64) @ w64
    return out + bias[:Cout].to(F64)


def conv3x3_ref_bf16(xpad, wt, bias, H, W, stride=1, res=None):
    """What the kernels store: bf16(conv + bias), and with `res` the residual form bf16(res + bf16(conv + bias)).  (fp64 -> fp32
    -> bf16: the callers' exact-grid sums are fp32 values, so the first step rounds nothing.)"""
    y = conv3x3_ref(xpad, wt, bias, H, W, stride).to(F32).to(BF16)
    if res is None:
        return y
    return (res.to(F64) + y.to(F64)).to(F32).to(BF16)


# -------------------------------------------------------------------------------------------------------------- GroupNorm
def group_norm_ref(x, gamma, beta, G, silu, eps=1e-6):
    """x [M, C] bf16 (one image, NHWC rows) -> (ref, bound), both fp64 [M, C].
    ref = [silu]((x - mean_g) / sqrt(var_g + eps) * gamma + beta) with the biased variance of group g over its M * C / G elements.
    bound = ulp_bf16(ref) + 2^-20 ((|x| + |mean|) rstd |gamma| + |beta|): see tests/test_hip_vae_kernels.py."""
    M, C = x.shape
    xd = x.to(F64).view(M, G, C // G)
    mean = xd.mean((0, 2), keepdim=True)
    var = ((xd - mean) ** 2).mean((0, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga, be = gamma.to(F64), beta.to(F64)
    t = ((xd - mean) * rstd).view(M, C) * ga + be
    ref = t * torch.sigmoid(t) if silu else t
    big = ((xd.abs() + mean.abs()) * rstd).view(M, C) * ga.abs() + be.abs()
    return ref, ulp_bf16(ref) + 2.0 ** -20 * big


# ---------------------------------------------------------------------------------------------------------------- softmax
def softmax_ref(S, scale):
    """fp64 softmax over the rows of float32(scale) * S, S fp32 [M, n] (-inf entries give exact zeros)."""
    s32 = torch.tensor(scale, dtype=F32).to(F64).item()
    return torch.softmax(S.to(F64) * s32, dim=-1)


def softmax_bound(ref):
    return ulp_bf16(ref) + 2.0 ** -120


# ------------------------------------------------------------------------------------------------- mid-block attention
def attention_ref(x, P, C, G, rounded, eps=1e-6):
    """AutoencoderKL._attention restated on x [M, C] bf16 with the weights P = {group_norm.weight/.bias [C], qkv.weight
    [3 C, C], qkv.bias [3 C], to_out.0.weight [C, C], to_out.0.bias [C]} (bf16), in fp64.  `rounded`: a bf16 rounding at each
    point where the host code stores bf16 -- the normalised activation, q | k | v, the probabilities, P v, the projection and the
    residual sum -- and S = q k^T in fp32; otherwise no rounding anywhere (returns fp64)."""
    r16 = (lambda t: t.to(F32).to(BF16).to(F64)) if rounded else (lambda t: t)
    r32 = (lambda t: t.to(F32).to(F64)) if rounded else (lambda t: t)
    w = {k: v.to(F64) for k, v in P.items()}
    n = r16(group_norm_ref(x, P["group_norm.weight"], P["group_norm.bias"], G, False, eps)[0])
    qkv = r16(n @ w["qkv.weight"].t() + w["qkv.bias"])
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    S = r32(q @ k.t())
    scale = torch.tensor(float(C) ** -0.5, dtype=F32).to(F64).item() if rounded else float(C) ** -0.5
    p = r16(torch.softmax(S * scale, dim=-1))
    o = r16(p @ v)
    y = r16(o @ w["to_out.0.weight"].t() + w["to_out.0.bias"])
    out = r16(x.to(F64) + y)
    return out.to(BF16) if rounded else out


def attention_weights(C, seed):
    """Random bf16 weights of one attention block, on the host."""
    g = torch.Generator().manual_seed(seed)
    P = {"group_norm.weight": 1.0 + 0.1 * torch.randn(C, generator=g), "group_norm.bias": 0.05 * torch.randn(C, generator=g)}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        P[n + ".weight"] = torch.randn(C, C, generator=g) / C ** 0.5
        P[n + ".bias"] = 0.05 * torch.randn(C, generator=g)
    P = {k: v.to(BF16) for k, v in P.items()}
    P["qkv.weight"] = torch.cat([P[f"to_{n}.weight"] for n in "qkv"], 0).contiguous()
    P["qkv.bias"] = torch.cat([P[f"to_{n}.bias"] for n in "qkv"], 0).contiguous()
    return P


def rel_l2(a, b):
    return ((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm().clamp_min(1e-30)).item()
