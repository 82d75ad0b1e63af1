"""HIP VAE encoder (mixgrpo_amd/vae.py `encode`, csrc/vae.hip, the stride-2 entry of csrc/gemm.hip's implicit convolution) and
the image-to-image path of the sampler, against the CPU restatement in tests/vae_encoder_ref.py (parity unpinned against
diffusers, like the decoder oracle it is built on).  Bounds: single kernels as their stride-1 / decoder counterparts in
tests/test_hip_vae.py; whole encoders the decoder tests' own bounds (same kernels, same rounding points, fewer layers)."""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_encoder_ref as ER
from oracle import vae as OV

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to vae_encode.json in that directory


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _record(**kw):
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "vae_encode.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d.update(kw)
    json.dump(d, open(path, "w"), indent=1)


def _ord(t):
    """bf16 tensor -> integers in which neighbouring bf16 values differ by one"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


# ---------------------------------------------------------------------------------------------------------- single kernels
@pytest.mark.parametrize("H,W,C,Cout", [(2, 2, 64, 4),            # one output pixel: every tap but those of row / column 0 on the border
                                         (24, 24, 64, 64),         # one tile
                                         (40, 72, 128, 128),       # 720 rows: image rows straddle the 256-row tiles
                                         (256, 256, 128, 512)])    # 128 tiles of 256 x 256: the persistent kernel
def test_conv3x3_stride2_vs_torch(H, W, C, Cout):
    from mixgrpo_amd import ops
    g = torch.Generator().manual_seed(H + C)
    x = torch.randn(C, H, W, generator=g).to(BF16)
    w = (torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(BF16)
    b = (0.1 * torch.randn(Cout, generator=g)).to(BF16)
    want = F.conv2d(F.pad(x.float()[None], (0, 1, 0, 1)), w.float(), b.float(), stride=2)[0]      # [Cout, H/2, W/2] fp32
    assert want.shape == (Cout, H // 2, W // 2)
    xp = torch.zeros(H + 2, W + 2, C, dtype=BF16, device="cuda")
    xp[1:-1, 1:-1] = x.permute(1, 2, 0).cuda()
    xp[0, 0, 0] = float("inf")                      # the top / left border is never read: no output may see this
    wt = w.permute(0, 2, 3, 1).contiguous().cuda()
    bias = torch.zeros(Cout + 8, dtype=BF16, device="cuda")
    bias[:Cout] = b.cuda()
    ld = max(Cout, 8)
    M = (H // 2) * (W // 2)
    out = torch.zeros(M, ld, dtype=BF16, device="cuda")
    ops.conv3x3s2(xp, wt, bias, out, H, W, C, Cout, ld_out=ld)
    got = out[:, :Cout].float().cpu().view(H // 2, W // 2, Cout).permute(2, 0, 1)
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    same = (got == want.to(BF16).float()).float().mean().item()
    print(f"conv3x3s2 {H}x{W}x{C}->{Cout}: max err {err:.3e} (bound {2.0 ** -8 * want.abs().max().item() + 1e-6:.3e}), bit-equal {same:.4f}")
    assert err <= 2.0 ** -8 * want.abs().max().item() + 1e-6
    assert same > 0.97                                                                    # bit-identical almost everywhere
    if ld > Cout:
        assert out[:, Cout:].abs().sum().item() == 0                                      # nothing past the output channels


@pytest.mark.parametrize("H,W", [(5, 7), (64, 64)])
@pytest.mark.parametrize("C,ld", [(64, 64), (64, 96)])
def test_pad_nhwc_copies_the_interior_and_keeps_the_border(H, W, C, ld):
    from mixgrpo_amd import ops
    x = torch.randn(H * W, ld, generator=torch.Generator().manual_seed(H + ld)).to(BF16).cuda()
    out = torch.zeros(H + 2, W + 2, C, dtype=BF16, device="cuda")
    ops.pad_nhwc(x, ld, out, H, W, C)
    assert torch.equal(out[1:-1, 1:-1], x[:, :C].reshape(H, W, C))
    assert out[0].abs().sum().item() == 0 and out[-1].abs().sum().item() == 0
    assert out[:, 0].abs().sum().item() == 0 and out[:, -1].abs().sum().item() == 0


@pytest.mark.parametrize("H,W,ld", [(9, 5, 32), (32, 32, 40)])
def test_diag_gaussian_vs_torch_on_bf16(H, W, ld):
    """mean is a copy.  std = bf16(exp(.)) may differ from the host's by one bf16 ulp where the two `exp` differ in the last
    fp32 bit in front of the rounding; a one-ulp std moves bf16(std * noise) by at most one ulp of that product and so the
    sum by at most one ulp at the magnitude of its larger term."""
    from mixgrpo_amd import ops
    Cz = 16
    g = torch.Generator().manual_seed(H)
    mom = torch.randn(H * W, ld, generator=g)
    mom[:, Cz:2 * Cz] *= 4.0
    for i, v in enumerate((-40.0, -30.0, 0.0, 20.0, 25.0)):
        mom[i::7, Cz + i] = v
        mom[3 + i, 2 * Cz - 1 - i] = v
    mom = mom.to(BF16)
    noise = torch.randn(Cz, H, W, generator=g).to(BF16)
    nchw = mom[:, :2 * Cz].reshape(H, W, 2 * Cz).permute(2, 0, 1).contiguous()
    w_mean, w_std, w_sample = ER.gaussian(nchw, noise)
    mean, std, sample = (torch.full((Cz, H, W), 7.0, dtype=BF16, device="cuda") for _ in range(3))
    ops.diag_gaussian(mom.cuda(), ld, noise.cuda(), mean, std, sample, Cz, H, W)
    mean, std, sample = mean.cpu(), std.cpu(), sample.cpu()
    assert torch.equal(mean, w_mean)
    assert torch.isfinite(std).all() and torch.isfinite(sample).all()
    d_std = (_ord(std) - _ord(w_std)).abs().max().item()
    prod = (w_std.float() * noise.float()).abs()
    ulp = 2.0 ** (torch.floor(torch.log2(torch.maximum(torch.maximum(prod, w_sample.float().abs()), torch.tensor(1e-30)))) - 7)
    d_sample = ((sample.float() - w_sample.float()).abs() / ulp).max().item()
    print(f"diag_gaussian {H}x{W}: std within {d_std} ulp, differing {(_ord(std) != _ord(w_std)).float().mean().item():.5f}; "
          f"sample within {d_sample:.3f} ulp")
    assert d_std <= 1
    assert d_sample <= 1.0
    flat = std.view(Cz, -1)                                                               # the clamp: -40 as -30, 25 as 20
    assert (flat[0, 0::7] == flat[1, 1]).all() and (flat[4, 4::7] == flat[3, 3]).all() and flat[2, 2].item() == 1.0
    assert abs(flat[3, 3].item() / np.exp(10.0) - 1) < 2.0 ** -7 and abs(flat[1, 1].item() / np.exp(-15.0) - 1) < 2.0 ** -7
    m2, s2, mode = (torch.empty(Cz, H, W, dtype=BF16, device="cuda") for _ in range(3))
    ops.diag_gaussian(mom.cuda(), ld, None, m2, s2, mode, Cz, H, W)
    assert torch.equal(mode.cpu(), w_mean) and torch.equal(m2.cpu(), w_mean) and torch.equal(s2.cpu(), std)


# ---------------------------------------------------------------------------------------------------------- whole encoders
def _model(cfg_kw, seed):
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    ocfg = OV.VaeConfig(**cfg_kw)
    P = {**OV.init_params(ocfg, seed=seed), **ER.init_params(ocfg, seed=seed + 1)}
    m = AutoencoderKL(VaeConfig(**cfg_kw), device="cuda").load_state_dict({k: v.to(BF16) for k, v in P.items()})
    assert m.has_encoder
    return ocfg, P, m


SMALL = dict(block_out_channels=(64, 128, 128), layers_per_block=1, sample_size=64)       # 4x; tile 64 px / 16 latent


@functools.lru_cache(maxsize=None)
def _small():
    return _model(SMALL, seed=3)


def test_small_encoder_vs_helper():
    ocfg, P, m = _small()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 64, 64, generator=g).clamp(-1, 1)
    want = ER.encoder(P, ocfg, x)
    dist = m.encode(x.cuda()).latent_dist
    got = dist.parameters
    assert got.shape == (2, 32, 16, 16) and got.dtype == BF16
    r1 = _rel(got.float().cpu(), want)
    x2 = torch.randn(1, 3, 40, 72, generator=g).clamp(-1, 1)                               # 10 x 18 latent: 180 attention tokens
    want2 = ER.encoder(P, ocfg, x2)
    got2 = m.encode(x2.cuda(), return_dict=False)[0].parameters
    assert got2.shape == (1, 32, 10, 18)
    r2 = _rel(got2.float().cpu(), want2)
    print(f"small encoder moments rel-L2: {r1:.3e} (2x3x64x64), {r2:.3e} (3x40x72)")
    _record(small_rel_l2_64=r1, small_rel_l2_40x72=r2)
    assert r1 < 2e-2 and r2 < 2e-2
    # the distribution's surface
    assert torch.equal(dist.mean, got[:, :16]) and torch.equal(dist.mode(), dist.mean)
    assert torch.equal(dist.logvar, got[:, 16:].clamp(-30.0, 20.0)) and torch.equal(dist.var, torch.exp(dist.logvar))
    w_mean, w_std, _ = ER.gaussian(got.cpu())
    assert (_ord(dist.std.cpu()) - _ord(w_std)).abs().max().item() <= 1
    gen = torch.Generator().manual_seed(5)
    s = dist.sample(generator=gen)
    noise = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(5), dtype=BF16)
    want_s = (dist.mean.cpu().float() + (dist.std.cpu().float() * noise.float()).to(BF16).float()).to(BF16)
    assert s.shape == (2, 16, 16, 16) and torch.equal(s.cpu(), want_s)
    assert dist.sample().shape == (2, 16, 16, 16)
    with pytest.raises(ValueError):
        m.encode(torch.zeros(1, 3, 30, 64).cuda())                                        # sides must be multiples of 4 here


def test_flux_encoder_256_vs_helper():
    ocfg, P, m = _model({}, seed=5)
    x = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(6)).clamp(-1, 1)
    want = ER.encoder(P, ocfg, x)
    got = m.encode(x.cuda()).latent_dist.parameters
    assert got.shape == (1, 32, 32, 32)
    r = _rel(got.float().cpu(), want)
    print(f"FLUX encoder 256x256 moments rel-L2: {r:.3e}")
    _record(flux_256_rel_l2=r, flux_256_max_abs=(got.float().cpu() - want).abs().max().item(),
            flux_256_moments_abs_mean=want.abs().mean().item())
    assert r < 3e-2, r


def test_tiled_encode_vs_helper():
    ocfg, P, m = _small()
    x = torch.randn(1, 3, 80, 112, generator=torch.Generator().manual_seed(12)).clamp(-1, 1)      # 2 x 3 tiles, ragged edges
    want = ER.encode_moments(P, ocfg, x, use_tiling=True)
    assert want.shape == (1, 32, 20, 28)
    m.enable_tiling()
    try:
        got = m.encode(x.cuda()).latent_dist.parameters
        direct = m.tiled_encode(x.cuda()).latent_dist.parameters
    finally:
        m.disable_tiling()
    assert got.shape == want.shape and torch.equal(got, direct)
    r = _rel(got.float().cpu(), want.float())
    print(f"tiled encode rel-L2: {r:.3e}")
    _record(small_tiled_rel_l2=r)
    assert r < 2e-2
    whole = m.encode(x.cuda()).latent_dist.parameters                                      # tiling off
    assert whole.shape == got.shape and not torch.equal(whole, got)
    per_image = m._encoder(x[0].cuda().float()).view(20, 28, 32).permute(2, 0, 1)
    assert torch.equal(whole[0], per_image)
    m.enable_tiling()                                                                      # within one tile: not tiled
    try:
        x1 = x[..., :64, :64].cuda()
        one = m.encode(x1).latent_dist.parameters
    finally:
        m.disable_tiling()
    assert torch.equal(one, m.encode(x1).latent_dist.parameters)


def test_flux_encode_1024_runs():
    """The headline shape: a 1024^2 image is exactly one tile (16384 mid-block tokens, the attention's limit)."""
    from mixgrpo_amd.vae import AutoencoderKL
    m = AutoencoderKL(device="cuda").init_synthetic(seed=1)
    m.enable_tiling()
    x = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(2)).clamp(-1, 1).cuda()
    got = m.encode(x).latent_dist.parameters
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        m.encode(x)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    print(f"encode 1024x1024: {ms:.1f} ms")
    _record(encode_1024_ms=ms)
    assert got.shape == (1, 32, 128, 128) and torch.isfinite(got.float()).all()


def test_round_trip_shapes():
    _, _, m = _small()
    z = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(4)).cuda()
    img = m.decode(z, return_dict=False)[0]
    back = m.encode(img).latent_dist
    assert img.shape == (2, 3, 64, 64) and back.mean.shape == z.shape and back.sample().shape == z.shape
    assert torch.isfinite(back.mean.float()).all()


# ---------------------------------------------------------------------------------------------------------- sampler
FLUX_TOY = dict(num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=4, joint_attention_dim=64,
                pooled_projection_dim=32)


class _Counting:
    def __init__(self, model):
        self.model, self.calls, self.store, self.cfg = model, 0, model.store, model.cfg

    def __call__(self, *a, **k):
        self.calls += 1
        return self.model(*a, **k)


def test_sampler_image_to_image():
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.sample_flux import DualFluxSampler, calculate_shift, flow_match_sigmas
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    from oracle import mmdit as OM

    def transformer(seed):
        P = OM.init_params(OM.FluxConfig(**FLUX_TOY), seed=seed, std=0.05, bias_std=0.05)
        t = FluxTransformer2DModel(FluxConfig(**FLUX_TOY), device="cuda")
        t.load_state_dict({k: v.cuda() for k, v in P.items()})
        return t.eval()

    vkw = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1, sample_size=256)      # 8x, like the FLUX VAE
    ocfg, VP, vae = _model(vkw, seed=4)
    base, new = _Counting(transformer(1)), _Counting(transformer(2))
    s = DualFluxSampler(base, new, vae=vae)
    g = torch.Generator().manual_seed(0)
    B, L, hw, N = 2, 24, 128, 8
    ehs = torch.randn(B, L, 64, generator=g).bfloat16().cuda()
    pooled = torch.randn(B, 32, generator=g).bfloat16().cuda()
    image = torch.randn(B, 3, hw, hw, generator=g).clamp(-1, 1)
    # encode_image: the helper's posterior sample with the same noise, normalised in bf16 and packed
    x0 = s.encode_image(image.cuda(), generator=torch.Generator().manual_seed(21))
    noise_p = torch.randn(B, 16, 16, 16, generator=torch.Generator().manual_seed(21), dtype=BF16)
    _, _, smp = ER.gaussian(ER.encoder(VP, ocfg, image), noise_p)
    want_x0 = ER.pack((smp - ocfg.shift_factor) * ocfg.scaling_factor)
    assert x0.shape == (B, 64, 64) and x0.dtype == BF16
    r = _rel(x0.float().cpu(), want_x0.float())
    print(f"encode_image rel-L2: {r:.3e}")
    _record(sampler_encode_image_rel_l2=r)
    assert r < 2e-2
    mode = s.encode_image(image.cuda(), sample_mode="argmax")
    assert torch.equal(mode, s.encode_image(image.cuda(), sample_mode="argmax")) and not torch.equal(mode, x0)
    # strength 0.5 of 8 steps: steps 4 .. 7 of the full schedule; mix_sampling_steps = 5 -> step 4 on the tuned model
    kw = dict(height=hw, width=hw, num_inference_steps=N, mix_sampling_steps=5)
    out = s(ehs, pooled, image=image.cuda(), strength=0.5, generator=torch.Generator().manual_seed(33), **kw)
    assert (new.calls, base.calls) == (1, 3)
    # the same run by hand: posterior noise first, then the initial noise, from one generator
    gen = torch.Generator().manual_seed(33)
    x0 = s.encode_image(image.cuda(), generator=gen)
    z = torch.randn(B, 16, 16, 16, generator=gen, dtype=BF16).cuda()
    noise = z.view(B, 16, 8, 2, 8, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, 64, 64)
    sig, _ = flow_match_sigmas(N, calculate_shift(64))
    s0 = sig[4].to(device="cuda", dtype=BF16)
    init = s0 * noise + (1.0 - s0) * x0
    tail = np.linspace(1.0, 1 / N, N)[4:]
    by_hand = s(ehs, pooled, height=hw, width=hw, num_inference_steps=4, mix_sampling_steps=1, sigmas=tail, latents=init)
    assert torch.equal(out, by_hand)
    assert (new.calls, base.calls) == (2, 6)
    # image=None: nothing changes
    lat = torch.randn(B, 64, 64, generator=g).bfloat16().cuda()
    assert torch.equal(s(ehs, pooled, latents=lat, **kw), s(ehs, pooled, latents=lat, image=None, strength=1.0, **kw))
    # refusals
    for bad in (0.0, 1.5, 0.1):
        with pytest.raises(ValueError):
            s(ehs, pooled, image=image.cuda(), strength=bad, **kw)
    _, _, dec_only = _decoder_only(vkw)
    with pytest.raises(ValueError, match="encoder"):
        DualFluxSampler(base, new, vae=dec_only)(ehs, pooled, image=image.cuda(), strength=0.5, **kw)
    with pytest.raises(ValueError, match="encoder"):
        DualFluxSampler(base, new)(ehs, pooled, image=image.cuda(), strength=0.5, **kw)


def _decoder_only(cfg_kw):
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    ocfg = OV.VaeConfig(**cfg_kw)
    P = OV.init_params(ocfg, seed=4)
    m = AutoencoderKL(VaeConfig(**cfg_kw), device="cuda").load_state_dict({k: v.to(BF16) for k, v in P.items()})
    assert not m.has_encoder
    return ocfg, P, m
