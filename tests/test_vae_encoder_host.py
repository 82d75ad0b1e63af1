"""Host-side checks of the VAE encoder (mixgrpo_amd/vae.py `encode` / `tiled_encode`, mixgrpo_amd/sample_flux.py img2img): the key
inventory, decoder-only loading, the encode tiling against the helper's restatement of `spatial_tiled_encode`
(tests/vae_encoder_ref.py; autoencoder_kl_causal_3d.py:408-470), the img2img schedule arithmetic, and that the synthetic decoder
weights did not move.  No GPU: the models live on the CPU and `_encoder`, the only device call of the tiling, is a stand-in."""
import hashlib

import pytest
import torch

import vae_encoder_ref as ER
from oracle import vae as OV

BF16 = torch.bfloat16


def test_encoder_key_inventory_of_the_flux_vae():
    from mixgrpo_amd.vae import VaeConfig
    from mixgrpo_amd.vae_arch import param_shapes
    cfg = VaeConfig()
    shp = param_shapes(cfg, "encoder")
    keys = list(shp)
    wb = lambda names: [f"{n}.{p}" for n in names for p in ("weight", "bias")]
    block0 = wb(["encoder.down_blocks.0.resnets.0.norm1", "encoder.down_blocks.0.resnets.0.conv1",
                 "encoder.down_blocks.0.resnets.0.norm2", "encoder.down_blocks.0.resnets.0.conv2",
                 "encoder.down_blocks.0.resnets.1.norm1", "encoder.down_blocks.0.resnets.1.conv1",
                 "encoder.down_blocks.0.resnets.1.norm2", "encoder.down_blocks.0.resnets.1.conv2",
                 "encoder.down_blocks.0.downsamplers.0.conv"])
    mid = wb(["encoder.mid_block.resnets.0.norm1", "encoder.mid_block.resnets.0.conv1", "encoder.mid_block.resnets.0.norm2",
              "encoder.mid_block.resnets.0.conv2", "encoder.mid_block.attentions.0.group_norm",
              "encoder.mid_block.attentions.0.to_q", "encoder.mid_block.attentions.0.to_k", "encoder.mid_block.attentions.0.to_v",
              "encoder.mid_block.attentions.0.to_out.0", "encoder.mid_block.resnets.1.norm1", "encoder.mid_block.resnets.1.conv1",
              "encoder.mid_block.resnets.1.norm2", "encoder.mid_block.resnets.1.conv2"])
    head = wb(["encoder.conv_in", "encoder.conv_norm_out", "encoder.conv_out"])
    for k in block0 + mid + head:
        assert k in shp, k
    assert [k for k in keys if k.startswith("encoder.down_blocks.0.")] == block0           # nothing else in block 0, in order
    assert sorted(k for k in keys if k.startswith("encoder.mid_block.")) == sorted(mid)
    assert shp["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert shp["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert shp["encoder.down_blocks.2.resnets.0.conv_shortcut.weight"] == (512, 256, 1, 1)
    assert "encoder.down_blocks.3.resnets.0.conv_shortcut.weight" not in shp
    assert "encoder.down_blocks.2.downsamplers.0.conv.weight" in shp and "encoder.down_blocks.3.downsamplers.0.conv.weight" not in shp
    assert shp["encoder.mid_block.attentions.0.to_q.weight"] == (512, 512)
    assert shp["encoder.conv_out.weight"] == (32, 512, 3, 3) and shp["encoder.conv_out.bias"] == (32,)
    # conv_in 2; blocks 0 and 3: 2 resnets x 8 (+ 2 for block 0's downsampler); blocks 1 and 2: 8 + 10 (one shortcut) + 2;
    # mid block 8 + 10 + 8; norm_out 2; conv_out 2
    assert len(keys) == 2 + (16 + 2) + (18 + 2) + (18 + 2) + 16 + 26 + 2 + 2 == 106
    assert len(set(keys)) == len(keys) and not set(keys) & set(param_shapes(cfg, "decoder"))
    assert shp == ER.param_shapes(OV.VaeConfig())                                           # the helper's restatement
    n = sum(torch.Size(s).numel() for s in shp.values())
    assert 34_000_000 < n < 35_000_000                                                      # the FLUX VAE encoder: 34.2 M


@pytest.mark.parametrize("kw", [{}, dict(block_out_channels=(64, 128, 128), layers_per_block=1),
                                dict(block_out_channels=(64, 64), layers_per_block=1, mid_block_add_attention=False)])
def test_both_inventories_equal_the_restatements_in_order(kw):
    """Key by key and in order (the order `init_synthetic` draws in): the decoder's against oracle/vae.py, the encoder's
    against tests/vae_encoder_ref.py -- neither of which reads the product's layer list."""
    from mixgrpo_amd.vae import VaeConfig
    from mixgrpo_amd.vae_arch import param_shapes
    cfg, ocfg = VaeConfig(**kw), OV.VaeConfig(**kw)
    assert list(param_shapes(cfg, "decoder").items()) == list(OV.param_shapes(ocfg).items())
    assert list(param_shapes(cfg, "encoder").items()) == list(ER.param_shapes(ocfg).items())


SMALL = dict(block_out_channels=(64, 64), layers_per_block=1, sample_size=32)


def test_decoder_only_state_dicts_give_a_decoder_only_object():
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    dec = {k: v.to(BF16) for k, v in OV.init_params(OV.VaeConfig(**SMALL), seed=1).items()}
    enc = {k: v.to(BF16) for k, v in ER.init_params(OV.VaeConfig(**SMALL), seed=2).items()}
    stray = dict(dec)
    stray["encoder.conv_in.weight"] = enc["encoder.conv_in.weight"]
    for sd in (dec, stray):
        m = AutoencoderKL(VaeConfig(**SMALL), device="cpu").load_state_dict(sd)
        assert m.has_encoder is False and not any(k.startswith("encoder.") for k in m.P)
        with pytest.raises(RuntimeError, match="decoder-only"):
            m.encode(torch.zeros(1, 3, 32, 32))
    m = AutoencoderKL(VaeConfig(**SMALL), device="cpu").load_state_dict({**dec, **enc})
    assert m.has_encoder is True
    assert m.P["encoder.conv_in.weight"].shape == (64, 3, 3, 64)                            # 3 input channels padded to the tap width
    assert m.P["encoder.conv_out.weight"].shape == (32, 3, 3, 64)
    assert m.P["encoder.mid_block.attentions.0.qkv.weight"].shape == (192, 64)
    assert AutoencoderKL(VaeConfig(**SMALL), device="cpu").has_encoder is False
    # values other than the FLUX VAE's are refused at encode, not at construction
    for kw in (dict(in_channels=4), dict(use_quant_conv=True), dict(double_z=False)):
        m = AutoencoderKL(VaeConfig(**SMALL, **kw), device="cpu")
        with pytest.raises(ValueError):
            m.encode(torch.zeros(1, 3, 32, 32))


def _standin(x, f, Cm):
    """A recording stand-in's moments for an image tile [B, 3, H, W]: [B, Cm, H / f, W / f] bf16, a function of the pixels and
    of the row inside the tile (so a wrong tile origin, size or blend shows)."""
    p = torch.nn.functional.avg_pool2d(x.float(), f)                                        # [B, 3, h, w]
    rows = torch.arange(p.shape[-2], dtype=torch.float32).view(1, 1, -1, 1)
    c = torch.arange(Cm, dtype=torch.float32).view(1, -1, 1, 1)
    return (p.sum(1, keepdim=True) * (1 + c / 8) + rows / 4 - c / 16).to(BF16)


@pytest.mark.parametrize("H,W,calls", [(56, 80, [(32, 32), (32, 32), (32, 32), (32, 8), (32, 32), (32, 32), (32, 32), (32, 8),
                                                 (8, 32), (8, 32), (8, 32), (8, 8)]),                # ragged last row and column
                                       (40, 72, [(32, 32), (32, 32), (32, 24), (16, 32), (16, 32), (16, 24)])])   # 2 x 3 tiles
def test_tiled_encode_schedule_blend_and_crop_vs_the_helper(H, W, calls):
    """sample_size 32, two blocks (f = 2): image tiles of 32 with stride 24, latent tiles of 16 blended over 4 and cropped to 12."""
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    cfg = OV.VaeConfig(**SMALL)
    m = AutoencoderKL(VaeConfig(**SMALL), device="cpu").init_synthetic(seed=0)
    assert m.has_encoder and (m.tile_sample_min_size, m.tile_latent_min_size) == (32, 16)
    Cm, f = 2 * cfg.latent_channels, 2
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H))
    seen, seen_ref = [], []

    def enc_ref(t):
        seen_ref.append(tuple(t.shape[-2:]))
        return _standin(t, f, Cm)

    def enc_product(img):                                                                   # `_encoder`: [3, H, W] -> plain NHWC
        seen.append(tuple(img.shape[-2:]))
        return _standin(img[None], f, Cm)[0].permute(1, 2, 0).reshape(-1, Cm).contiguous()

    want = ER.tiled_moments(None, cfg, x, encode_tile=enc_ref)
    m._encoder = enc_product
    got = m.tiled_encode(x, return_moments=True)
    assert seen_ref == calls and seen == [c for c in calls for _ in range(2)]               # per tile, one call per image
    lat = lambda n: sum(min(12, (min(32, n - o)) // f) for o in range(0, n, 24))
    assert tuple(want.shape) == (2, Cm, lat(H), lat(W))
    assert got.dtype == BF16 and got.shape == want.shape and torch.equal(got, want)


def test_img2img_schedule_arithmetic():
    from mixgrpo_amd.sample_flux import img2img_start
    N = 8
    assert [N - img2img_start(N, s) for s in (1.0, 0.5, 0.3)] == [8, 4, 2]
    assert [img2img_start(N, s) for s in (1.0, 0.5, 0.3)] == [0, 4, 6]
    with pytest.raises(ValueError):
        img2img_start(N, 0.1)                                                               # leaves no step
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            img2img_start(N, bad)


def _digest(P, prefix):
    h = hashlib.sha256()
    for k in sorted(k for k in P if k.startswith(prefix)):
        h.update(k.encode())
        h.update(str(tuple(P[k].shape)).encode())
        h.update(P[k].contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()


# sha256 over the converted decoder tensors of `AutoencoderKL(VaeConfig(**SMALL), "cpu").init_synthetic(seed=7).P`, taken from
# the commit before the encoder existed (same `_digest`)
PARENT_DECODER_DIGEST = "f0d7c09803f486a3580c01cfa4386b122ed9efe4e6496966bf752caaf6d62a95"


def test_synthetic_decoder_weights_did_not_move():
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    m = AutoencoderKL(VaeConfig(**SMALL), device="cpu").init_synthetic(seed=7)
    assert _digest(m.P, "decoder.") == PARENT_DECODER_DIGEST
    assert m.has_encoder
    # the encoder's draws come from a second generator, seed + 1, in key order
    want = ER.init_params(OV.VaeConfig(**SMALL), seed=8)
    assert torch.equal(m.P["encoder.conv_norm_out.weight"].float(), want["encoder.conv_norm_out.weight"])
    assert torch.equal(m.P["encoder.conv_in.weight"][..., :3].float(), want["encoder.conv_in.weight"].permute(0, 2, 3, 1))
