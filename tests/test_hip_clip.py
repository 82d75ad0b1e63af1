"""The CLIP image tower's kernels (csrc/clip.hip), the tower (mixgrpo_amd/clip_vision.py) and the rewards built on it
(mixgrpo_amd/rewards.py) on the GPU, against the float64 restatement of tests/clip_refs.py."""
import json
import os
import sys

import pytest
import torch

import attn_refs as A
import clip_refs as R
import norm_refs as N

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -776.0                                          # exact in bf16: memory a kernel must leave alone holds it
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to clip.json in that directory


def _record(**kw):
    print(json.dumps(kw))
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "clip.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d.update(kw)
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _g(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ops():
    from mixgrpo_amd import ops
    return ops


# -------------------------------------------------------------------------------------------------------------- attention
ATTN = [(1, 1, 1, 64), (2, 3, 17, 80), (1, 2, 64, 64), (1, 2, 65, 80), (2, 16, 257, 80), (1, 4, 577, 64)]
# every instance of the dispatch (csrc/encoder_attn.hip): DP = 32 exact and padded (d = 32, 16), 64 padded (48), 96 exact, 128
# padded and exact (112, 128), at one key and at 70 (two query blocks, two key blocks, the second with 6 keys)
HEAD_DIMS = [16, 32, 48, 96, 112, 128]
ATTN += [(2, 3, S, d) for d in HEAD_DIMS for S in (1, 70)]
GUARD = 8                                              # guard columns left and right of both buffers (16 bytes)


@pytest.mark.parametrize("family", ["uniform", "ramp"])
@pytest.mark.parametrize("B,H,S,d", ATTN)
def test_vit_attn_fwd(B, H, S, d, family):
    """O against float64 softmax attention on the same bf16 operands, every row within the budget of tests/attn_refs.py for O
    (its constant C["O"], calibrated on the rounding model that kernel contract shares: P rounded to bf16 against a running
    maximum, one rounding of O).  `ramp`: the keys drift along the sequence, so the running maximum keeps growing and the
    accumulators are rescaled in every block.  q | k | v sit inside a buffer whose guard row above and below and guard columns
    left and right hold inf / NaN; O likewise: nothing may leak in, and the guards come back bit for bit."""
    ops = _ops()
    w = H * d
    g = _g(B * 1000 + H * 100 + S + d)
    ld, ldo = 3 * w + 2 * GUARD, w + 2 * GUARD
    buf = torch.full((B * S + 2, ld), float("nan"), dtype=BF, device="cuda")
    buf[:, 0::2] = float("inf")
    q, k, v = (torch.randn(B, S, H, d, device="cuda", generator=g) for _ in range(3))
    if family == "ramp":
        k = k + 3.0 * torch.linspace(0, 1, S, device="cuda").view(1, S, 1, 1) * q.mean(dim=1, keepdim=True).sign()
    buf[1:-1, GUARD:GUARD + 3 * w] = torch.cat([t.reshape(B * S, w) for t in (q, k, v)], 1).to(BF)
    obuf = torch.full((B * S + 2, ldo), float("nan"), dtype=BF, device="cuda")
    obuf[:, 1::2] = float("-inf")
    buf0, obuf0 = buf.clone(), obuf.clone()
    scale = d ** -0.5
    assert ops.vit_attn_fwd(buf[1, GUARD:], ld, obuf[1, GUARD:], ldo, B, H, S, d, scale)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), buf0.view(torch.int16))                    # the operands are only read
    guard = torch.ones_like(obuf, dtype=torch.bool)
    guard[1:-1, GUARD:GUARD + w] = False
    assert torch.equal(obuf.view(torch.int16)[guard], obuf0.view(torch.int16)[guard])
    qkv = buf[1:-1, GUARD:GUARD + 3 * w]
    qb, kb, vb = (t.reshape(B, S, H, d).transpose(1, 2).to(F64) for t in qkv.split(w, -1))
    out = obuf[1:-1, GUARD:GUARD + w].reshape(B, S, H, d).transpose(1, 2)
    ref, budget = R.attention(qb, kb, vb, scale), R.attention_budget(qb, kb, vb, scale)
    ok, msg = A.rows_close(out, ref, budget, A.C["O"])
    print(f"attention {B, H, S, d} {family}: {msg}")
    assert ok, msg
    # power: the reference without its last key is rejected (S > 1)
    if S > 1:
        assert not A.rows_close(out, R.attention(qb, kb[..., :-1, :], vb[..., :-1, :], scale), budget, A.C["O"])[0]


def test_vit_attn_fwd_refuses_long_sequences_and_bad_heads():
    from mixgrpo_amd._lib import MgxError
    ops = _ops()
    x = torch.zeros(8, 3 * 64, dtype=BF, device="cuda")
    o = torch.full((8, 64), SENT, dtype=BF, device="cuda")
    assert ops.vit_attn_fwd(x, 192, o, 64, 1, 1, 4097, 64, 0.125) is False              # rc 1 before anything is launched
    with pytest.raises(MgxError):
        ops.vit_attn_fwd(x, 3 * 72, o, 72, 1, 1, 2, 72, 0.1)                             # head dim % 16
    torch.cuda.synchronize()
    assert (o == SENT).all()


# -------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("M", [1, 17, 514])
@pytest.mark.parametrize("D", [64, 320, 768, 1280, 2048])
def test_layer_norm_affine(D, M):
    """Strided input (ldx = D + 8) and output (ldy = D + 16) with sentinel columns; budget as tests/test_hip_norm_kernels.py
    derives it for ln_modulate: one bf16 ulp plus c 2^-24 on the terms the fp32 arithmetic cancels, c = D / 64 sequential terms
    of a lane + the 6-level wave tree + rsqrt and the products."""
    ops = _ops()
    g = _g(D * 7 + M)
    eps = 1e-5
    xs = torch.full((M, D + 8), SENT, dtype=BF, device="cuda")
    xs[:, :D] = (torch.randn(M, D, device="cuda", generator=g) * 1.5 + 0.3).to(BF)
    gamma = 1 + 0.2 * torch.randn(D, device="cuda", generator=g)
    beta = 0.3 * torch.randn(D, device="cuda", generator=g)
    y = torch.full((M + 1, D + 16), SENT, dtype=BF, device="cuda")
    ops.layer_norm_affine(xs, D + 8, gamma, beta, y, D + 16, M, D, eps)
    x = xs[:, :D]
    xh, mean, rstd = N.layer_norm(x, eps)
    gm, bt = gamma.to(F64), beta.to(F64)
    ref = xh * gm + bt
    c = D / 64 + 8
    mabs = x.to(F64).abs().mean(-1, keepdim=True)
    bound = c * N.U32 * (xh.abs() + mabs * rstd) * gm.abs() + 2 * N.U32 * (xh.abs() * gm.abs() + bt.abs())
    N.assert_ok(N.bf16_close(y[:M, :D], ref, bound))
    assert (y[M] == SENT).all() and (y[:, D:] == SENT).all()
    # power: a mean that misses the row's last 64 elements (one element per lane) is rejected
    if D > 64:
        wrong = (x.to(F64) - x[:, :D - 64].to(F64).sum(-1, keepdim=True) / D) * rstd * gm + bt
        assert not N.bf16_close(y[:M, :D], wrong, bound)[0]
    # in place
    ops.layer_norm_affine(xs, D + 8, gamma, beta, xs, D + 8, M, D, eps)
    assert torch.equal(xs[:, :D], y[:M, :D]) and (xs[:, D:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------ activations
def _act_values():
    v = torch.cat([torch.linspace(-30, 30, 6001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-10, -1e-10, 1e-3, -1e-3, 1e4, -1e4]),
                   torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3])
    return v.to(BF)


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_act_rows(act):
    """Both activations within one bf16 ulp of the float64 result, on values across +-30 with 0, tiny and large magnitudes
    (for x < 0 the exact GELU's 1 + erf(x / sqrt 2) cancels: the result's relative precision must survive it); strided rows,
    out of place and in place."""
    from mixgrpo_amd.clip_vision import ACTS
    ops = _ops()
    v = _act_values()
    n = v.numel()
    Ncol = 64
    M = (n + Ncol - 1) // Ncol
    x = torch.full((M, Ncol + 8), SENT, dtype=BF, device="cuda")
    flat = torch.zeros(M * Ncol, dtype=BF)
    flat[:n] = v
    x[:, :Ncol] = flat.view(M, Ncol).cuda()
    y = torch.full((M + 1, Ncol + 4), SENT, dtype=BF, device="cuda")
    ops.act_rows(x, Ncol + 8, y, Ncol + 4, M, Ncol, ACTS[act])
    ref = R.ACT[act](x[:, :Ncol].to(F64))
    out = y[:M, :Ncol].to(F64)
    assert torch.isfinite(out).all()
    excess = (out - ref).abs() - N.bf16_ulp(ref)
    i = int(excess.flatten().argmax())
    assert excess.max().item() <= 0, (x[:, :Ncol].flatten()[i].item(), out.flatten()[i].item(), ref.flatten()[i].item())
    assert (out != N.bf(ref)).double().mean().item() <= 0.01             # and nearly all correctly rounded
    assert (y[M] == SENT).all() and (y[:, Ncol:] == SENT).all()
    ops.act_rows(x, Ncol + 8, x, Ncol + 8, M, Ncol, ACTS[act])
    assert torch.equal(x[:, :Ncol], y[:M, :Ncol]) and (x[:, Ncol:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("hw,R_", R.RESIZES + [((56, 56), 56)])
def test_clip_preprocess(hw, R_, kind):
    """Levels equal to the restatement's except where its float64 pre-rounding value lies within 1e-3 of a tie (at most 0.5 % of
    the image, each within one level; tests/test_clip_refs.py holds the reference alone to that cap); the patch rows are exactly
    bf16((q / 255 - mean) / std) of those levels in fp32, in the layout row py g + px, column c p p + dy p + dx, the columns
    588 .. 639 zero; the row behind the last patch keeps its sentinel."""
    from mixgrpo_amd.clip_vision import OPENAI_MEAN, OPENAI_STD
    ops = _ops()
    H, W = hw
    p = 14
    img = R.make_image(H, W, kind)
    g = R_ // p
    Kp = ops.clip_patch_cols(p)
    assert Kp == 640
    patches = torch.full((g * g + 1, Kp), SENT, dtype=BF, device="cuda")
    levels = torch.full((3, R_, R_), 7, dtype=torch.uint8, device="cuda")
    ops.clip_preprocess(img.cuda(), R_, p, OPENAI_MEAN, OPENAI_STD, patches[:g * g], levels)
    ref = R.preprocess(img, R_, p, OPENAI_MEAN, OPENAI_STD)
    lv = levels.cpu().to(F64)
    near = R.tie_distance(ref["pre"]) < R.TIE
    assert near.double().mean().item() <= R.TIE_CAP
    diff = (lv - ref["levels"]).abs()
    assert diff[~near].max().item() == 0
    assert diff.max().item() <= 1
    if hw == (56, 56):
        assert torch.equal(lv, R.image_levels(img).to(F64))            # scale 1: the filter is the identity
    m, s = (torch.tensor(t, dtype=F32).view(3, 1, 1) for t in (OPENAI_MEAN, OPENAI_STD))
    want = R.patchify(((lv.float() / 255.0 - m) / s).to(BF)[None], p)
    got = patches.cpu()
    assert torch.equal(got[:g * g, :3 * p * p], want)
    assert (got[:g * g, 3 * p * p:] == 0).all() and (got[g * g] == SENT).all()


# ------------------------------------------------------------------------------------------------------------------ tower
def _configs():
    from mixgrpo_amd.clip_vision import ClipVisionConfig as C
    return {"d80_gelu_56": C(width=320, layers=2, heads=4, mlp_width=640, image_size=56, embed_dim=64, act="gelu"),
            "d64_quick_56": C(width=128, layers=2, heads=2, mlp_width=256, image_size=56, embed_dim=32, act="quick_gelu"),
            "d80_gelu_224": C(width=320, layers=2, heads=4, mlp_width=640, image_size=224, embed_dim=64, act="gelu"),
            "vit_h_width_224": C(width=1280, layers=2, heads=16, mlp_width=5120, image_size=224, embed_dim=1024, act="gelu")}


@pytest.mark.parametrize("name", ["d80_gelu_56", "d64_quick_56", "d80_gelu_224", "vit_h_width_224"])
def test_tower_against_restatement(name):
    """Batches of 1 and 3.  Tolerance: the restatement's bf16-emulation arm against its float64 arm is the error the number
    format causes; the HIP result may be at most twice that in relative L2 and in 1 - cosine (the factor covers a different
    fp32 summation order inside GEMM and attention).  The rows of the batch of 3 equal the one-at-a-time rows bit for bit, and
    a second run gives the same bits."""
    from mixgrpo_amd.clip_vision import ClipVisionTower, convert_state_dict, synthetic_state_dict
    c = _configs()[name]
    sd = synthetic_state_dict(c, seed=5, device="cuda")
    tower = ClipVisionTower(c, device="cuda").load_state_dict(sd)
    P, _ = convert_state_dict(sd, c)
    px = torch.randn(3, 3, c.image_size, c.image_size, device="cuda", generator=_g(11)).to(BF).float()
    got = tower.encode_image(pixel_values=px, normalize=False)
    assert got.shape == (3, c.embed_dim) and got.dtype == F32
    again = tower.encode_image(pixel_values=px, normalize=False)
    assert torch.equal(got, again)
    for i in range(3):
        one = tower.encode_image(pixel_values=px[i:i + 1], normalize=False)
        assert torch.equal(one[0], got[i]), f"image {i} alone differs from its row of the batch"
    f64 = R.tower(P, c, px.to(F64))
    emu = R.tower(P, c, px.to(F64), emulate_bf16=True)
    fig = {"emu_rel_l2": R.rel_l2(emu, f64), "hip_rel_l2": R.rel_l2(got, f64),
           "emu_1mcos": R.one_minus_cos(emu, f64), "hip_1mcos": R.one_minus_cos(got, f64)}
    _record(**{f"tower_{name}": fig})
    assert torch.isfinite(got).all()
    assert fig["hip_rel_l2"] <= 2 * fig["emu_rel_l2"], fig
    assert fig["hip_1mcos"] <= 2 * fig["emu_1mcos"], fig
    nrm = tower.encode_image(pixel_values=px)                              # normalize=True
    assert torch.allclose(nrm.to(F64), got.to(F64) / got.to(F64).norm(dim=-1, keepdim=True), rtol=0, atol=1e-6)


def test_cosine_score_kernel():
    ops = _ops()
    g = _g(3)
    f, t = torch.randn(5, 1024, device="cuda", generator=g), torch.randn(5, 1024, device="cuda", generator=g)
    for fa in (f, f.to(BF)):
        for ta in (t, t.to(BF), t[:1].contiguous()):
            out = torch.empty(5, device="cuda")
            ops.cosine_score(fa, ta, out, 100.0, 18.0, 8.0)
            ref = R.score(fa, ta.expand(5, -1) if ta.shape[0] == 1 else ta, 100.0, 18.0, 8.0)
            # fp32 sums of 1024 terms: 1024 * 2^-24 relative on each of the three sums, scaled by logit_scale / std
            assert (out.to(F64) - ref).abs().max().item() <= 3 * 1024 * 2.0 ** -24 * 100.0 / 8.0


# ---------------------------------------------------------------------------------------------------------------- rewards
def test_rewards_end_to_end(monkeypatch):
    """A tiny synthetic VAE decode -> make_reward_function with the three kinds, no image_processor, PIL not importable on the
    path.  Scores against the restatement's: the tower's float64 arm on the pixels of the levels the preprocessing kernel gives
    for the same decoded images (test_clip_preprocess holds those).  Tolerance from the same rule as the tower's: a cosine moves
    by at most |f' / |f'| - f / |f|| <= 2 |f' - f| / |f|, and the HIP features may be off by twice the emulation arm's relative
    error e (worst image): |score' - score| <= (logit scale / std) * 4 e."""
    from mixgrpo_amd import ops
    from mixgrpo_amd.clip_vision import ClipVisionConfig, ClipVisionTower, convert_state_dict, synthetic_state_dict
    from mixgrpo_amd.reward_adapter import decode_latents, make_reward_function
    from mixgrpo_amd.rewards import KINDS, ClipReward, TextFeatureCache
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    monkeypatch.setitem(sys.modules, "PIL", None)
    monkeypatch.setitem(sys.modules, "PIL.Image", None)
    vae = AutoencoderKL(VaeConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1, sample_size=64), device="cuda")
    vae.init_synthetic(seed=2)
    c = ClipVisionConfig(width=320, layers=2, heads=4, mlp_width=640, image_size=56, embed_dim=64, act="gelu")
    sd = synthetic_state_dict(c, seed=7, device="cuda")
    tower = ClipVisionTower(c, device="cuda").load_state_dict(sd)
    prompts = ["a red cube", "a blue sphere", "a red cube"]
    text = torch.randn(2, c.embed_dim, generator=torch.Generator().manual_seed(1))
    cache = TextFeatureCache(features=text, prompts=prompts[:2])
    models = {k: ClipReward(tower, cache, k) for k in KINDS}
    weights = {"HPSClipRewardModel": 1.0, "CLIPScoreRewardModel": 0.5, "PickScoreRewardModel": 2.0}
    latents = torch.randn(3, 16, 64, device="cuda", generator=_g(4)).to(BF)
    total, per = make_reward_function(vae, models, weights, 64, 64)(latents, prompts)
    assert set(per) == set(KINDS) and len(total) == 3
    with pytest.raises(KeyError, match="a green cone"):
        make_reward_function(vae, models, weights, 64, 64)(latents[:1], ["a green cone"])
    # the restatement on the same decoded images
    images = decode_latents(vae, latents, 64, 64)
    assert images.shape == (3, 3, 64, 64) and images.dtype == BF
    P, ls = convert_state_dict(sd, c)
    m, s = (torch.tensor(t, dtype=F64, device="cuda").view(3, 1, 1) for t in (c.image_mean, c.image_std))
    px = []
    for im in images:
        lv = torch.empty(3, 56, 56, dtype=torch.uint8, device="cuda")
        ops.clip_preprocess(im.contiguous(), 56, 14, c.image_mean, c.image_std, torch.empty(16, 640, dtype=BF, device="cuda"), lv)
        px.append(R.bf((lv.to(F64) / 255 - m) / s))
    px = torch.stack(px)
    f64, emu = R.tower(P, c, px), R.tower(P, c, px, emulate_bf16=True)
    e = max(R.rel_l2(emu[i], f64[i]) for i in range(3))
    t = text.cuda()[[0, 1, 0]]
    fig = {"emu_rel_l2_worst": e}
    for k in KINDS:
        scale, mean, std = models[k].score_params()
        ref = R.score(f64, t, scale, mean, std)
        err = (torch.tensor(per[k], dtype=F64, device="cuda") - ref).abs().max().item()
        fig[k] = {"err": err, "tol": scale / std * 4 * e}
        assert err <= scale / std * 4 * e, (k, fig)
    assert models["PickScoreRewardModel"].score_params()[0] == pytest.approx(100.0, rel=1e-6)
    for i in range(3):
        assert total[i] == pytest.approx(sum(weights[k] * per[k][i] for k in KINDS))
    assert per["HPSClipRewardModel"][0] != per["HPSClipRewardModel"][1]
    _record(rewards_end_to_end=fig)


# ----------------------------------------------------------------------------------------------------------------- timing
def test_vit_h_14_timing_is_recorded():
    """Milliseconds per image of the full ViT-H/14 (32 layers, synthetic weights) at batch 8: the tower alone from pixel values,
    and from eight decoded 1024 x 1024 images through the preprocessing.  Recorded, no threshold."""
    from mixgrpo_amd.clip_vision import VIT_H_14, ClipVisionTower
    tower = ClipVisionTower(VIT_H_14, device="cuda").init_synthetic(seed=0)
    px = torch.randn(8, 3, 224, 224, device="cuda", generator=_g(0))
    images = (torch.rand(8, 3, 1024, 1024, device="cuda", generator=_g(1)) * 2 - 1).to(BF)
    fig, REPS = {}, 20                                                      # a window of about 0.2 s per figure
    for tag, kw in (("tower_ms_per_image", dict(pixel_values=px)), ("preprocess_and_tower_ms_per_image", dict(images=images))):
        out = tower.encode_image(**kw)                                      # warm-up: buffers, kernel loads
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            out = tower.encode_image(**kw)
        e1.record()
        torch.cuda.synchronize()
        fig[tag] = e0.elapsed_time(e1) / REPS / 8
        assert torch.isfinite(out).all() and out.shape == (8, 1024)
    _record(vit_h_14_batch8=fig)
