"""The ImageReward scorer on the GPU: the two kernels of csrc/blip.hip, the encoders and the scorer of
mixgrpo_amd/image_reward.py and the ImageRewardModel entry of rewards.builtin_rewards, against the float64 restatements of
tests/blip_refs.py."""
import json
import math
import os

import pytest
import torch

import attn_refs as A
import blip_refs as BR
import clip_refs as R
import norm_refs as NR

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -776.0                                          # exact in bf16 and fp32: memory a kernel must leave alone holds it
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to image_reward.json in that directory


def _record(**kw):
    print(json.dumps(kw))
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "image_reward.json")
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
XATTN = [(1, 1, 1, 1, 64), (2, 3, 5, 17, 64), (2, 12, 35, 35, 64), (1, 2, 35, 197, 64), (1, 2, 64, 65, 64), (1, 2, 65, 64, 80),
         (1, 4, 130, 300, 128)]
# every DP of the dispatch (csrc/encoder_attn.hip): 32 exact and padded (d = 32, 16), 64 padded (48), 96 exact, 128 padded and
# exact (112, 128); 5 queries against two key blocks (the second with 6 keys), and two query blocks against 5 keys
HEAD_DIMS = [16, 32, 48, 96, 112, 128]
XATTN += [(2, 3, Sq, Skv, d) for d in HEAD_DIMS for Sq, Skv in ((5, 70), (70, 5))]
GUARD = 8                                              # guard columns left and right of every buffer (16 bytes)


def _length_vectors(B, Skv):
    """The ragged arm's key lengths: 1, 63, 64, 65, 129 and Skv, those that fit, rotated through the samples -- every one of
    them is used at every shape it fits"""
    cand = sorted({n for n in (1, 63, 64, 65, 129, Skv) if n <= Skv})
    return [torch.tensor([cand[(j + b) % len(cand)] for b in range(B)]) for j in range(len(cand))]


def _guarded(rows, cols, fill=None):
    """[rows + 2, cols + 2 GUARD] bf16 of inf / NaN with `fill` [rows, cols] inside a guard row above and below and guard
    columns left and right"""
    buf = torch.full((rows + 2, cols + 2 * GUARD), float("nan"), dtype=BF, device="cuda")
    buf[:, 0::2] = float("inf")
    if fill is not None:
        buf[1:-1, GUARD:GUARD + cols] = fill.to(BF)
    return buf


@pytest.mark.parametrize("arm", ["all_keys", "ragged"])
@pytest.mark.parametrize("B,H,Sq,Skv,d", XATTN)
def test_xattn_fwd(B, H, Sq, Skv, d, arm):
    """O against float64 attention over the keys below each sample's length on the same bf16 operands, every row within the
    budget of tests/attn_refs.py for O.  The construction is test_text_attn_fwd's: q, k and v each sit inside a buffer of their
    own whose guard rows and columns hold inf / NaN, and in the ragged arm so do the k and v rows at or beyond kv_len[b]; O lies
    between sentinels, which come back bit for bit; the operands are only read.  Power: the ragged arm rejects the reference
    that ignores the lengths and the one with every length off by one."""
    ops = _ops()
    w = H * d
    g = _g(B * 1000 + H * 100 + Sq * 7 + Skv + d)
    q, k, v = (torch.randn(B, S, H, d, device="cuda", generator=g) for S in (Sq, Skv, Skv))
    scale = d ** -0.5
    qh, kh, vh = (t.to(BF).transpose(1, 2).to(F64) for t in (q, k, v))
    for lens in ([None] if arm == "all_keys" else _length_vectors(B, Skv)):
        kk, vv = k.clone(), v.clone()
        if lens is not None:
            for b in range(B):
                kk[b, int(lens[b]):, :, 0::2], kk[b, int(lens[b]):, :, 1::2] = float("nan"), float("-inf")
                vv[b, int(lens[b]):, :, 0::2], vv[b, int(lens[b]):, :, 1::2] = float("inf"), float("nan")
        qb, kb, vb = _guarded(B * Sq, w, q.reshape(B * Sq, w)), _guarded(B * Skv, w, kk.reshape(B * Skv, w)), _guarded(B * Skv, w, vv.reshape(B * Skv, w))
        ob = torch.full((B * Sq + 2, w + 2 * GUARD), float("nan"), dtype=BF, device="cuda")
        ob[:, 1::2] = float("-inf")
        keep = [t.clone() for t in (qb, kb, vb, ob)]
        ld = w + 2 * GUARD
        assert ops.xattn_fwd(qb[1, GUARD:], ld, kb[1, GUARD:], ld, vb[1, GUARD:], ld, ob[1, GUARD:], ld, B, H, Sq, Skv, d, scale, kv_len=lens)
        torch.cuda.synchronize()
        for t, t0 in zip((qb, kb, vb), keep):
            assert torch.equal(t.view(torch.int16), t0.view(torch.int16))                # the operands are only read
        guard = torch.ones_like(ob, dtype=torch.bool)
        guard[1:-1, GUARD:GUARD + w] = False
        assert torch.equal(ob.view(torch.int16)[guard], keep[3].view(torch.int16)[guard])
        out = ob[1:-1, GUARD:GUARD + w].reshape(B, Sq, H, d).transpose(1, 2)
        ref, budget = BR.xattention(qh, kh, vh, scale, lens), BR.xattention_budget(qh, kh, vh, scale, lens)
        ok, msg = A.rows_close(out, ref, budget, A.C["O"])
        print(f"xattn {B, H, Sq, Skv, d} lengths {None if lens is None else lens.tolist()}: {msg}")
        assert ok, msg
        if lens is not None and bool((lens < Skv).any()):
            assert not A.rows_close(out, BR.xattention(qh, kh, vh, scale), budget, A.C["O"])[0]
        if lens is not None and Skv > 1:
            off = torch.where(lens > 1, lens - 1, lens + 1)
            assert not A.rows_close(out, BR.xattention(qh, kh, vh, scale, off), budget, A.C["O"])[0]


@pytest.mark.parametrize("B,H,S,d", [(2, 3, 17, 64), (1, 2, 130, 80), (2, 12, 35, 64), (2, 3, 70, 16), (2, 3, 70, 128)])
def test_xattn_fwd_packed(B, H, S, d):
    """q, k and v pointing into one packed q | k | v buffer, Sq == Skv, no lengths: the problem of mgx_vit_attn_fwd.  Both
    entry points launch the same kernel instance (csrc/encoder_attn.hip), so beyond the float64 budget the two agree bit for
    bit."""
    ops = _ops()
    w = H * d
    qkv = torch.randn(B * S, 3 * w, device="cuda", generator=_g(S + d)).to(BF)
    o, o_vit = (torch.full((B * S + 1, w), SENT, dtype=BF, device="cuda") for _ in range(2))
    assert ops.xattn_fwd(qkv, 3 * w, qkv[:, w:], 3 * w, qkv[:, 2 * w:], 3 * w, o, w, B, H, S, S, d, d ** -0.5)
    assert ops.vit_attn_fwd(qkv, 3 * w, o_vit, w, B, H, S, d, d ** -0.5)
    qh, kh, vh = (t.reshape(B, S, H, d).transpose(1, 2).to(F64) for t in qkv.split(w, -1))
    ref, budget = BR.xattention(qh, kh, vh, d ** -0.5), BR.xattention_budget(qh, kh, vh, d ** -0.5)
    A.assert_ok(A.rows_close(o[:B * S].reshape(B, S, H, d).transpose(1, 2), ref, budget, A.C["O"]))
    assert (o[B * S] == SENT).all()
    assert torch.equal(o.view(torch.int16), o_vit.view(torch.int16))


def test_xattn_fwd_refusals():
    """More than 4096 keys or queries: False before anything is launched; a head dim off 16 raises; a length of 0, one above
    Skv, a float or a wrongly sized length tensor raise a ValueError in the wrapper.  O stays untouched in all of these."""
    from mixgrpo_amd._lib import MgxError
    ops = _ops()
    x = torch.randn(64, 128, device="cuda", generator=_g(1)).to(BF)
    o = torch.full((64, 128), SENT, dtype=BF, device="cuda")
    assert ops.xattn_fwd(x, 64, x, 64, x, 64, o, 64, 1, 1, 2, 4097, 64, 0.125) is False
    assert ops.xattn_fwd(x, 64, x, 64, x, 64, o, 64, 1, 1, 4097, 2, 64, 0.125) is False
    with pytest.raises(MgxError):
        ops.xattn_fwd(x, 72, x, 72, x, 72, o, 72, 1, 1, 2, 2, 72, 0.1)                    # head dim % 16
    with pytest.raises(MgxError):
        ops.xattn_fwd(x, 68, x, 64, x, 64, o, 64, 1, 1, 2, 2, 64, 0.1)                    # a row stride off 8
    for bad in (torch.tensor([3, 0]), torch.tensor([9, 1]), torch.tensor([-1, 2])):
        with pytest.raises(ValueError, match=str(int(bad[(bad < 1) | (bad > 8)][0]))):
            ops.xattn_fwd(x, 128, x, 128, x, 128, o, 128, 2, 2, 4, 8, 64, 0.125, kv_len=bad)
    with pytest.raises(ValueError):
        ops.xattn_fwd(x, 128, x, 128, x, 128, o, 128, 2, 2, 4, 8, 64, 0.125, kv_len=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError):
        ops.xattn_fwd(x, 128, x, 128, x, 128, o, 128, 2, 2, 4, 8, 64, 0.125, kv_len=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        ops.xattn_fwd(x, 128, x, 128, x, 128, o, 128, 2, 2, 4, 8, 64, 0.125, kv_len=torch.tensor([9, 1]).cuda())   # on the device too
    torch.cuda.synchronize()
    assert (o == SENT).all()


# ------------------------------------------------------------------------------------------------------------ fp32 Linear
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 16), (3, 16, 64), (17, 1024, 768), (40, 1, 16)])
def test_linear_rows_f32(M, N, K, dtype):
    """Strided input (K + 8) and output (N + 3) rows with sentinels, against float64.  Bound, by the rule tests/norm_refs.py
    uses for sums (`reduction_close`): c 2^-24 sum |terms| with c = K / 64 sequential terms of a lane (at least 1) + the 6-level
    wave tree + the product's rounding and the bias sum (+ 8 in all).  With shift and scale the result equals the separate fp32
    evaluation (plain - shift) / scale to one fp32 ulp."""
    ops = _ops()
    g = _g(M * 31 + N * 7 + K)
    xs = torch.full((M, K + 8), SENT, dtype=dtype, device="cuda")
    xs[:, :K] = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    x = xs[:, :K]
    W, bias = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5, torch.randn(N, device="cuda", generator=g)
    ys = torch.full((M + 1, N + 3), SENT, dtype=F32, device="cuda")
    ops.linear_rows_f32(x, W, bias, ys[:M, :N])
    ref = x.to(F64) @ W.to(F64).t() + bias.to(F64)
    terms = x.to(F64).abs() @ W.to(F64).abs().t() + bias.to(F64).abs()
    c = max(K / 64, 1) + 8
    NR.assert_ok(NR.reduction_close(ys[:M, :N], ref, terms, c))
    assert (ys[M] == SENT).all() and (ys[:, N:] == SENT).all() and (xs[:, K:] == SENT).all()
    # power: the sum without its last four terms, and without the bias, is rejected
    assert not NR.reduction_close(ys[:M, :N], x.to(F64)[:, :K - 4] @ W.to(F64)[:, :K - 4].t() + bias.to(F64), terms, c)[0]
    assert not NR.reduction_close(ys[:M, :N], ref - bias.to(F64), terms, c)[0]
    nb = torch.full((M, N), SENT, dtype=F32, device="cuda")
    ops.linear_rows_f32(x, W, None, nb)
    NR.assert_ok(NR.reduction_close(nb, ref - bias.to(F64), terms, c))
    zs = torch.full((M + 1, N + 3), SENT, dtype=F32, device="cuda")
    ops.linear_rows_f32(x, W, bias, zs[:M, :N], shift=0.16717362830052426, scale=1.0333394966054072)
    want = (ys[:M, :N] - torch.tensor(0.16717362830052426, dtype=F32, device="cuda")) / torch.tensor(1.0333394966054072, dtype=F32, device="cuda")
    assert ((zs[:M, :N] - want).abs() <= 2.0 ** -23 * want.abs()).all()
    assert (zs[M] == SENT).all() and (zs[:, N:] == SENT).all()


def test_linear_rows_f32_refusals():
    from mixgrpo_amd._lib import MgxError
    ops = _ops()
    y = torch.full((2, 4), SENT, dtype=F32, device="cuda")
    with pytest.raises(MgxError):
        ops.linear_rows_f32(torch.zeros(2, 6, dtype=BF, device="cuda"), torch.zeros(4, 6, device="cuda"), None, y)     # K % 4
    with pytest.raises(ValueError):
        ops.linear_rows_f32(torch.zeros(2, 8, dtype=BF, device="cuda"), torch.zeros(4, 8, dtype=BF, device="cuda"), None, y)
    with pytest.raises(ValueError):
        ops.linear_rows_f32(torch.zeros(2, 8, dtype=BF, device="cuda"), torch.zeros(4, 8, device="cuda"), None, y, shift=1.0)
    with pytest.raises(MgxError):
        ops.linear_rows_f32(torch.zeros(2, 8, dtype=BF, device="cuda"), torch.zeros(4, 8, device="cuda"), None, y, shift=1.0, scale=0.0)
    torch.cuda.synchronize()
    assert (y == SENT).all()


# --------------------------------------------------------------------------------------------------------------- encoders
PROMPTS = ["", "a red cube", "x" * 34, "a green cone on a long, long table, seen from above", "two dogs"]      # lengths 1, 11, 35, 35, 9


@pytest.fixture(scope="module")
def wide():
    """True widths (ViT 1024, BERT 768, 197 image tokens), 2 layers each, synthetic weights: (model, internal dict)"""
    from mixgrpo_amd import image_reward as IR
    vc = IR.BlipVisionConfig(layers=2)
    tc = IR.BertXattnConfig(vocab=1000, layers=2)
    sd = IR.synthetic_state_dict(vc, tc, seed=5, device="cuda")
    model = IR.ImageRewardModel(vc, tc, tokenizer=BR.stub_tokenizer(35, 1000), device="cuda").load_state_dict(sd)
    return model, IR.convert_state_dict(sd, vc, tc)


def test_encoders_against_restatement(wide):
    """Batch 3.  Tolerance, the rule of tests/test_hip_text.py::test_towers_against_restatement: the restatement's
    bf16-emulation arm against its float64 arm is the error the number format causes; the HIP result may be at most twice that
    in relative L2.  The image encoder: all 3 x 197 token rows.  The text encoder: ragged prompts (lengths 1, 11 and 35) against
    those image tokens -- all three arms read the HIP tokens, so that the figure is the text encoder's own --, compared on the
    real rows and on the scores."""
    model, P = wide
    vc, tc = model.vision.config, model.text.config
    px = torch.randn(3, 3, 224, 224, device="cuda", generator=_g(11)).to(BF).float()
    tokens = model.vision.encode_tokens(pixel_values=px).clone()
    assert tokens.shape == (3 * 197, 1024) and tokens.dtype == BF and torch.isfinite(tokens.float()).all()
    assert torch.equal(tokens, model.vision.encode_tokens(pixel_values=px))
    f64, emu = (BR.vit_encoder(P, vc, px.to(F64), emulate_bf16=e) for e in (False, True))
    fig = {"vit_emu_rel_l2": BR.rel_l2(emu, f64), "vit_hip_rel_l2": BR.rel_l2(tokens.view(3, 197, 1024), f64)}
    ids, lens = model.tokenize(PROMPTS[:3])
    assert lens.tolist() == [1, 11, 35]
    hidden = model.text.encode(ids, lens, tokens).view(3, 35, 768).clone()
    t64 = tokens.view(3, 197, 1024).to(F64)
    h64, hemu = (BR.text_encoder(P, tc, ids, lens, t64, emulate_bf16=e) for e in (False, True))
    real = (torch.arange(35)[None] < lens[:, None]).cuda()
    fig.update(text_emu_rel_l2=BR.rel_l2(hemu[real], h64[real]), text_hip_rel_l2=BR.rel_l2(hidden[real], h64[real]))
    scores = model.score_tokens(ids, lens, pixel_values=px)
    assert scores.shape == (3,) and scores.dtype == F32
    s64, semu = ((BR.head_layers(P, h[:, 0]) - model.mean) / model.std for h in (h64, hemu))
    fig.update(score_emu_rel_l2=BR.rel_l2(semu, s64), score_hip_rel_l2=BR.rel_l2(scores, s64), scores=scores.tolist())
    _record(encoders_against_restatement=fig)
    assert fig["vit_hip_rel_l2"] <= 2 * fig["vit_emu_rel_l2"], fig
    assert fig["text_hip_rel_l2"] <= 2 * fig["text_emu_rel_l2"], fig
    assert fig["score_hip_rel_l2"] <= 2 * fig["score_emu_rel_l2"], fig
    assert len(set(scores.tolist())) == 3


def test_score_invariances(wide):
    """All torch.equal: a pair's score alone and inside a batch of 5; whatever token ids its padding holds; whatever its batch
    neighbours' prompts are."""
    model, _ = wide
    images = (torch.rand(5, 3, 96, 80, device="cuda", generator=_g(4)) * 2 - 1).to(BF)
    ids, lens = model.tokenize(PROMPTS)
    assert lens.tolist() == [1, 11, 35, 35, 9]
    batch = model.score_tokens(ids, lens, images=list(images)).clone()
    assert torch.isfinite(batch).all() and len(set(batch.tolist())) == 5
    for i in range(5):
        alone = model.score_tokens(ids[i:i + 1], lens[i:i + 1], images=[images[i]])
        assert torch.equal(alone[0], batch[i]), f"pair {i} alone differs from its place in the batch"
    other = ids.clone()
    pad = torch.arange(35)[None] >= lens[:, None]
    other[pad] = torch.randint(1, 1000, (int(pad.sum()),), generator=torch.Generator().manual_seed(1))
    assert torch.equal(model.score_tokens(other, lens, images=list(images)), batch)
    ids2, lens2 = model.tokenize(["something else entirely", PROMPTS[1], "q", "", PROMPTS[4]])
    mixed = model.score_tokens(ids2, lens2, images=list(images))
    assert torch.equal(mixed[[1, 4]], batch[[1, 4]]) and not torch.equal(mixed[[0, 2, 3]], batch[[0, 2, 3]])
    with pytest.raises(ValueError, match="outside"):
        model.score_tokens(ids, torch.tensor([1, 11, 36, 35, 9]), images=list(images))
    with pytest.raises(ValueError, match="vocabulary"):
        model.score_tokens(ids + 995, lens, images=list(images))


# ------------------------------------------------------------------------------------------------------------- end to end
def _tiny():
    from mixgrpo_amd import image_reward as IR
    return (IR.BlipVisionConfig(width=128, layers=2, heads=2, mlp_width=256, patch_size=16, image_size=64),
            IR.BertXattnConfig(vocab=300, positions=40, width=128, layers=2, heads=2, mlp_width=256, encoder_width=128))


def test_image_reward_through_compute_reward():
    """ImageRewardModel on synthetic weights through reward_adapter.compute_reward next to a ClipReward head, with weights;
    mismatched counts raise before anything runs."""
    from mixgrpo_amd import image_reward as IR
    from mixgrpo_amd.clip_vision import ClipVisionConfig, ClipVisionTower
    from mixgrpo_amd.reward_adapter import compute_reward
    from mixgrpo_amd.rewards import ClipReward, TextFeatureCache
    vc, tc = _tiny()
    ir = IR.ImageRewardModel(vc, tc, tokenizer=BR.stub_tokenizer(35, 300), device="cuda").init_synthetic(seed=3)
    c = ClipVisionConfig(width=128, layers=2, heads=2, mlp_width=256, image_size=56, embed_dim=64, act="quick_gelu")
    tower = ClipVisionTower(c, device="cuda").init_synthetic(seed=7)
    prompts = ["a red cube", "a blue sphere", "a red cube"]
    cache = TextFeatureCache(features=torch.randn(2, 64, generator=torch.Generator().manual_seed(1)), prompts=prompts[:2])
    models = {"ImageRewardModel": ir, "HPSClipRewardModel": ClipReward(tower, cache, "HPSClipRewardModel")}
    weights = {"ImageRewardModel": 0.5, "HPSClipRewardModel": 2.0}
    images = list((torch.rand(3, 3, 72, 64, device="cuda", generator=_g(4)) * 2 - 1).to(BF))
    total, ok, per, _ = compute_reward(images, prompts, models, weights)
    assert set(per) == set(models) and ok == [1, 1, 1] and all(math.isfinite(v) for v in per["ImageRewardModel"])
    for i in range(3):
        assert total[i] == pytest.approx(0.5 * per["ImageRewardModel"][i] + 2.0 * per["HPSClipRewardModel"][i])
    assert per["ImageRewardModel"] == ir(images, prompts) and per["ImageRewardModel"][0] != per["ImageRewardModel"][2]
    assert ir(images[0], prompts[0]) == per["ImageRewardModel"][:1]                      # one image, one string
    assert ir(torch.stack(images), prompts) == per["ImageRewardModel"]                    # a [B, 3, H, W] tensor
    # against the restatement, on the pixels of the levels the preprocessing kernel gives: |hip - f64| <= 2 |emu - f64| over the batch
    P = IR.convert_state_dict(IR.synthetic_state_dict(vc, tc, seed=3, device="cuda"), vc, tc)
    ids, lens = ir.tokenize(prompts)
    s64, semu = (BR.score(P, vc, tc, _kernel_pixels(images, vc), ids, lens, ir.mean, ir.std, emulate_bf16=e)[0] for e in (False, True))
    got = torch.tensor(per["ImageRewardModel"], dtype=F64, device="cuda")
    assert (got - s64).norm().item() <= 2 * (semu - s64).norm().item(), (got, s64, semu)
    with pytest.raises(ValueError, match="3 images for 2 prompts"):
        ir(images, prompts[:2])
    with pytest.raises(AssertionError):
        compute_reward(images, prompts[:2], models, weights)


def _kernel_pixels(images, vc):
    """[B, 3, R, R] float64: the bf16 pixels of the levels mgx_clip_preprocess gives (tests/test_hip_clip.py holds those)"""
    ops = _ops()
    m, s = (torch.tensor(t, dtype=F64, device="cuda").view(3, 1, 1) for t in (vc.image_mean, vc.image_std))
    g = vc.grid
    px = []
    for im in images:
        lv = torch.empty(3, vc.image_size, vc.image_size, dtype=torch.uint8, device="cuda")
        ops.clip_preprocess(im.contiguous(), vc.image_size, vc.patch_size, vc.image_mean, vc.image_std,
                            torch.empty(g * g, ops.clip_patch_cols(vc.patch_size), dtype=BF, device="cuda"), lv)
        px.append(R.bf((lv.to(F64) / 255 - m) / s))
    return torch.stack(px)


def test_pil_images_take_the_host_path():
    """The same four images as PIL images (resized by PIL on the host, as the reference does) and as device tensors (resized by
    the preprocessing kernel).  The two resizes may differ by one level (tests/test_clip_refs.py::
    test_preprocess_layout_and_pil_path), so the two scores are different numbers: each is held to the restatement on its own
    pixels by the encoders' rule, |hip - f64| <= 2 |emu - f64| over the batch, and the levels are within one of each other."""
    from PIL import Image
    from mixgrpo_amd import image_reward as IR
    from mixgrpo_amd.clip_vision import pil_pixel_values
    vc, tc = _tiny()
    sd = IR.synthetic_state_dict(vc, tc, seed=6, device="cuda")
    ir = IR.ImageRewardModel(vc, tc, tokenizer=BR.stub_tokenizer(35, 300), device="cuda").load_state_dict(sd)
    P = IR.convert_state_dict(sd, vc, tc)
    prompts = ["a red cube", "", "a blue sphere on a table", "two dogs"]
    imgs = [R.make_image(H, W, kind, seed=i) for i, (H, W, kind) in enumerate([(96, 80, "smooth"), (64, 64, "noise"), (100, 130, "smooth"), (80, 96, "noise")])]
    pils = [Image.fromarray(R.image_levels(im).permute(1, 2, 0).numpy().astype("uint8")) for im in imgs]
    dev = [im.cuda() for im in imgs]
    ids, lens = ir.tokenize(prompts)
    px_pil = torch.stack([R.bf(pil_pixel_values(p, vc).to(F64)) for p in pils]).cuda()
    px_dev = _kernel_pixels(dev, vc)
    step = 1 / (255 * min(vc.image_std))
    assert (px_pil - px_dev).abs().max().item() <= step * 1.01 + 2.0 ** -8 * px_dev.abs().max().item()    # one level + the bf16 rounding
    fig = {}
    for tag, images, px in (("pil", pils, px_pil), ("device", dev, px_dev)):
        got = torch.tensor(ir(images, prompts), dtype=F64, device="cuda")
        s64, semu = (BR.score(P, vc, tc, px, ids, lens, ir.mean, ir.std, emulate_bf16=e)[0] for e in (False, True))
        fig[tag] = {"hip_err": (got - s64).norm().item(), "emu_err": (semu - s64).norm().item(), "scores": got.tolist()}
        assert fig[tag]["hip_err"] <= 2 * fig[tag]["emu_err"], fig
    _record(pil_versus_device=fig)
    assert ir([pils[0], dev[1]], prompts[:2]) == [fig["pil"]["scores"][0], fig["device"]["scores"][1]]     # mixed in one call


def test_builtin_rewards_from_files(tmp_path, monkeypatch):
    """A written checkpoint (.safetensors in transformers' names, .pt in upstream's) + med_config.json + the config file: the
    same scores as the model built in memory; `args` supplies the two paths an entry leaves out."""
    from types import SimpleNamespace
    from safetensors.torch import save_file
    from mixgrpo_amd import image_reward as IR
    from mixgrpo_amd import rewards as RW
    vc, tc = _tiny()
    sd = {k: v.cpu().contiguous() for k, v in IR.synthetic_state_dict(vc, tc, seed=3, device="cuda").items()}
    med = dict(vocab_size=tc.vocab, max_position_embeddings=tc.positions, hidden_size=tc.width, num_hidden_layers=tc.layers,
               num_attention_heads=tc.heads, intermediate_size=tc.mlp_width, layer_norm_eps=tc.layer_norm_eps, hidden_act="gelu")
    (tmp_path / "med_config.json").write_text(json.dumps(med))
    save_file(sd, str(tmp_path / "ImageReward.safetensors"))
    a, b = IR._hf_names(vc, tc), IR._upstream_names(vc, tc)
    up = {}
    for name, src in a.items():
        for x, y in zip(src if isinstance(src, tuple) else (src,), b[name] if isinstance(b[name], tuple) else (b[name],)):
            up[y] = sd[x]
    torch.save(up, str(tmp_path / "ImageReward.pt"))
    cfg = tmp_path / "rewards.json"
    monkeypatch.setenv(RW.CONFIG_ENV, str(cfg))
    images = list((torch.rand(2, 3, 64, 64, device="cuda", generator=_g(2)) * 2 - 1).to(BF))
    prompts = ["a red cube", "a blue sphere"]
    want = IR.ImageRewardModel(vc, tc, tokenizer=BR.stub_tokenizer(35, 300), mean=0.25, std=2.0, device="cuda").load_state_dict(sd)(images, prompts)
    cfg.write_text(json.dumps({"ImageRewardModel": {"checkpoint": str(tmp_path / "ImageReward.safetensors"),
                                                    "med_config": str(tmp_path / "med_config.json"), "mean": 0.25, "std": 2.0}}))
    m = RW.builtin_rewards(None)["ImageRewardModel"]
    assert isinstance(m, IR.ImageRewardModel) and m.tokenizer == str(tmp_path) and (m.vision.config, m.text.config) == (vc, tc)
    m.tokenizer = BR.stub_tokenizer(35, 300)                                             # no vocabulary file exists offline
    assert m(images, prompts) == want
    cfg.write_text(json.dumps({"ImageRewardModel": {"mean": 0.25, "std": 2.0, "tokenizer_dir": "/nowhere"}}))
    m = RW.builtin_rewards(SimpleNamespace(image_reward_path=str(tmp_path / "ImageReward.pt"),
                                           image_reward_med_config=str(tmp_path / "med_config.json")))["ImageRewardModel"]
    assert m.tokenizer == "/nowhere"
    m.tokenizer = BR.stub_tokenizer(35, 300)
    assert m(images, prompts) == want


# ----------------------------------------------------------------------------------------------------------------- timing
def test_image_reward_timing_is_recorded():
    """Full size (ViT-L/16 of 24 layers, BERT of 12), batch 8, synthetic weights, device events around 20 calls after a warm-up
    call: milliseconds per batch and per pair for the image encoder alone (from pixel values) and for the whole score (eight
    decoded 1024 x 1024 images through the preprocessing, token ids from the host); the text encoder's launch count (its 8 x 35
    rows are latency-bound).  Recorded, no threshold: nobody has measured this."""
    from mixgrpo_amd import image_reward as IR
    model = IR.ImageRewardModel(tokenizer=BR.stub_tokenizer(35, 30524), device="cuda").init_synthetic(seed=0)
    REPS, B = 20, 8
    px = torch.randn(B, 3, 224, 224, device="cuda", generator=_g(0))
    images = list((torch.rand(B, 3, 1024, 1024, device="cuda", generator=_g(1)) * 2 - 1).to(BF))
    ids, lens = model.tokenize([p + " number %d" % i for i, p in enumerate(PROMPTS + PROMPTS[1:4])])
    fig = {}
    for tag, call in (("image_encoder", lambda: model.vision.encode_tokens(pixel_values=px)),
                      ("whole_score", lambda: model.score_tokens(ids, lens, images=images))):
        out = call()                                                        # warm-up: buffers, kernel loads
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            out = call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / REPS
        fig[tag] = {"ms_per_batch8": ms, "ms_per_pair": ms / B}
        assert torch.isfinite(out.float()).all() and math.isfinite(ms) and ms > 0
    fig["text_encoder_launches"] = model.text.launches
    assert model.text.launches == 3 + 12 * 12          # embedding, its LayerNorm, the one K | V GEMM; 12 launches a layer
    _record(image_reward_batch8=fig)
