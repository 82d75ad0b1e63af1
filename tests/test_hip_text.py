"""The text encoders' kernels (csrc/text.hip), the towers (mixgrpo_amd/clip_text.py, mixgrpo_amd/t5.py) and the rewards that
encode their own prompts (mixgrpo_amd/rewards.py) on the GPU, against the float64 restatements of tests/text_refs.py."""
import json
import math
import os
from dataclasses import replace

import pytest
import torch

import attn_refs as A
import norm_refs as N
import text_refs as T

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -776.0                                          # exact in bf16: memory a kernel must leave alone holds it
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to text.json in that directory


def _record(**kw):
    print(json.dumps(kw))
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "text.json")
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
ATTN = [(1, 1, 1, 64), (2, 3, 17, 64), (1, 2, 64, 64), (1, 2, 65, 64), (2, 12, 77, 64), (1, 2, 130, 80), (1, 4, 512, 64)]
GUARD = 8                                              # guard columns left and right of both buffers (16 bytes)
# every instance of the dispatch (csrc/encoder_attn.hip): DP = 32 exact and padded (d = 32, 16), 64 padded (48), 96 exact, 128
# padded and exact (112, 128), at one key and at 70 (two query blocks, two key blocks, the second with 6 keys, a diagonal block
# for the causal arm); `both` (mask and table at once) once per DP
HEAD_DIMS = [16, 32, 48, 96, 112, 128]
ATTN_ARMS = [shape + (arm,) for shape in ATTN + [(2, 3, S, d) for d in HEAD_DIMS for S in (1, 70)] for arm in ("causal", "bias", "plain")]
ATTN_ARMS += [(2, 3, 70, d, "both") for d in (16, 48, 96, 112)]


@pytest.mark.parametrize("B,H,S,d,arm", ATTN_ARMS)
def test_text_attn_fwd(B, H, S, d, arm):
    """O against float64 softmax attention (mask and bias inside the scores) on the same bf16 operands, every row within the
    budget of tests/attn_refs.py for O.  The construction is test_vit_attn_fwd's: q | k | v sit inside a buffer whose guard row
    above and below and guard columns left and right hold inf / NaN; O likewise: nothing may leak in, and the guards come back
    bit for bit.  The bias table is drawn with standard deviation 2, so that it matters.  `plain` (no mask, no table) must
    equal mgx_vit_attn_fwd bit for bit.  Power: the causal arm rejects the non-causal reference, the bias arm the bias-free
    reference and the reference whose table is reversed along k - q (S > 1: a single key has weight 1 whatever its score);
    `both` (mask and table at once: no tower uses it, the entry point allows it) rejects the reference without either."""
    ops = _ops()
    w = H * d
    g = _g(B * 1000 + H * 100 + S + d)
    ld, ldo = 3 * w + 2 * GUARD, w + 2 * GUARD
    buf = torch.full((B * S + 2, ld), float("nan"), dtype=BF, device="cuda")
    buf[:, 0::2] = float("inf")
    q, k, v = (torch.randn(B, S, H, d, device="cuda", generator=g) for _ in range(3))
    buf[1:-1, GUARD:GUARD + 3 * w] = torch.cat([t.reshape(B * S, w) for t in (q, k, v)], 1).to(BF)
    obuf = torch.full((B * S + 2, ldo), float("nan"), dtype=BF, device="cuda")
    obuf[:, 1::2] = float("-inf")
    buf0, obuf0 = buf.clone(), obuf.clone()
    scale = d ** -0.5
    causal = arm in ("causal", "both")
    table = 2.0 * torch.randn(H, 2 * S - 1, device="cuda", generator=g) if arm in ("bias", "both") else None
    assert ops.text_attn_fwd(buf[1, GUARD:], ld, obuf[1, GUARD:], ldo, B, H, S, d, scale, causal=causal, rel_bias=table)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), buf0.view(torch.int16))                    # the operands are only read
    guard = torch.ones_like(obuf, dtype=torch.bool)
    guard[1:-1, GUARD:GUARD + w] = False
    assert torch.equal(obuf.view(torch.int16)[guard], obuf0.view(torch.int16)[guard])
    qkv = buf[1:-1, GUARD:GUARD + 3 * w]
    qb, kb, vb = (t.reshape(B, S, H, d).transpose(1, 2).to(F64) for t in qkv.split(w, -1))
    out = obuf[1:-1, GUARD:GUARD + w].reshape(B, S, H, d).transpose(1, 2)
    ref = T.attention(qb, kb, vb, scale, causal, table)
    budget = T.attention_budget(qb, kb, vb, scale, causal, table)
    ok, msg = A.rows_close(out, ref, budget, A.C["O"])
    print(f"text attention {B, H, S, d} {arm}: {msg}")
    assert ok, msg
    if arm == "plain":
        vit = obuf0.clone()
        assert ops.vit_attn_fwd(buf[1, GUARD:], ld, vit[1, GUARD:], ldo, B, H, S, d, scale)
        assert torch.equal(vit.view(torch.int16), obuf.view(torch.int16))
    if S > 1 and arm == "causal":
        assert not A.rows_close(out, T.attention(qb, kb, vb, scale), budget, A.C["O"])[0]
    if S > 1 and arm == "bias":
        assert not A.rows_close(out, T.attention(qb, kb, vb, scale), budget, A.C["O"])[0]
        assert not A.rows_close(out, T.attention(qb, kb, vb, scale, table=table.flip(1)), budget, A.C["O"])[0]
    if arm == "both":
        assert not A.rows_close(out, T.attention(qb, kb, vb, scale, False, table), budget, A.C["O"])[0]
        assert not A.rows_close(out, T.attention(qb, kb, vb, scale, True), budget, A.C["O"])[0]


def test_text_attn_fwd_causal_with_a_table_and_refusals():
    """Both flags at once (no tower uses it, the entry point allows it), a table of the wrong shape, S > 4096."""
    from mixgrpo_amd._lib import MgxError
    ops = _ops()
    B, H, S, d = 1, 2, 70, 64
    g = _g(9)
    qkv = torch.randn(B * S, 3 * H * d, device="cuda", generator=g).to(BF)
    table = 2.0 * torch.randn(H, 2 * S - 1, device="cuda", generator=g)
    o = torch.full((B * S + 1, H * d), SENT, dtype=BF, device="cuda")
    assert ops.text_attn_fwd(qkv, 3 * H * d, o, H * d, B, H, S, d, 0.125, causal=True, rel_bias=table)
    qb, kb, vb = (t.reshape(B, S, H, d).transpose(1, 2).to(F64) for t in qkv.split(H * d, -1))
    out = o[:B * S].reshape(B, S, H, d).transpose(1, 2)
    A.assert_ok(A.rows_close(out, T.attention(qb, kb, vb, 0.125, True, table), T.attention_budget(qb, kb, vb, 0.125, True, table), A.C["O"]))
    assert (o[B * S] == SENT).all()
    o.fill_(SENT)
    with pytest.raises(ValueError, match="rel_bias"):
        ops.text_attn_fwd(qkv, 3 * H * d, o, H * d, B, H, S, d, 0.125, rel_bias=table[:, :-1].contiguous())
    assert ops.text_attn_fwd(qkv, 192, o, 64, 1, 1, 4097, 64, 0.125, causal=True) is False   # rc 1 before anything is launched
    with pytest.raises(MgxError):
        ops.text_attn_fwd(qkv, 3 * 72, o, 72, 1, 1, 2, 72, 0.1, causal=True)                 # head dim % 16
    torch.cuda.synchronize()
    assert (o == SENT).all()


# --------------------------------------------------------------------------------------------------------------- RMS norm
@pytest.mark.parametrize("M", [1, 17, 514])
@pytest.mark.parametrize("D", [64, 768, 4096])
def test_rms_norm_affine(D, M):
    """Strided input (ldx = D + 8) and output (ldy = D + 16) with sentinel columns.  Budget by the rule of
    test_layer_norm_affine: one bf16 ulp plus c 2^-24 |ref|, c = D / 64 sequential terms of a lane + the 6-level wave tree +
    rsqrt and the two products (+ 8 in all).  Nothing cancels here -- the sum of squares has positive terms only -- so the
    fp32 part is relative to the result itself."""
    ops = _ops()
    g = _g(D * 7 + M)
    eps = 1e-6
    xs = torch.full((M, D + 8), SENT, dtype=BF, device="cuda")
    xs[:, :D] = (torch.randn(M, D, device="cuda", generator=g) * 1.5 + 0.3).to(BF)
    gamma = 1 + 0.2 * torch.randn(D, device="cuda", generator=g)
    y = torch.full((M + 1, D + 16), SENT, dtype=BF, device="cuda")
    ops.rms_norm_affine(xs, D + 8, gamma, y, D + 16, M, D, eps)
    x = xs[:, :D]
    ref = T.rms_norm(x, gamma, eps)
    bound = (D / 64 + 8) * N.U32 * ref.abs()
    N.assert_ok(N.bf16_close(y[:M, :D], ref, bound))
    assert (y[M] == SENT).all() and (y[:, D:] == SENT).all()
    # power: a mean of squares that misses the row's last 64 elements (one element per lane) is rejected; so is LayerNorm
    if D > 64:
        x64 = x.to(F64)
        wrong = x64 * torch.rsqrt(x64[:, :D - 64].pow(2).sum(-1, keepdim=True) / D + eps) * gamma.to(F64)
        assert not N.bf16_close(y[:M, :D], wrong, bound)[0]
    assert not N.bf16_close(y[:M, :D], N.layer_norm(x, eps)[0] * gamma.to(F64), bound)[0]
    # in place
    ops.rms_norm_affine(xs, D + 8, gamma, xs, D + 8, M, D, eps)
    assert torch.equal(xs[:, :D], y[:M, :D]) and (xs[:, D:] == SENT).all()


def test_rms_norm_affine_refuses_wide_rows():
    from mixgrpo_amd._lib import MgxError
    ops = _ops()
    x = torch.zeros(2, 4160, dtype=BF, device="cuda")
    y = torch.full((2, 4160), SENT, dtype=BF, device="cuda")
    for D in (4160, 96):
        with pytest.raises(MgxError):
            ops.rms_norm_affine(x, 4160, torch.ones(4160, device="cuda"), y, 4160, 2, D, 1e-6)
    torch.cuda.synchronize()
    assert (y == SENT).all()


# ------------------------------------------------------------------------------------------------------------ activations
def _act_values():
    """`_act_values` of tests/test_hip_clip.py, plus large magnitudes"""
    v = torch.cat([torch.linspace(-30, 30, 6001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-10, -1e-10, 1e-3, -1e-3, 1e4, -1e4]),
                   torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3,
                   torch.tensor([1e8, -1e8, 1e20, -1e20, 1e30, -1e30, 300.0, -300.0])])
    return v.to(BF)


@pytest.mark.parametrize("act", ["gelu", "quick_gelu", "gelu_tanh"])
def test_gated_act_rows(act):
    """y = bf16(act(a) * b) against float64, out of place (three different strides) and in place (y = a).  Tolerance: one bf16
    ulp of the exact product -- the single rounding -- plus the fp32 evaluation error (16 + 4 |t|) 2^-24 |ref|: every one of
    the three is x times a quantity that decays like exp(-t) for x < 0 (t = x^2 / 2 for the exact GELU, 1.702 |x| for the
    quick one, 2 sqrt(2 / pi) |x + 0.044715 x^3| for the tanh form), and an fp32 argument carries a relative error of a few
    2^-24, which exp turns into |t| times as much; 16 covers the function's own few ulps, the sum, the quotient and the product
    with b.  t is capped at 200: beyond it the result is below every bf16 number.  At most 1 % of the elements may differ from
    the correctly rounded value.  The tanh form must keep its relative precision for x < 0, where 1 + tanh cancels."""
    ops = _ops()
    code = {"gelu": ops.ACT_GELU, "quick_gelu": ops.ACT_QUICK_GELU, "gelu_tanh": ops.ACT_GELU_TANH}[act]
    v = _act_values()
    n = v.numel()
    Ncol = 64
    M = (n + Ncol - 1) // Ncol
    a = torch.full((M, Ncol + 8), SENT, dtype=BF, device="cuda")
    flat = torch.zeros(M * Ncol, dtype=BF)
    flat[:n] = v
    a[:, :Ncol] = flat.view(M, Ncol).cuda()
    b = torch.full((M, Ncol + 24), SENT, dtype=BF, device="cuda")
    bv = (1.5 * torch.randn(M, Ncol, device="cuda", generator=_g(1))).to(BF)
    bv[:, 0], bv[:, 1], bv[:, 2] = 1.0, -1.0, 0.0
    b[:, :Ncol] = bv
    y = torch.full((M + 1, Ncol + 4), SENT, dtype=BF, device="cuda")
    ops.gated_act_rows(a, Ncol + 8, b, Ncol + 24, y, Ncol + 4, M, Ncol, code)
    x = a[:, :Ncol].to(F64)
    ref = T.ACT[act](x) * bv.to(F64)
    t = {"gelu": x * x / 2, "quick_gelu": 1.702 * x.abs(),
         "gelu_tanh": 2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3).abs()}[act].clamp(max=200.0)
    bound = (16 + 4 * t) * N.U32 * ref.abs()
    N.assert_ok(N.bf16_close(y[:M, :Ncol], ref, bound))
    assert (y[M] == SENT).all() and (y[:, Ncol:] == SENT).all()
    # power: the other two activations, and the ungated one, are rejected
    for other in T.ACT:
        if other != act:
            assert not N.bf16_close(y[:M, :Ncol], T.ACT[other](x) * bv.to(F64), bound)[0]
    assert not N.bf16_close(y[:M, :Ncol], T.ACT[act](x), bound)[0]
    ops.gated_act_rows(a, Ncol + 8, b, Ncol + 24, a, Ncol + 8, M, Ncol, code)
    assert torch.equal(a[:, :Ncol], y[:M, :Ncol]) and (a[:, Ncol:] == SENT).all() and (b[:, Ncol:] == SENT).all()
    assert torch.equal(b[:, :Ncol], bv)


# ------------------------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("with_pos", [True, False])
def test_token_embed(with_pos):
    """Exactly bf16(table[ids].float() + pos[s]); an out-of-range id raises a ValueError that names it and its position before
    anything is launched: the output keeps its sentinels."""
    ops = _ops()
    B, S, D, V = 3, 7, 200, 50
    g = _g(4)
    table = torch.randn(V, D, device="cuda", generator=g).to(BF)
    pos = torch.randn(S + 2, D, device="cuda", generator=g) if with_pos else None
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(6))
    ids[0, 0], ids[2, 6] = 0, V - 1
    x = torch.full((B * S + 1, D), SENT, dtype=BF, device="cuda")
    ops.token_embed(ids, table, pos, x[:B * S])
    want = table[ids.cuda()].float()
    if with_pos:
        want = want + pos[:S]
    assert torch.equal(x[:B * S].view(B, S, D), want.to(BF)) and (x[B * S] == SENT).all()
    ops.token_embed(ids.cuda().int(), table, pos, x[:B * S])             # ids already on the device, int32
    assert torch.equal(x[:B * S].view(B, S, D), want.to(BF))
    x.fill_(SENT)
    for bad, where in ((V, (1, 3)), (-1, (2, 0)), (1 << 20, (0, 6))):
        wrong = ids.clone()
        wrong[where] = bad
        with pytest.raises(ValueError) as e:
            ops.token_embed(wrong, table, pos, x[:B * S])
        assert str(bad) in str(e.value) and str(where) in str(e.value)
    with pytest.raises(ValueError):
        ops.token_embed(ids.float(), table, pos, x[:B * S])
    torch.cuda.synchronize()
    assert (x == SENT).all()


# ----------------------------------------------------------------------------------------------------------------- towers
def _clip_ids(V, B=3, S=77, seed=2):
    """ids below V - 1 with the end-of-text token, the largest id, at positions 9, 30 and 76"""
    ids = torch.randint(3, V - 1, (B, S), generator=torch.Generator().manual_seed(seed))
    for b, p in enumerate((9, 30, 76)[:B]):
        ids[b, p] = V - 1
    return ids


def _tower_configs():
    from mixgrpo_amd.clip_text import ClipTextConfig as C
    from mixgrpo_amd.t5 import T5EncoderConfig as E
    return {"clip_w128_quick": (C(vocab=1000, width=128, layers=2, heads=2, mlp_width=256, embed_dim=64, act="quick_gelu"), 77),
            "clip_w1024_gelu": (C(vocab=1000, width=1024, layers=2, heads=16, mlp_width=4096, embed_dim=1024, act="gelu"), 77),
            "t5_d128_s130": (E(vocab=1000, d_model=128, layers=2, heads=2, d_kv=64, d_ff=256), 130),
            "t5_xxl_width_s512": (E(vocab=1000, d_model=4096, layers=2, heads=64, d_kv=64, d_ff=10240), 512)}


@pytest.mark.parametrize("name", ["clip_w128_quick", "clip_w1024_gelu", "t5_d128_s130", "t5_xxl_width_s512"])
def test_towers_against_restatement(name):
    """Batches of 1 and 3.  Tolerance, the rule of tests/test_hip_clip.py::test_tower_against_restatement: the restatement's
    bf16-emulation arm against its float64 arm is the error the number format causes; the HIP result may be at most twice that
    in relative L2 and in 1 - cosine (per prompt).  The rows of the batch of 3 equal the one-at-a-time rows bit for bit, and a
    second run gives the same bits.  CLIP: the projected pooled rows (`encode_text`, not normalised) and `pooled_output`; T5:
    the whole `last_hidden_state`."""
    from mixgrpo_amd import clip_text, t5
    c, S = _tower_configs()[name]
    if name.startswith("clip"):
        sd = clip_text.synthetic_state_dict(c, seed=5, device="cuda")
        tower = clip_text.ClipTextTower(c, device="cuda").load_state_dict(sd)
        P, _ = clip_text.convert_state_dict(sd, c)
        ids = _clip_ids(c.vocab)
        run = lambda i: tower.encode_text(i, normalize=False)
        restate = lambda emu: T.clip_text_tower(P, c, ids, emulate_bf16=emu, device="cuda")[0]
        shape = (3, c.embed_dim)
    else:
        sd = t5.synthetic_state_dict(c, seed=5, device="cuda")
        tower = t5.T5Encoder(c, device="cuda").load_state_dict(sd)
        P = t5.convert_state_dict(sd, c)
        ids = torch.randint(0, c.vocab, (3, S), generator=torch.Generator().manual_seed(2))
        ids[1, S // 3:] = 0                                                 # a padded prompt: its padding is attended
        run = tower.encode
        restate = lambda emu: T.t5_encoder(P, c, ids, emulate_bf16=emu, device="cuda")
        shape = (3, S, c.d_model)
    got = run(ids)
    assert tuple(got.shape) == shape and got.dtype == (F32 if name.startswith("clip") else BF)
    assert torch.equal(got, run(ids))
    for i in range(3):
        assert torch.equal(run(ids[i:i + 1])[0], got[i]), f"prompt {i} alone differs from its row of the batch"
    f64, emu = restate(False), restate(True)
    flat = lambda t: t.reshape(3, -1)
    fig = {"emu_rel_l2": T.rel_l2(emu, f64), "hip_rel_l2": T.rel_l2(got, f64),
           "emu_1mcos": T.one_minus_cos(flat(emu), flat(f64)), "hip_1mcos": T.one_minus_cos(flat(got), flat(f64))}
    _record(**{f"tower_{name}": fig})
    assert torch.isfinite(got).all()
    assert fig["hip_rel_l2"] <= 2 * fig["emu_rel_l2"], fig
    assert fig["hip_1mcos"] <= 2 * fig["emu_1mcos"], fig
    if name.startswith("clip"):
        pooled = tower.pooled_output(ids)
        assert pooled.shape == (3, c.width) and pooled.dtype == BF
        pf, pe = (T.clip_text_tower(P, c, ids, emulate_bf16=e, device="cuda")[1] for e in (False, True))
        assert T.rel_l2(pooled, pf) <= 2 * T.rel_l2(pe, pf)
        nrm = tower.encode_text(ids)                                        # normalize=True
        assert torch.allclose(nrm.to(F64), got.to(F64) / got.to(F64).norm(dim=-1, keepdim=True), rtol=0, atol=1e-6)
        # the other pooling rule: the first position that holds eos_token_id
        other = clip_text.ClipTextTower(replace(c, eos_token_id=7), device="cuda").load_state_dict(sd)
        ids7 = ids.clone()
        ids7[0, 12] = ids7[1, 5] = ids7[1, 40] = ids7[2, 76] = 7
        n = other._hidden(ids7).view(3, S, c.width).clone()
        assert torch.equal(other.pooled_output(ids7), torch.stack([n[0, 12], n[1, 5], n[2, 76]]))
    else:
        with pytest.raises(NotImplementedError):
            tower.encode(ids, attention_mask=torch.ones_like(ids))


# ---------------------------------------------------------------------------------------------------------------- rewards
def test_rewards_from_prompts(tmp_path):
    """ClipReward with TextTowerFeatures (synthetic towers, a stub tokenizer) gives exactly the scores of the same reward with
    a TextFeatureCache built offline from the same tower's encode_text."""
    from mixgrpo_amd.clip_text import ClipTextConfig, ClipTextTower
    from mixgrpo_amd.clip_vision import ClipVisionConfig, ClipVisionTower
    from mixgrpo_amd.rewards import KINDS, ClipReward, TextFeatureCache, TextTowerFeatures, build_text_feature_cache
    vision = ClipVisionTower(ClipVisionConfig(width=128, layers=2, heads=2, mlp_width=256, image_size=56, embed_dim=64,
                                              act="quick_gelu"), device="cuda").init_synthetic(seed=7)
    text = ClipTextTower(ClipTextConfig(vocab=300, width=128, layers=2, heads=2, mlp_width=256, embed_dim=64), device="cuda")
    text.init_synthetic(seed=8)
    tok = T.stub_tokenizer(77, 300)
    prompts = ["a red cube", "a blue sphere", "a red cube", "a green cone on a long, long table"]
    images = (torch.rand(4, 3, 64, 64, device="cuda", generator=_g(4)) * 2 - 1).to(BF)
    path = build_text_feature_cache(prompts, lambda ps: text.encode_text(tok(ps)), str(tmp_path / "t.safetensors"), batch_size=2)
    cache, live = TextFeatureCache(path), TextTowerFeatures(text, tok)
    for k in KINDS:
        a, b = ClipReward(vision, live, k)(images, prompts), ClipReward(vision, cache, k)(images, prompts)
        assert a == b and len(a) == 4 and all(math.isfinite(v) for v in a), (k, a, b)
        assert a[0] != a[1]
    assert ClipReward(vision, live, KINDS[0])(images[:1], ["never seen before"])[0] != 0.0       # no KeyError: encoded on the spot
    with pytest.raises(KeyError):
        ClipReward(vision, cache, KINDS[0])(images[:1], ["never seen before"])


# ----------------------------------------------------------------------------------------------------------------- timing
def test_text_timing_is_recorded():
    """Milliseconds per call at batch 8 after a warm-up, device events around 20 calls, synthetic weights: CLIP_L_TEXT whole
    (12 layers, 77 tokens) and a 4-layer T5-XXL-width encoder at S = 512; per-layer TFLOP/s from the layers' GEMM and attention
    FLOPs (causal attention counted whole).  Recorded, no threshold: nobody has measured these kernels."""
    from mixgrpo_amd.clip_text import CLIP_L_TEXT, ClipTextTower
    from mixgrpo_amd.t5 import T5_XXL, T5Encoder
    REPS, B = 20, 8
    c = CLIP_L_TEXT
    clip = ClipTextTower(c, device="cuda").init_synthetic(seed=0)
    e = replace(T5_XXL, layers=4)
    enc = T5Encoder(e, device="cuda").init_synthetic(seed=0)
    M = B * 77
    clip_flops = 2.0 * M * (4 * c.width * c.width + 2 * c.width * c.mlp_width) + 4.0 * B * c.heads * 77 * 77 * c.head_dim
    M = B * 512
    t5_flops = 2.0 * M * (4 * e.d_model * e.inner + 3 * e.d_model * e.d_ff) + 4.0 * B * e.heads * 512 * 512 * e.d_kv
    jobs = (("clip_l_text", lambda: clip.encode_text(_clip_ids(c.vocab, B)), c.layers, clip_flops),
            ("t5_xxl_width_4_layers_s512", lambda: enc.encode(torch.randint(0, e.vocab, (B, 512), generator=torch.Generator().manual_seed(1))),
             e.layers, t5_flops))
    fig = {}
    for tag, call, layers, flops in jobs:
        out = call()                                                        # warm-up: buffers, kernel loads, the bias table
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            out = call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / REPS
        fig[tag] = {"ms_per_call_batch8": ms, "per_layer_tflops": flops * layers / (ms * 1e-3) / 1e12}   # `flops` is one layer's
        assert torch.isfinite(out.float()).all()
        assert math.isfinite(ms) and ms > 0 and fig[tag]["per_layer_tflops"] > 0
    _record(text_batch8=fig)
