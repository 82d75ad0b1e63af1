"""CPU checks of the ImageReward path: the float64 restatements (tests/blip_refs.py) against transformers' BlipVisionModel and
BlipTextModel, the key conversions of mixgrpo_amd/image_reward.py, the attention and head references, and the host logic of
image_reward.ImageRewardModel and rewards.builtin_rewards with stubs."""
import json
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import blip_refs as BR
from mixgrpo_amd import image_reward as IR
from mixgrpo_amd import rewards as RW

F64 = torch.float64
VIS = IR.BlipVisionConfig(width=128, layers=2, heads=2, mlp_width=256, patch_size=16, image_size=48)      # 10 tokens
TXT = IR.BertXattnConfig(vocab=100, positions=40, width=128, layers=2, heads=2, mlp_width=256, encoder_width=128)
S = 12
LENGTHS = torch.tensor([12, 1, 7])


def text_ids(seed=3):
    return torch.randint(1, 100, (3, S), generator=torch.Generator().manual_seed(seed))


# transformers is imported in a child process, as in tests/test_clip_refs.py and for the reason given there
_HF_CHILD = r"""
import sys, torch
from transformers import BlipTextConfig, BlipVisionConfig, BlipVisionModel
from transformers.models.blip.modeling_blip_text import BlipTextModel
job, out = torch.load(sys.argv[1], weights_only=False), sys.argv[2]

def perturb(m):                                        # biases and norm weights away from their 0 / 1 initial values
    for n, p in m.named_parameters():
        if p.dim() == 1:
            p.add_(0.1 * torch.randn_like(p))

v, t = job["vis"], job["txt"]
torch.manual_seed(0)
vm = BlipVisionModel(BlipVisionConfig(hidden_size=v["width"], intermediate_size=v["mlp_width"], num_hidden_layers=v["layers"],
                                      num_attention_heads=v["heads"], image_size=v["image_size"], patch_size=v["patch_size"],
                                      hidden_act="gelu", layer_norm_eps=v["layer_norm_eps"], initializer_range=0.1)).double().eval()
tm = BlipTextModel(BlipTextConfig(vocab_size=t["vocab"], hidden_size=t["width"], encoder_hidden_size=t["encoder_width"],
                                  intermediate_size=t["mlp_width"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"],
                                  max_position_embeddings=t["positions"], hidden_act="gelu", layer_norm_eps=t["layer_norm_eps"],
                                  is_decoder=True, initializer_range=0.1, hidden_dropout_prob=0.0,
                                  attention_probs_dropout_prob=0.0, pad_token_id=0, bos_token_id=1, sep_token_id=2, eos_token_id=2),
                   add_pooling_layer=False).double().eval()
with torch.no_grad():
    perturb(vm)
    perturb(tm)
    for n, p in vm.named_parameters():                 # the class token and the position embeddings start at zero / tiny
        if n.endswith("class_embedding") or n.endswith("position_embedding"):
            p.copy_(0.5 * torch.randn_like(p))
    tokens = vm(pixel_values=job["pixels"]).last_hidden_state
    mask = (torch.arange(job["ids"].shape[1])[None] < job["lengths"][:, None]).long()
    run = lambda ids: tm(input_ids=ids, attention_mask=mask, encoder_hidden_states=tokens,
                         encoder_attention_mask=torch.ones(tokens.shape[:2], dtype=torch.long), is_decoder=False).last_hidden_state
    hidden = run(job["ids"])
    hidden_other_padding = run(job["ids_other_padding"])
sd = {"vision_model." + k: p.detach().clone() for k, p in vm.state_dict().items()}
sd.update({"text_encoder." + k: p.detach().clone() for k, p in tm.state_dict().items()})
torch.save({"sd": sd, "tokens": tokens, "hidden": hidden, "hidden_other_padding": hidden_other_padding}, out)
"""


def _head_sd(seed=4):
    g = torch.Generator().manual_seed(seed)
    sd, k = {}, TXT.width
    for n, layer in zip(IR.HEAD_WIDTHS, IR.HEAD_LAYERS):
        sd[f"mlp.layers.{layer}.weight"] = torch.randn(n, k, generator=g, dtype=F64) * k ** -0.5
        sd[f"mlp.layers.{layer}.bias"] = torch.randn(n, generator=g, dtype=F64) * 0.1
        k = n
    return sd


@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    d = tmp_path_factory.mktemp("hf_blip")
    ids = text_ids()
    other = ids.clone()
    pad = torch.arange(S)[None] >= LENGTHS[:, None]
    other[pad] = torch.randint(1, 100, (int(pad.sum()),), generator=torch.Generator().manual_seed(9))
    job = {"vis": dict(VIS.__dict__), "txt": dict(TXT.__dict__), "ids": ids, "ids_other_padding": other, "lengths": LENGTHS,
           "pixels": torch.randn(3, 3, VIS.image_size, VIS.image_size, generator=torch.Generator().manual_seed(5), dtype=F64)}
    torch.save(job, str(d / "job.pt"))
    r = subprocess.run([sys.executable, "-c", _HF_CHILD, str(d / "job.pt"), str(d / "res.pt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = torch.load(str(d / "res.pt"), weights_only=False)
    res["job"] = job
    res["sd"].update(_head_sd())
    return res


# ------------------------------------------------------------------------------------------------------------ restatements
def test_restatements_match_transformers(hf):
    """The float64 encoders on the converted state dict against tiny random-init float64 BlipVisionModel and BlipTextModel
    (is_decoder=True in the config so that the cross-attention exists, called with is_decoder=False, the image tokens as
    encoder_hidden_states, an all-ones encoder mask and a ragged attention_mask): every image token, and the real rows of every
    prompt, to a relative error of 1e-10, the bound of the same comparison in tests/test_text_refs.py.  Pins the transformers
    key names (convert_state_dict refuses a missing or unknown tensor), the missing pre-LayerNorm, the patch bias, the order
    self-attention / cross-attention / FFN, the post-LayerNorms and the exclusion of the padding keys."""
    job = hf["job"]
    P = IR.convert_state_dict(hf["sd"], VIS, TXT)
    assert set(P) == set(IR.param_shapes(VIS, TXT))
    assert IR.vision_config_from_state_dict(hf["sd"]) == VIS
    tokens = BR.vit_encoder(P, VIS, job["pixels"])
    assert tokens.shape == hf["tokens"].shape == (3, VIS.tokens, VIS.width)
    assert BR.rel_l2(tokens, hf["tokens"]) <= 1e-10
    hidden = BR.text_encoder(P, TXT, job["ids"], LENGTHS, hf["tokens"])
    assert hidden.shape == hf["hidden"].shape == (3, S, TXT.width)
    real = torch.arange(S)[None] < LENGTHS[:, None]
    assert BR.rel_l2(hidden[real], hf["hidden"][real]) <= 1e-10
    # transformers' own real rows do not see the padding ids, and neither do the restatement's
    assert torch.equal(hf["hidden"][real], hf["hidden_other_padding"][real])
    again = BR.text_encoder(P, TXT, job["ids_other_padding"], LENGTHS, hf["tokens"])
    assert torch.equal(again[real], hidden[real]) and not torch.equal(again[~real], hidden[~real])
    # power: lengths ignored, and lengths off by one, are seen on the real rows of the prompts they change
    full = BR.text_encoder(P, TXT, job["ids"], torch.full((3,), S), hf["tokens"])
    assert BR.rel_l2(full[1:][real[1:]], hf["hidden"][1:][real[1:]]) > 1e-6
    off = BR.text_encoder(P, TXT, job["ids"], (LENGTHS - 1).clamp(min=1), hf["tokens"])
    assert BR.rel_l2(off[0], hf["hidden"][0]) > 1e-6
    # the emulation arm moves the result by about a bf16 step, not more
    emu = BR.text_encoder(P, TXT, job["ids"], LENGTHS, BR.vit_encoder(P, VIS, job["pixels"], emulate_bf16=True), emulate_bf16=True)
    assert 1e-4 < BR.rel_l2(emu[real], hidden[real]) < 5e-2


def test_score_is_head_of_token_zero(hf):
    job = hf["job"]
    P = IR.convert_state_dict(hf["sd"], VIS, TXT)
    s, hidden, tokens = BR.score(P, VIS, TXT, job["pixels"], job["ids"], LENGTHS, IR.MEAN, IR.STD)
    assert s.shape == (3,) and BR.rel_l2(tokens, hf["tokens"]) <= 1e-10
    assert torch.allclose(s, (BR.head_layers(P, hf["hidden"][:, 0]) - IR.MEAN) / IR.STD, rtol=0, atol=1e-9)
    assert IR.MEAN == 0.16717362830052426 and IR.STD == 1.0333394966054072


# ---------------------------------------------------------------------------------------------------------- key conversion
def _to_upstream(sd):
    """Re-key a format (a) state dict to upstream ImageReward's names."""
    a, b = IR._hf_names(VIS, TXT), IR._upstream_names(VIS, TXT)
    out = {}
    for name, src in a.items():
        for x, y in zip(src if isinstance(src, tuple) else (src,), b[name] if isinstance(b[name], tuple) else (b[name],)):
            out[y] = sd[x]
    out["blip.text_encoder.embeddings.position_ids"] = torch.arange(40)[None]          # a buffer, not a tensor of the layout
    return out


def test_key_conversion_round_trip():
    sd = IR.synthetic_state_dict(VIS, TXT, seed=3)
    up = _to_upstream(sd)
    assert "blip.visual_encoder.blocks.1.attn.qkv.weight" in up and "blip.visual_encoder.cls_token" in up
    assert "blip.text_encoder.encoder.layer.1.crossattention.self.key.weight" in up and "mlp.layers.7.bias" in up
    assert up["blip.visual_encoder.pos_embed"].shape == (1, VIS.tokens, VIS.width)
    a, b = IR.convert_state_dict(sd, VIS, TXT), IR.convert_state_dict(up, VIS, TXT)
    assert set(a) == set(b) == set(IR.param_shapes(VIS, TXT))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert IR.vision_config_from_state_dict(up) == VIS
    w = TXT.width                                                                   # the stacked cross-attention weight
    assert torch.equal(a["txt.xkv.weight"][2 * w + w:4 * w], sd["text_encoder.encoder.layer.1.crossattention.self.value.weight"])
    assert torch.equal(a["txt.layers.0.qkv.bias"][w:2 * w], sd["text_encoder.encoder.layer.0.attention.self.key.bias"])


@pytest.mark.parametrize("upstream", [False, True])
def test_missing_misshapen_and_unknown_tensors_are_named(upstream):
    sd = IR.synthetic_state_dict(VIS, TXT)
    conv = _to_upstream if upstream else (lambda d: dict(d))
    v, t = ("blip.visual_encoder.", "blip.text_encoder.") if upstream else ("vision_model.", "text_encoder.")
    gone = t + "encoder.layer.1.crossattention.output.LayerNorm.bias"
    bad = {k: x for k, x in conv(sd).items() if k != gone}
    extra = v + ("blocks.9.mlp.fc1.weight" if upstream else "encoder.layers.9.mlp.fc1.weight")
    bad[extra] = torch.zeros(1)
    bad["mlp.layers.3.weight"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        IR.convert_state_dict(bad, VIS, TXT)
    assert gone in str(e.value) and extra in str(e.value) and "mlp.layers.3.weight" in str(e.value)
    name = "mlp.layers.4.weight"
    with pytest.raises(ValueError, match="wrong shapes") as e:
        IR.convert_state_dict(dict(conv(sd), **{name: torch.zeros(3, 3)}), VIS, TXT)
    assert name in str(e.value)
    assert "position_ids" not in str(IR.convert_state_dict(dict(conv(sd), **{t + "embeddings.position_ids": torch.zeros(1, 4)}), VIS, TXT).keys())


def test_from_pretrained_reads_both_file_formats(tmp_path):
    """.safetensors and .pt (weights_only) + med_config.json; the image encoder's sizes come from the tensors, encoder_width
    from the image encoder; matrices and biases of the encoders in bf16, LayerNorm parameters, class token, position embeddings
    and the head in fp32."""
    from safetensors.torch import save_file
    sd = {k: v.contiguous() for k, v in IR.synthetic_state_dict(VIS, TXT, seed=1).items()}
    med = dict(vocab_size=TXT.vocab, max_position_embeddings=TXT.positions, hidden_size=TXT.width, num_hidden_layers=TXT.layers,
               num_attention_heads=TXT.heads, intermediate_size=TXT.mlp_width, layer_norm_eps=1e-12, hidden_act="gelu",
               encoder_width=768)
    (tmp_path / "med_config.json").write_text(json.dumps(med))
    save_file(sd, str(tmp_path / "m.safetensors"))
    torch.save(_to_upstream(sd), str(tmp_path / "m.pt"))
    models = [IR.ImageRewardModel.from_pretrained(str(tmp_path / f), str(tmp_path / "med_config.json"), device="cpu")
              for f in ("m.safetensors", "m.pt")]
    for m in models:
        assert m.vision.config == VIS and m.text.config == TXT and (m.mean, m.std) == (IR.MEAN, IR.STD)
        P, Q = m.vision.P, m.text.P
        assert P["patch.weight"].dtype == P["patch.bias"].dtype == P["layers.1.fc1.bias"].dtype == torch.bfloat16
        assert P["cls"].dtype == P["pos"].dtype == P["ln_post.weight"].dtype == P["layers.0.ln_2.bias"].dtype == torch.float32
        assert Q["tok"].dtype == Q["xkv.weight"].dtype == Q["layers.1.xq.bias"].dtype == torch.bfloat16
        assert Q["pos"].dtype == Q["ln_emb.weight"].dtype == Q["layers.1.ln_x.bias"].dtype == torch.float32
        assert Q["xkv.weight"].shape == (TXT.layers * 2 * TXT.width, VIS.width)
        assert [tuple(W.shape) for W, _ in m.head] == [(1024, 128), (128, 1024), (64, 128), (16, 64), (1, 16)]
        assert all(W.dtype == b.dtype == torch.float32 for W, b in m.head)
    for k in models[0].text.P:
        assert torch.equal(models[0].text.P[k], models[1].text.P[k]), k
    with pytest.raises(ValueError, match="hidden_act"):
        IR.bert_config_from_json(dict(med, hidden_act="relu"), 128)


def test_presets():
    v, t = IR.BLIP_VIT_L_16, IR.BERT_BASE_XATTN
    assert (v.width, v.layers, v.heads, v.mlp_width, v.patch_size, v.image_size, v.layer_norm_eps, v.act) == (1024, 24, 16, 4096, 16, 224, 1e-6, "gelu")
    assert v.tokens == 197 and v.head_dim == 64 and v.image_mean[0] == pytest.approx(0.48145466)
    assert (t.vocab, t.positions, t.width, t.layers, t.heads, t.mlp_width, t.layer_norm_eps, t.encoder_width) == (30524, 512, 768, 12, 12, 3072, 1e-12, 1024)
    v.check()
    t.check()
    with pytest.raises(ValueError):
        IR.BertXattnConfig(width=768, heads=10).check()
    with pytest.raises(ValueError, match="encoder_width"):
        IR.ImageRewardModel(VIS, IR.BertXattnConfig(encoder_width=256), device="cpu")


# ------------------------------------------------------------------------------------------------- attention and the head
def test_attention_reference_with_lengths_is_truncation():
    """The reference with lengths equals the plain reference on K and V cut to each sample's length, whatever the excluded
    rows hold; without lengths it is the plain softmax attention."""
    g = torch.Generator().manual_seed(0)
    B, H, Sq, Skv, d = 3, 2, 5, 9, 16
    q, k, v = torch.randn(B, H, Sq, d, generator=g), torch.randn(B, H, Skv, d, generator=g), torch.randn(B, H, Skv, d, generator=g)
    lens = torch.tensor([9, 1, 4])
    for b in range(B):
        k[b, :, lens[b]:] = float("nan")
        v[b, :, lens[b]:] = float("inf")
    out, budget = BR.xattention(q, k, v, 0.3, lens), BR.xattention_budget(q, k, v, 0.3, lens)
    assert torch.isfinite(out).all() and torch.isfinite(budget).all() and (budget > 0).all()
    for b in range(B):
        n = int(lens[b])
        want = BR.R.attention(q[b], k[b, :, :n], v[b, :, :n], 0.3)
        assert torch.allclose(out[b], want, rtol=0, atol=1e-14)
    assert torch.equal(out[1], v[1, :, :1].to(F64).expand(-1, Sq, -1))              # one key: weight 1
    clean = torch.randn(B, H, Skv, d, generator=g)
    assert torch.allclose(BR.xattention(q, clean, clean, 0.3), BR.R.attention(q, clean, clean, 0.3), rtol=0, atol=1e-14)


def test_head_layer_by_layer_equals_the_composition():
    P = {k.replace("mlp.layers.", "head."): v for k, v in _head_sd().items()}
    P = {f"head.{j}.{p}": P[f"head.{n}.{p}"] for j, n in enumerate(IR.HEAD_LAYERS) for p in ("weight", "bias")}
    h0 = torch.randn(7, TXT.width, generator=torch.Generator().manual_seed(2), dtype=F64)
    a, b = BR.head_layers(P, h0), BR.head_composed(P, h0)
    assert a.shape == (7,) and (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())
    assert a.abs().max().item() > 1e-3


# ------------------------------------------------------------------------------------------------------------- host logic
def test_stub_tokenizer_is_ragged():
    tok = BR.stub_tokenizer(35, 1000)
    ids, lens = tok(["", "a cat", "x" * 34, "y" * 80])
    assert ids.shape == (4, 35) and lens.tolist() == [1, 6, 35, 35]
    assert ids[0].tolist() == [1] + [0] * 34 and (ids[1, 6:] == 0).all() and (ids[2:] != 0).all()
    assert int(ids.max()) < 1000 and int(ids.min()) >= 0


class _Recorder:
    made = []

    @classmethod
    def from_pretrained(cls, checkpoint, med_config, tokenizer=None, mean=None, std=None, device="cuda"):
        cls.made.append(dict(checkpoint=checkpoint, med_config=med_config, tokenizer=tokenizer, mean=mean, std=std, device=device))
        return cls()


def test_builtin_rewards_parses_an_image_reward_entry(tmp_path, monkeypatch):
    """The entry's own `checkpoint` / `med_config`, or `args.image_reward_path` / `args.image_reward_med_config`; an entry
    without a checkpoint and no args raises; KINDS is still the three CLIP kinds."""
    assert RW.KINDS == ("HPSClipRewardModel", "CLIPScoreRewardModel", "PickScoreRewardModel") and RW.IMAGE_REWARD == "ImageRewardModel"
    monkeypatch.setattr(IR, "ImageRewardModel", _Recorder)
    _Recorder.made = []
    cfg = tmp_path / "rewards.json"
    monkeypatch.setenv(RW.CONFIG_ENV, str(cfg))
    cfg.write_text(json.dumps({"ImageRewardModel": {"checkpoint": "/w/ImageReward.pt", "med_config": "/w/med_config.json",
                                                    "tokenizer_dir": "/w/tok", "mean": 0.5, "std": 2.0, "device": "cpu"}}))
    models = RW.builtin_rewards(None)
    assert list(models) == ["ImageRewardModel"] and isinstance(models["ImageRewardModel"], _Recorder)
    assert _Recorder.made == [dict(checkpoint="/w/ImageReward.pt", med_config="/w/med_config.json", tokenizer="/w/tok", mean=0.5,
                                   std=2.0, device="cpu")]
    cfg.write_text(json.dumps({"ImageRewardModel": {}}))
    args = SimpleNamespace(image_reward_path="/a/ImageReward.pt", image_reward_med_config="/a/med_config.json")
    RW.builtin_rewards(args)
    assert _Recorder.made[-1] == dict(checkpoint="/a/ImageReward.pt", med_config="/a/med_config.json", tokenizer="/a", mean=IR.MEAN,
                                      std=IR.STD, device="cuda")
    with pytest.raises(ValueError, match=r"ImageRewardModel lacks \['checkpoint', 'med_config'\]"):
        RW.builtin_rewards(None)
    cfg.write_text(json.dumps({"ImageRewardModel": {"med_config": "/w/med_config.json"}}))
    with pytest.raises(ValueError, match=r"ImageRewardModel lacks \['checkpoint'\]"):
        RW.builtin_rewards(SimpleNamespace())
    cfg.write_text(json.dumps({"SomethingElse": {}}))
    with pytest.raises(ValueError, match="SomethingElse"):
        RW.builtin_rewards(None)


def test_scorer_checks_its_inputs_before_any_launch():
    """Mismatched counts, a missing tokenizer and a tokenizer that returns the wrong shapes raise on the host (a CPU model: any
    launch would raise MgxError instead)."""
    m = IR.ImageRewardModel(VIS, TXT, device="cpu")
    img = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="2 images for 1 prompts"):
        m([img, img], ["a"])
    with pytest.raises(ValueError, match="tokenizer"):
        m([img], ["a"])
    m.tokenizer = lambda prompts: (torch.zeros(len(prompts) + 1, 35, dtype=torch.long), torch.ones(len(prompts), dtype=torch.long))
    with pytest.raises(ValueError, match="tokenizer returned"):
        m([img], ["a"])
    m.tokenizer = BR.stub_tokenizer()
    with pytest.raises(RuntimeError, match="not loaded"):
        m([img], ["a"])


def test_import_does_not_import_transformers():
    code = "import sys, mixgrpo_amd.image_reward, mixgrpo_amd.rewards; assert 'transformers' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
