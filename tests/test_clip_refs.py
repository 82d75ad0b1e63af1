"""CPU checks of the CLIP reward path: the float64 restatement (tests/clip_refs.py) against transformers' CLIPModel, torch's
antialiased bicubic and PIL; the key conversion; the host logic of mixgrpo_amd/rewards.py with a stub tower."""
import json

import pytest
import torch

import clip_refs as R
from mixgrpo_amd import clip_vision as CV
from mixgrpo_amd import rewards as RW
from mixgrpo_amd.reward_adapter import compute_reward

F64 = torch.float64
TINY = {"d80_gelu": CV.ClipVisionConfig(width=320, layers=2, heads=4, mlp_width=640, patch_size=14, image_size=56, embed_dim=64, act="gelu"),
        "d64_quick": CV.ClipVisionConfig(width=128, layers=2, heads=2, mlp_width=256, patch_size=14, image_size=56, embed_dim=32,
                                         act="quick_gelu")}
RESIZES = R.RESIZES


# transformers is imported in a child process: importing it pulls in torch.distributed's FSDP / sharding modules, which changes
# how later tests of this suite that create process groups see their file store torn down
_HF_CHILD = r"""
import json, sys, torch
from transformers import CLIPConfig, CLIPModel
cases, out = json.loads(sys.argv[1]), sys.argv[2]
res = {}
for name, c in cases.items():
    torch.manual_seed(0)
    cfg = CLIPConfig(vision_config=dict(hidden_size=c["width"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                                        intermediate_size=c["mlp_width"], patch_size=c["patch_size"], image_size=c["image_size"],
                                        hidden_act=c["act"], layer_norm_eps=c["layer_norm_eps"]),
                     text_config=dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                      vocab_size=100, max_position_embeddings=8),
                     projection_dim=c["embed_dim"])
    m = CLIPModel(cfg).double().eval()
    with torch.no_grad():                              # biases and LayerNorm parameters away from their 0 / 1 initial values
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        px = torch.randn(3, 3, c["image_size"], c["image_size"], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        ref = m.get_image_features(pixel_values=px)
    ref = ref if torch.is_tensor(ref) else ref.pooler_output
    res[name] = {"sd": {k: v.detach().clone() for k, v in m.state_dict().items()}, "px": px, "ref": ref.detach(),
                 "logit_scale": float(m.logit_scale), "config": m.config.to_dict()}
torch.save(res, out)
"""


@pytest.fixture(scope="module")
def hf_cases(tmp_path_factory):
    import subprocess
    import sys
    out = str(tmp_path_factory.mktemp("hf") / "cases.pt")
    cases = {k: {f: getattr(c, f) for f in ("width", "layers", "heads", "mlp_width", "patch_size", "image_size", "embed_dim", "act",
                                            "layer_norm_eps")} for k, c in TINY.items()}
    r = subprocess.run([sys.executable, "-c", _HF_CHILD, json.dumps(cases), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out, weights_only=False)


@pytest.mark.parametrize("name", sorted(TINY))
def test_restatement_matches_transformers(name, hf_cases):
    """The float64 tower on the converted HF state dict against CLIPModel.get_image_features (`.pooler_output`, or the tensor
    if that is what this transformers returns) of a tiny random-init CLIPModel in float64: relative error <= 1e-10.  Pins the
    HF key names (convert_state_dict refuses a missing or unknown vision tensor)."""
    c, h = TINY[name], hf_cases[name]
    P, ls = CV.convert_state_dict(h["sd"], c)
    assert ls == pytest.approx(h["logit_scale"])
    out = R.tower(P, c, h["px"])
    assert out.shape == h["ref"].shape == (3, c.embed_dim)
    assert R.rel_l2(out, h["ref"]) <= 1e-10
    assert CV.config_from_json(h["config"]) == c


def _to_open_clip(sd, c):
    """Re-key an HF state dict to open_clip's names (in_proj fused, proj transposed)."""
    hf, oc = CV._hf_names(c), CV._open_clip_names(c)
    out = {}
    for name, src in hf.items():
        t = torch.cat([sd[k] for k in src], 0) if isinstance(src, tuple) else sd[src]
        out[oc[name]] = t.t().contiguous() if name == "proj.weight" else t
    out["logit_scale"] = sd["logit_scale"]
    out["text_projection"] = torch.zeros(2, 2)             # text-tower tensors are ignored
    return out


def test_key_conversion_round_trip():
    c = TINY["d80_gelu"]
    sd = CV.synthetic_state_dict(c, seed=3)
    a, la = CV.convert_state_dict(sd, c)
    b, lb = CV.convert_state_dict(_to_open_clip(sd, c), c)
    assert la == lb and set(a) == set(b) == set(CV.param_shapes(c))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    oc = _to_open_clip(sd, c)
    assert oc["visual.transformer.resblocks.1.attn.in_proj_weight"].shape == (3 * c.width, c.width)
    assert oc["visual.proj"].shape == (c.width, c.embed_dim)


def test_missing_and_unknown_tensors_are_named():
    c = TINY["d64_quick"]
    sd = CV.synthetic_state_dict(c)
    gone = "vision_model.encoder.layers.1.mlp.fc2.bias"
    bad = {k: v for k, v in sd.items() if k != gone}
    bad["vision_model.encoder.layers.7.mlp.fc1.weight"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        CV.convert_state_dict(bad, c)
    assert gone in str(e.value) and "layers.7.mlp.fc1.weight" in str(e.value)
    with pytest.raises(ValueError, match="wrong shapes"):
        CV.convert_state_dict(dict(sd, **{"visual_projection.weight": torch.zeros(3, 3)}), c)


# ------------------------------------------------------------------------------------------------------------- preprocess
_image = R.make_image


@pytest.mark.parametrize("hw,R_", RESIZES)
def test_resize_matches_torch_antialias_bicubic(hw, R_):
    """The restatement's pre-rounding resize equals F.interpolate(mode="bicubic", antialias=True) in float64 to 1e-9 (levels)."""
    H, W = hw
    lv = R.image_levels(_image(H, W, "noise")).to(F64)
    oh, ow = R.resized_hw(H, W, R_)
    ref = torch.nn.functional.interpolate(lv[None], size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)[0]
    assert (R.resize(lv, oh, ow) - ref).abs().max().item() <= 1e-9


def test_identity_resize_is_exact():
    lv = R.image_levels(_image(56, 56, "noise")).to(F64)
    assert torch.equal(R.resize(lv, 56, 56), lv)
    assert torch.equal(R.resize_matrix(56, 56), torch.eye(56, dtype=F64))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("hw,R_", RESIZES)
def test_resize_within_one_level_of_pil(hw, R_, kind, record_property):
    """Against PIL itself, Image.fromarray(a).resize(..., BICUBIC): at most 1 level apart.  PIL rounds to uint8 between its two
    passes (and works in fixed point), the kernel's rule does not; the share of differing pixels is recorded, not capped
    (measured on these images at 1024 -> 224: 9.8 % on noise, 5.6 % on the smooth image; 16 .. 22 % at 64 x 48 -> 28 and when
    upscaling 100 -> 224)."""
    import numpy as np
    from PIL import Image
    H, W = hw
    img = _image(H, W, kind)
    a = R.image_levels(img).permute(1, 2, 0).numpy().astype("uint8")
    oh, ow = R.resized_hw(H, W, R_)
    pil = torch.from_numpy(np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC)).copy()).permute(2, 0, 1).to(F64)
    ours = R.resize(R.image_levels(img).to(F64), oh, ow).round().clamp(0, 255)
    diff = (ours - pil).abs()
    share = (diff > 0).double().mean().item()
    record_property("share_differing", share)
    print(f"{H}x{W} -> {R_} {kind}: {100 * share:.2f} % of the pixels differ from PIL, max {diff.max().item():.0f} level")
    assert diff.max().item() <= 1


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("hw,R_", R.RESIZES + [((56, 56), 56)])
def test_reference_ties_stay_within_the_cap(hw, R_, kind):
    """tests/test_hip_clip.py excludes the pixels whose float64 pre-rounding value lies within 1e-3 of a tie from its exact
    comparison and caps their share at 0.5 %; a uniform fractional part gives 0.2 %.  The reference alone, on the images that
    test uses, stays within the cap (at scale 1 every value is an integer: no pixel is excluded)."""
    H, W = hw
    r = R.preprocess(_image(H, W, kind), R_, 14, CV.OPENAI_MEAN, CV.OPENAI_STD)
    share = (R.tie_distance(r["pre"]) < R.TIE).double().mean().item()
    assert share <= R.TIE_CAP, share
    if hw == (56, 56):
        assert share == 0.0


def test_preprocess_layout_and_pil_path():
    """Patch rows: row py g + px, column c p p + dy p + dx; and clip_vision.pil_pixel_values (the host path for PIL images)
    follows the same crop and normalisation."""
    from PIL import Image
    c = TINY["d64_quick"]
    img = _image(64, 80, "smooth")
    r = R.preprocess(img, c.image_size, c.patch_size, c.image_mean, c.image_std)
    p, g = c.patch_size, c.grid
    assert r["patches"].shape == (g * g, 3 * p * p)
    assert r["patches"][1 * g + 2, 2 * p * p + 3 * p + 5] == r["pixels"][2, 1 * p + 3, 2 * p + 5]
    pil = Image.fromarray(R.image_levels(img).permute(1, 2, 0).numpy().astype("uint8"))
    pv = CV.pil_pixel_values(pil, c)
    assert pv.shape == (3, c.image_size, c.image_size)
    step = 1 / (255 * min(c.image_std))
    assert (pv.double() - r["pixels"]).abs().max().item() <= step * 1.001      # PIL's own resize: one level at most


# -------------------------------------------------------------------------------------------------------------- host logic
class _StubTower:
    """encode_image returns fixed features: rewards.py's host logic without a GPU"""

    def __init__(self, feats, logit_scale=4.0):
        self.device, self.logit_scale, self.feats, self.calls = torch.device("cpu"), logit_scale, feats, 0

    def encode_image(self, images=None, pixel_values=None, normalize=True):
        self.calls += 1
        return self.feats[:len(images)]


def _cpu_cosine(monkeypatch):
    """ops.cosine_score is a HIP launch; on the CPU its float64 restatement stands in, so that what ClipReward asks of it (the
    operands and the three parameters per kind) is what the formulas are checked on."""
    def fake(f, t, out, logit_scale=1.0, mean=0.0, std=1.0):
        out.copy_(R.score(f, t.expand(f.shape[0], -1), logit_scale, mean, std))
    monkeypatch.setattr(RW.ops, "cosine_score", fake)


def test_score_formulas_and_unknown_prompt(monkeypatch):
    _cpu_cosine(monkeypatch)
    g = torch.Generator().manual_seed(0)
    feats, text = torch.randn(3, 16, generator=g), torch.randn(4, 16, generator=g)
    prompts = ["a cat", "a dog", "a \"quoted\" bird", "unused"]
    cache = RW.TextFeatureCache(features=text, prompts=prompts)
    tower = _StubTower(feats, logit_scale=4.0)
    cos = torch.nn.functional.cosine_similarity(feats.double(), text[:3].double(), dim=-1)
    images = [torch.zeros(3, 8, 8)] * 3
    for kind in ("HPSClipRewardModel", "CLIPScoreRewardModel"):
        out = RW.ClipReward(tower, cache, kind)(images, prompts[:3])
        assert isinstance(out, list) and all(isinstance(v, float) for v in out)
        assert torch.allclose(torch.tensor(out, dtype=F64), cos, atol=1e-6)
    out = RW.ClipReward(tower, cache, "PickScoreRewardModel", mean=18.0, std=8.0)(images, prompts[:3])
    assert torch.allclose(torch.tensor(out, dtype=F64), (torch.tensor(4.0).exp().double() * cos - 18.0) / 8.0, atol=1e-5)
    calls = tower.calls
    with pytest.raises(KeyError) as e:
        RW.ClipReward(tower, cache, "HPSClipRewardModel")(images[:1], ["a fish called 'Wanda'"])
    assert "a fish called 'Wanda'" in str(e.value).replace("\\'", "'") and tower.calls == calls      # nothing ran
    with pytest.raises(ValueError):
        RW.ClipReward(tower, cache, "UnifiedRewardModel")
    with pytest.raises(ValueError, match="logit_scale"):
        RW.ClipReward(_StubTower(feats, logit_scale=None), cache, "PickScoreRewardModel")
    # the reward adapter's contract with ClipReward values
    models = {k: RW.ClipReward(tower, cache, k) for k in ("HPSClipRewardModel", "PickScoreRewardModel")}
    total, ok, per, _ = compute_reward(images, prompts[:3], models, {"HPSClipRewardModel": 2.0, "PickScoreRewardModel": 0.5})
    assert ok == [1, 1, 1] and set(per) == set(models)
    for i in range(3):
        assert total[i] == pytest.approx(2.0 * per["HPSClipRewardModel"][i] + 0.5 * per["PickScoreRewardModel"][i])


@pytest.mark.parametrize("ext", [".safetensors", ".pt"])
def test_text_feature_cache_files(tmp_path, ext):
    prompts = ["one", "two", "one", "three"]
    calls = []

    def encode_text(ps):
        calls.append(list(ps))
        return torch.tensor([[float(len(p)), 1.0] for p in ps])
    path = RW.build_text_feature_cache(prompts, encode_text, str(tmp_path / ("t" + ext)), batch_size=2)
    assert calls == [["one", "two"], ["three"]]
    c = RW.TextFeatureCache(path)
    assert c.prompts == ["one", "two", "three"]
    assert torch.equal(c.lookup(["three", "one"], "cpu"), torch.tensor([[5.0, 1.0], [3.0, 1.0]]))
    with pytest.raises(KeyError, match="four"):
        c.rows(["four"])


def test_builtin_rewards_from_a_config(tmp_path, monkeypatch):
    """The plugin factory: tower directory (config.json + safetensors in HF names) and text cache named by a JSON file that
    MGX_REWARD_CONFIG points at; towers of one directory are shared; the trainer's flag list is untouched."""
    from safetensors.torch import save_file
    c = TINY["d64_quick"]
    d = tmp_path / "tower"
    d.mkdir()
    sd = {k: v.contiguous() for k, v in CV.synthetic_state_dict(c).items()}
    save_file(sd, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps({"projection_dim": c.embed_dim, "vision_config": dict(
        hidden_size=c.width, num_hidden_layers=c.layers, num_attention_heads=c.heads, intermediate_size=c.mlp_width,
        patch_size=c.patch_size, image_size=c.image_size, hidden_act=c.act)}))
    (d / "preprocessor_config.json").write_text(json.dumps({"image_mean": [0.5, 0.5, 0.5], "image_std": [0.25, 0.25, 0.25]}))
    tf = RW.build_text_feature_cache(["p"], lambda ps: torch.ones(len(ps), c.embed_dim), str(tmp_path / "text.safetensors"))
    cfg = tmp_path / "rewards.json"
    cfg.write_text(json.dumps({"HPSClipRewardModel": {"tower_dir": str(d), "text_features": tf, "device": "cpu"},
                               "PickScoreRewardModel": {"tower_dir": str(d), "text_features": tf, "device": "cpu", "std": 4.0}}))
    monkeypatch.delenv(RW.CONFIG_ENV, raising=False)
    with pytest.raises(ValueError, match=RW.CONFIG_ENV):
        RW.builtin_rewards(None)
    monkeypatch.setenv(RW.CONFIG_ENV, str(cfg))
    from mixgrpo_amd.train_grpo_flux import load_reward_plugin
    models = load_reward_plugin("mixgrpo_amd.rewards:builtin_rewards", None)
    assert set(models) == {"HPSClipRewardModel", "PickScoreRewardModel"}
    hps, pick = models["HPSClipRewardModel"], models["PickScoreRewardModel"]
    assert hps.tower is pick.tower and hps.text_features is pick.text_features
    assert hps.tower.config == CV.ClipVisionConfig(**{**c.__dict__, "image_mean": (0.5, 0.5, 0.5), "image_std": (0.25, 0.25, 0.25)})
    assert pick.score_params() == (pytest.approx(100.0, rel=1e-6), 18.0, 4.0) and hps.score_params() == (1.0, 0.0, 1.0)
    assert set(hps.tower.P) == set(CV.param_shapes(c))
    cfg.write_text(json.dumps({"UnifiedRewardModel": {"tower_dir": str(d), "text_features": tf}}))
    with pytest.raises(ValueError, match="UnifiedRewardModel"):
        RW.builtin_rewards(None)


def test_presets():
    h, l = CV.VIT_H_14, CV.VIT_L_14
    assert (h.width, h.layers, h.heads, h.mlp_width, h.patch_size, h.image_size, h.embed_dim, h.act) == (1280, 32, 16, 5120, 14, 224, 1024, "gelu")
    assert (l.width, l.layers, l.heads, l.mlp_width, l.patch_size, l.image_size, l.embed_dim, l.act) == (1024, 24, 16, 4096, 14, 224, 768, "quick_gelu")
    assert h.head_dim == 80 and l.head_dim == 64 and h.tokens == l.tokens == 257
    assert h.image_mean == (0.48145466, 0.4578275, 0.40821073) and h.image_std == (0.26862954, 0.26130258, 0.27577711)
    assert h.layer_norm_eps == 1e-5
    with pytest.raises(ValueError):
        CV.ClipVisionConfig(width=1280, heads=12).check()           # head dim 106.67
