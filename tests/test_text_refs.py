"""CPU checks of the text-encoder path: the float64 restatements (tests/text_refs.py) against transformers'
CLIPTextModelWithProjection and T5EncoderModel, the relative-position table against transformers' own bucket function, the key
conversions, and the host logic of text_encoders.py, preprocess_flux_embedding.py and rewards.TextTowerFeatures with stubs."""
import json
import subprocess
import sys

import pytest
import torch

import text_refs as T
from mixgrpo_amd import clip_text as CT
from mixgrpo_amd import clip_vision as CV
from mixgrpo_amd import rewards as RW
from mixgrpo_amd import t5 as T5

F64 = torch.float64
CLIP_TINY = dict(vocab=100, context=77, width=128, layers=2, heads=2, mlp_width=256, embed_dim=32)
CLIP_CASES = {"legacy_eos2": CT.ClipTextConfig(**CLIP_TINY, act="quick_gelu", eos_token_id=2),
              "eos7": CT.ClipTextConfig(**CLIP_TINY, act="gelu", eos_token_id=7)}
T5_TINY = T5.T5EncoderConfig(vocab=100, d_model=128, layers=2, heads=2, d_kv=64, d_ff=256)
T5_S = 130                     # distances pass max_exact = 8 and run through the log buckets up to max_distance = 128


def clip_ids(name):
    """[3, 77] ids.  legacy_eos2: ids below 99 with the largest id, 99, at positions 9 and 30 (and at 76, the row's end).
    eos7: ids that avoid 7, then id 7 at 12 / twice (5 and 40: the first counts) / at 76."""
    g = torch.Generator().manual_seed(3)
    if name == "legacy_eos2":
        ids = torch.randint(3, 99, (3, 77), generator=g)
        ids[0, 9] = ids[1, 30] = ids[2, 76] = 99
        return ids
    ids = torch.randint(8, 100, (3, 77), generator=g)
    ids[0, 12] = ids[1, 5] = ids[1, 40] = ids[2, 76] = 7
    return ids


# transformers is imported in a child process, as in tests/test_clip_refs.py and for the reason given there
_HF_CHILD = r"""
import json, sys, torch
from transformers import CLIPTextConfig, CLIPTextModelWithProjection, T5Config, T5EncoderModel
from transformers.models.t5.modeling_t5 import T5Attention
job, out = torch.load(sys.argv[1], weights_only=False), sys.argv[2]
res = {"clip": {}}

def perturb(m):                                        # biases and norm weights away from their 0 / 1 initial values
    for n, p in m.named_parameters():
        if p.dim() == 1:
            p.add_(0.1 * torch.randn_like(p))

for name, c in job["clip"].items():
    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=c["vocab"], hidden_size=c["width"], intermediate_size=c["mlp_width"],
                         projection_dim=c["embed_dim"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                         max_position_embeddings=c["context"], hidden_act=c["act"], layer_norm_eps=c["layer_norm_eps"],
                         eos_token_id=c["eos_token_id"], bos_token_id=0, pad_token_id=1)
    m = CLIPTextModelWithProjection(cfg).double().eval()
    with torch.no_grad():
        perturb(m)
        embeds = m(input_ids=c["ids"]).text_embeds
        pooled = m.text_model(input_ids=c["ids"]).pooler_output
    res["clip"][name] = {"sd": {k: v.detach().clone() for k, v in m.state_dict().items()}, "embeds": embeds.detach(),
                         "pooled": pooled.detach(), "config": m.config.to_dict()}
c = job["t5"]
torch.manual_seed(1)
cfg = T5Config(vocab_size=c["vocab"], d_model=c["d_model"], d_kv=c["d_kv"], num_heads=c["heads"], d_ff=c["d_ff"],
               num_layers=c["layers"], feed_forward_proj="gated-gelu", relative_attention_num_buckets=c["num_buckets"],
               relative_attention_max_distance=c["max_distance"], layer_norm_epsilon=c["eps"], dropout_rate=0.0)
m = T5EncoderModel(cfg).double().eval()
with torch.no_grad():
    perturb(m)
    for n, p in m.named_parameters():                  # T5's init makes the attention nearly uniform: give the scores some size
        if n.endswith("SelfAttention.q.weight"):
            p.mul_(8.0)
    hidden = m(input_ids=c["ids"]).last_hidden_state
res["t5"] = {"sd": {k: v.detach().clone() for k, v in m.state_dict().items()}, "hidden": hidden.detach(),
             "config": m.config.to_dict()}
S = job["bucket_S"]
pos = torch.arange(S)
res["buckets"] = T5Attention._relative_position_bucket(pos[None, :] - pos[:, None], bidirectional=True, num_buckets=32,
                                                       max_distance=128)
torch.save(res, out)
"""


@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    d = tmp_path_factory.mktemp("hf_text")
    fields = ("vocab", "context", "width", "layers", "heads", "mlp_width", "embed_dim", "act", "layer_norm_eps", "eos_token_id")
    job = {"clip": {k: dict({f: getattr(c, f) for f in fields}, ids=clip_ids(k)) for k, c in CLIP_CASES.items()},
           "t5": dict(T5_TINY.__dict__, ids=torch.randint(0, 100, (2, T5_S), generator=torch.Generator().manual_seed(5))),
           "bucket_S": 512}
    torch.save(job, str(d / "job.pt"))
    r = subprocess.run([sys.executable, "-c", _HF_CHILD, str(d / "job.pt"), str(d / "res.pt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = torch.load(str(d / "res.pt"), weights_only=False)
    res["job"] = job
    return res


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("name", sorted(CLIP_CASES))
def test_clip_text_restatement_matches_transformers(name, hf):
    """The float64 tower on the converted HF state dict against a tiny random-init float64 CLIPTextModelWithProjection:
    `text_embeds` and the pooled rows (`text_model(...).pooler_output`) to a relative error of 1e-10.  Pins the HF key names
    (convert_state_dict refuses a missing or unknown text tensor), the causal mask and both pooling rules."""
    c, h = CLIP_CASES[name], hf["clip"][name]
    ids = clip_ids(name)
    want = {"legacy_eos2": [9, 30, 76], "eos7": [12, 5, 76]}[name]
    assert CT.pooled_positions(ids, c.eos_token_id).tolist() == want
    P, ls = CT.convert_state_dict(h["sd"], c)
    assert ls is None and set(P) == set(CT.param_shapes(c))
    embeds, pooled = T.clip_text_tower(P, c, ids)
    assert embeds.shape == h["embeds"].shape == (3, c.embed_dim) and pooled.shape == h["pooled"].shape == (3, c.width)
    assert T.rel_l2(embeds, h["embeds"]) <= 1e-10
    assert T.rel_l2(pooled, h["pooled"]) <= 1e-10
    assert CT.config_from_json(h["config"]) == c
    # the mask itself, on equal scores: query q spreads evenly over the keys 0 .. q
    full = torch.softmax(T.scores(torch.ones(1, 1, 4, 8), torch.ones(1, 1, 4, 8), 1.0, causal=True), -1)
    assert torch.equal(full[0, 0], torch.tensor([[1, 0, 0, 0], [1 / 2, 1 / 2, 0, 0], [1 / 3] * 3 + [0], [1 / 4] * 4], dtype=F64))


def test_t5_restatement_matches_transformers(hf):
    """The float64 encoder against a tiny float64 T5EncoderModel (gated-gelu) at S = 130: relative error <= 1e-10.  Pins the key
    names, the fused q | k | v and wi_0 | wi_1 orders, the unscaled scores, the bias direction (key - query) and `gelu_new`.
    transformers' T5LayerNorm takes its mean of squares in float32 whatever the model's dtype; the restatement reproduces that
    one step for this comparison (`hf_variance`), and its plain float64 arm -- the one the kernels are held to -- stays within
    1e-5 of it (measured: 4.5e-7)."""
    h = hf["t5"]
    ids = hf["job"]["t5"]["ids"]
    P = T5.convert_state_dict(h["sd"], T5_TINY)
    assert set(P) == set(T5.param_shapes(T5_TINY))
    out = T.t5_encoder(P, T5_TINY, ids, hf_variance=True)
    assert out.shape == h["hidden"].shape == (2, T5_S, 128)
    assert T.rel_l2(out, h["hidden"]) <= 1e-10
    assert T.rel_l2(T.t5_encoder(P, T5_TINY, ids), h["hidden"]) <= 1e-5
    assert T5.config_from_json(h["config"]) == T5_TINY
    # power: the table reversed along delta (query - key) is seen
    flipped = T.t5_encoder(P, T5_TINY, ids.flip(1), hf_variance=True).flip(1)           # reversing the sequence reverses every distance
    assert T.rel_l2(flipped, h["hidden"]) > 1e-6
    x = torch.linspace(-6, 6, 1001, dtype=F64)
    assert (T.gelu_tanh(x) - T.gelu_tanh_stable(x)).abs().max().item() <= 1e-15


def test_relative_bias_table_equals_transformers_buckets(hf):
    """t5_relative_bias_table against transformers' own _relative_position_bucket gathered through a random weight, S = 512:
    every (h, delta) exactly equal, and every (q, k) pair of the [S, S] bias reads its own entry of the compact table."""
    S, H = 512, 5
    buckets = hf["buckets"]                                              # [q, k] -> bucket of k - q
    assert buckets.shape == (S, S) and int(buckets.max()) == 31 and int(buckets.min()) == 0
    w = torch.randn(32, H, generator=torch.Generator().manual_seed(2))
    table = T5.t5_relative_bias_table(w, S, 32, 128)
    assert table.shape == (H, 2 * S - 1) and table.dtype == torch.float32
    full = w[buckets].permute(2, 0, 1)                                   # T5Attention.compute_bias: [H, q, k]
    assert torch.equal(T.bias_matrix(table, S), full.to(F64))
    pos = torch.arange(S)
    for delta in (-(S - 1), -129, -128, -127, -9, -8, -7, -1, 0, 1, 7, 8, 9, 127, 128, 129, S - 1):
        q = int(pos[(pos + delta >= 0) & (pos + delta < S)][0])
        assert torch.equal(table[:, delta + S - 1], full[:, q, q + delta])
    assert torch.equal(T5.relative_position_bucket(pos[None, :] - pos[:, None]), buckets)


def test_t5_refuses_an_attention_mask_and_other_feed_forwards():
    enc = T5.T5Encoder(T5_TINY, device="cpu")
    with pytest.raises(NotImplementedError, match="attention_mask"):
        enc.encode(torch.zeros(1, 4, dtype=torch.long), attention_mask=torch.ones(1, 4))
    with pytest.raises(ValueError, match="gated-gelu"):
        T5.config_from_json({"feed_forward_proj": "relu", "vocab_size": 10, "d_model": 64, "num_layers": 1, "num_heads": 1,
                             "d_kv": 64, "d_ff": 64})


# ---------------------------------------------------------------------------------------------------------- key conversion
def _to_open_clip(sd, c):
    """Re-key an HF text state dict to open_clip's names (in_proj fused, text_projection transposed)."""
    hfn, oc = CT._hf_names(c), CT._open_clip_names(c)
    out = {}
    for name, src in hfn.items():
        t = torch.cat([sd[k] for k in src], 0) if isinstance(src, tuple) else sd[src]
        out[oc[name]] = t.t().contiguous() if name == "proj.weight" else t
    out["logit_scale"] = sd["logit_scale"]
    out["attn_mask"] = torch.zeros(2, 2)                                  # open_clip's buffer: not a tensor of the layout
    return out


def test_key_conversion_round_trip():
    c = CLIP_CASES["legacy_eos2"]
    sd = CT.synthetic_state_dict(c, seed=3)
    oc = _to_open_clip(sd, c)
    a, la = CT.convert_state_dict(sd, c)
    b, lb = CT.convert_state_dict(oc, c)
    assert la == lb == pytest.approx(4.605170185988092) and set(a) == set(b) == set(CT.param_shapes(c))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert oc["transformer.resblocks.1.attn.in_proj_weight"].shape == (3 * c.width, c.width)
    assert oc["text_projection"].shape == (c.width, c.embed_dim) and oc["positional_embedding"].shape == (77, c.width)


def test_missing_and_unknown_tensors_are_named():
    c = CLIP_CASES["eos7"]
    sd = CT.synthetic_state_dict(c)
    gone = "text_model.encoder.layers.1.mlp.fc2.bias"
    bad = {k: v for k, v in sd.items() if k != gone}
    bad["text_model.encoder.layers.7.mlp.fc1.weight"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        CT.convert_state_dict(bad, c)
    assert gone in str(e.value) and "layers.7.mlp.fc1.weight" in str(e.value)
    with pytest.raises(ValueError, match="wrong shapes"):
        CT.convert_state_dict(dict(sd, **{"text_projection.weight": torch.zeros(3, 3)}), c)
    # a bare CLIPTextModel (FLUX's text_encoder) has no text_projection: allowed
    P, _ = CT.convert_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"}, c)
    assert "proj.weight" not in P and set(P) | {"proj.weight"} == set(CT.param_shapes(c))
    t = T5.synthetic_state_dict(T5_TINY)
    assert t["shared.weight"] is t["encoder.embed_tokens.weight"]
    gone = "encoder.block.1.layer.1.DenseReluDense.wi_1.weight"
    bad = {k: v for k, v in t.items() if k != gone}
    bad["encoder.block.9.layer.0.layer_norm.weight"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        T5.convert_state_dict(bad, T5_TINY)
    assert gone in str(e.value) and "block.9.layer.0.layer_norm.weight" in str(e.value)
    only = {k: v for k, v in t.items() if k != "shared.weight"}          # either name of the tied table will do
    assert torch.equal(T5.convert_state_dict(only, T5_TINY)["tok"], t["shared.weight"])


def test_a_whole_clip_model_converts_into_both_towers():
    """Vision tensors in a text conversion are ignored, and text tensors in a vision conversion still are, in both key formats."""
    ct = CLIP_CASES["legacy_eos2"]
    cv = CV.ClipVisionConfig(width=128, layers=1, heads=2, mlp_width=256, image_size=28, embed_dim=32, act="quick_gelu")
    text, vision = CT.synthetic_state_dict(ct, seed=1), CV.synthetic_state_dict(cv, seed=2)
    both = {**vision, **text}
    Pt, ls = CT.convert_state_dict(both, ct)
    Pv, lv = CV.convert_state_dict(both, cv)
    assert set(Pt) == set(CT.param_shapes(ct)) and set(Pv) == set(CV.param_shapes(cv)) and ls == lv
    assert torch.equal(Pt["tok"], text["text_model.embeddings.token_embedding.weight"])
    # open_clip names: `visual.*` next to the bare text names
    hfv, ocv = CV._hf_names(cv), CV._open_clip_names(cv)
    oc = _to_open_clip(text, ct)
    for name, src in hfv.items():
        t = torch.cat([vision[k] for k in src], 0) if isinstance(src, tuple) else vision[src]
        oc[ocv[name]] = t.t().contiguous() if name == "proj.weight" else t
    Pt2, _ = CT.convert_state_dict(oc, ct)
    Pv2, _ = CV.convert_state_dict(oc, cv)
    for k in Pt:
        assert torch.equal(Pt[k], Pt2[k]), k
    for k in Pv:
        assert torch.equal(Pv[k], Pv2[k]), k


def test_from_pretrained_reads_config_and_safetensors(tmp_path):
    """config.json in transformers' form (flat for a text model, nested for a CLIPModel) + *.safetensors; a FLUX-style bare
    CLIPTextModel without text_projection loads, and only its encode_text is refused."""
    from safetensors.torch import save_file
    c = CLIP_CASES["eos7"]
    flat = dict(vocab_size=c.vocab, max_position_embeddings=c.context, hidden_size=c.width, num_hidden_layers=c.layers,
                num_attention_heads=c.heads, intermediate_size=c.mlp_width, hidden_act=c.act, eos_token_id=7)
    sd = {k: v.contiguous() for k, v in CT.synthetic_state_dict(c).items()}
    for name, cfg, drop in (("nested", {"projection_dim": c.embed_dim, "text_config": flat}, ()),
                            ("flat", dict(flat, projection_dim=c.embed_dim), ("text_projection.weight",))):
        d = tmp_path / name
        d.mkdir()
        (d / "config.json").write_text(json.dumps(cfg))
        save_file({k: v for k, v in sd.items() if k not in drop}, str(d / "model.safetensors"))
        tower = CT.ClipTextTower.from_pretrained(str(d), device="cpu")
        assert tower.config == c and set(tower.P) == set(CT.param_shapes(c)) - {"proj.weight" if drop else None}
        assert tower.P["tok"].dtype == torch.bfloat16 and tower.P["pos"].dtype == tower.P["layers.1.ln_2.bias"].dtype == torch.float32
    d = tmp_path / "t5"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(vocab_size=100, d_model=128, num_layers=2, num_heads=2, d_kv=64, d_ff=256,
                                                   feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
                                                   relative_attention_max_distance=128, layer_norm_epsilon=1e-6)))
    t = T5.synthetic_state_dict(T5_TINY)
    save_file({k: v.contiguous() for k, v in t.items() if k != "encoder.embed_tokens.weight"}, str(d / "model.safetensors"))
    enc = T5.T5Encoder.from_pretrained(str(d), device="cpu")
    assert enc.config == T5_TINY and set(enc.P) == set(T5.param_shapes(T5_TINY))
    assert enc.P["rel_bias"].dtype == enc.P["ln_final.weight"].dtype == torch.float32 and enc.P["layers.0.wi.weight"].shape == (512, 128)
    table = enc.bias_table(130)
    assert table.shape == (2, 259) and enc.bias_table(130) is table                     # built once per S
    (tmp_path / "empty").mkdir()
    (tmp_path / "empty" / "config.json").write_text(json.dumps({"preset": "CLIP_L_TEXT"}))
    with pytest.raises(FileNotFoundError):
        CT.ClipTextTower.from_pretrained(str(tmp_path / "empty"), device="cpu")


def test_presets():
    l, h, x = CT.CLIP_L_TEXT, CT.VIT_H_14_TEXT, T5.T5_XXL
    assert (l.vocab, l.context, l.width, l.layers, l.heads, l.mlp_width, l.embed_dim, l.act) == (49408, 77, 768, 12, 12, 3072, 768, "quick_gelu")
    assert (h.vocab, h.context, h.width, h.layers, h.heads, h.mlp_width, h.embed_dim, h.act) == (49408, 77, 1024, 24, 16, 4096, 1024, "gelu")
    assert (x.vocab, x.d_model, x.layers, x.heads, x.d_kv, x.d_ff, x.num_buckets, x.max_distance, x.eps) == (32128, 4096, 24, 64, 64, 10240, 32, 128, 1e-6)
    assert l.head_dim == h.head_dim == 64 and x.inner == 4096 and l.eos_token_id == 2
    for c in (l, h, x):
        c.check()
    with pytest.raises(ValueError):
        CT.ClipTextConfig(width=768, heads=10).check()
    with pytest.raises(ValueError):
        T5.T5EncoderConfig(d_model=8192).check()


# ------------------------------------------------------------------------------------------------------------- host logic
stub_tokenizer = T.stub_tokenizer


class _StubClip:
    def __init__(self, width=768):
        self.config, self.device, self.width, self.calls = CT.ClipTextConfig(), torch.device("cpu"), width, []

    def pooled_output(self, ids):
        self.calls.append(tuple(ids.shape))
        return (ids.sum(-1, keepdim=True) % 251).to(torch.bfloat16).expand(-1, self.width).contiguous()

    def encode_text(self, ids, normalize=True):
        self.calls.append(tuple(ids.shape))
        return torch.stack([ids.sum(-1) % 251, (ids != 0).sum(-1)], -1).float()


class _StubT5:
    def __init__(self, d_model=4096):
        self.device, self.d_model, self.calls = torch.device("cpu"), d_model, []

    def encode(self, ids):
        self.calls.append(tuple(ids.shape))
        return (ids % 128).to(torch.bfloat16)[..., None].expand(-1, -1, self.d_model).contiguous()


def test_flux_prompt_encoder_and_cache_script(tmp_path):
    """Stub towers and stub tokenizers on the CPU: encode_prompt's three tensors, then the cache the script's writer leaves is
    read back by LatentDataset + latent_collate_function as [B, 512, 4096] / [B, 768] / [B, 3], the captions in file order; two
    ranks' strided shares give the same files as one process."""
    from mixgrpo_amd import preprocess_flux_embedding as PF
    from mixgrpo_amd.latent_flux_rl_datasets import LatentDataset, latent_collate_function
    from mixgrpo_amd.text_encoders import FluxPromptEncoder
    clip, t5 = _StubClip(), _StubT5()
    enc = FluxPromptEncoder(clip, t5, stub_tokenizer(77), stub_tokenizer(512))
    e, p, ti = enc.encode_prompt(["a cat", "a much longer prompt about a dog"])
    assert e.shape == (2, 512, 4096) and e.dtype == torch.bfloat16 and p.shape == (2, 768) and p.dtype == torch.bfloat16
    assert ti.shape == (512, 3) and not ti.any()
    assert clip.calls == [(2, 77)] and t5.calls == [(2, 512)]
    assert enc.encode_prompt("one string")[0].shape == (1, 512, 4096)
    # the prompt file formats
    prompts = ["a cat", "two dogs, running", "a \"quoted\" bird", "the fourth", "and a fifth"]
    (tmp_path / "p.txt").write_text("\n".join(prompts[:2]) + "\n\n" + "\n".join(prompts[2:]) + "\n")
    (tmp_path / "s.json").write_text(json.dumps(prompts))
    (tmp_path / "o.json").write_text(json.dumps([{"caption": p, "extra": 1} for p in prompts]))
    for name in ("p.txt", "s.json", "o.json"):
        assert PF.read_prompts(str(tmp_path / name)) == prompts
    (tmp_path / "bad.json").write_text(json.dumps([{"text": "no caption"}]))
    with pytest.raises(ValueError, match="caption"):
        PF.read_prompts(str(tmp_path / "bad.json"))
    # one process, batches of 2
    one = tmp_path / "one"
    path = PF.write_cache(enc, prompts, str(one), batch_size=2)
    entries = json.load(open(path))
    assert [x["caption"] for x in entries] == prompts
    assert set(entries[3]) == {"prompt_embed_path", "pooled_prompt_embeds_path", "text_ids", "caption"}
    assert entries[3]["prompt_embed_path"] == entries[3]["pooled_prompt_embeds_path"] == entries[3]["text_ids"] == "3.pt"
    assert torch.load(str(one / "prompt_embed" / "3.pt"), weights_only=True).shape == (1, 512, 4096)       # as the reference saves
    assert torch.load(str(one / "pooled_prompt_embeds" / "3.pt"), weights_only=True).shape == (1, 768)
    ds = LatentDataset(path, 1, 0.0)
    assert len(ds) == 5
    batch = latent_collate_function([ds[i] for i in range(5)])
    assert batch[0].shape == (5, 512, 4096) and batch[1].shape == (5, 768) and batch[2].shape == (5, 3)
    assert list(batch[3]) == prompts
    want_e, want_p, _ = enc.encode_prompt(prompts)
    assert torch.equal(batch[0], want_e) and torch.equal(batch[1], want_p) and not batch[2].any()
    # two ranks: rank 1 first (it writes no prompt.json), then rank 0
    two = tmp_path / "two"
    waited = []
    PF.write_cache(enc, prompts, str(two), batch_size=1, rank=1, world_size=2, barrier=lambda: waited.append(1))
    assert not (two / "prompt.json").exists() and sorted(f.name for f in (two / "prompt_embed").iterdir()) == ["1.pt", "3.pt"]
    PF.write_cache(enc, prompts, str(two), batch_size=4, rank=0, world_size=2, barrier=lambda: waited.append(0))
    assert waited == [1, 0] and json.load(open(two / "prompt.json")) == entries
    for i in range(5):
        for sub in ("prompt_embed", "pooled_prompt_embeds", "text_ids"):
            assert torch.equal(torch.load(str(two / sub / f"{i}.pt"), weights_only=True), torch.load(str(one / sub / f"{i}.pt"), weights_only=True))
    args = PF.parse_args(["--model_path", "m", "--prompt_path", "p", "--output_dir", "o", "--train_batch_size", "4", "--model_type",
                          "mochi", "--dataloader_num_workers", "2", "--text_encoder_name", "x", "--cache_dir", "c", "--vae_debug"])
    assert (args.model_path, args.prompt_path, args.output_dir, args.train_batch_size) == ("m", "p", "o", 4)


def test_package_import_does_not_import_transformers():
    code = "import sys, mixgrpo_amd, mixgrpo_amd.text_encoders, mixgrpo_amd.rewards, mixgrpo_amd.clip_text, mixgrpo_amd.t5, " \
           "mixgrpo_amd.preprocess_flux_embedding; assert 'transformers' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_text_tower_features_memoise():
    tower = _StubClip()
    f = RW.TextTowerFeatures(tower, stub_tokenizer(77))
    a = f.lookup(["a cat", "a dog", "a cat"], "cpu")
    assert a.shape == (3, 2) and a.dtype == torch.float32 and torch.equal(a[0], a[2]) and not torch.equal(a[0], a[1])
    assert tower.calls == [(2, 77)]                                     # the two distinct prompts as one batch
    b = f.lookup(["a dog", "a cat"], "cpu")
    assert tower.calls == [(2, 77)] and torch.equal(b, a[[1, 0]])       # the second lookup does not call the tower
    c = f.lookup(["a fish", "a dog"], "cpu")
    assert tower.calls == [(2, 77), (1, 77)] and torch.equal(c[1], a[1])


def test_builtin_rewards_with_a_text_tower(tmp_path, monkeypatch):
    """`text_tower_dir` (+ optional `tokenizer_dir`) instead of `text_features`; entries with text_features behave as before; an
    entry with neither fails with the message it always had."""
    made = []

    class Vision:
        logit_scale = 4.6

        @classmethod
        def from_pretrained(cls, path, device="cuda"):
            made.append(("vision", path, device))
            return cls()

    class Text:
        config = CT.ClipTextConfig()

        @classmethod
        def from_pretrained(cls, path, device="cuda"):
            made.append(("text", path, device))
            return cls()
    monkeypatch.setattr(CV, "ClipVisionTower", Vision)
    monkeypatch.setattr(CT, "ClipTextTower", Text)
    tf = RW.build_text_feature_cache(["p"], lambda ps: torch.ones(len(ps), 4), str(tmp_path / "text.safetensors"))
    cfg = tmp_path / "rewards.json"
    cfg.write_text(json.dumps({"HPSClipRewardModel": {"tower_dir": "/t/clip", "text_tower_dir": "/t/clip", "device": "cpu"},
                               "PickScoreRewardModel": {"tower_dir": "/t/clip", "text_tower_dir": "/t/clip", "device": "cpu"},
                               "CLIPScoreRewardModel": {"tower_dir": "/t/clip", "text_features": tf, "device": "cpu"}}))
    monkeypatch.setenv(RW.CONFIG_ENV, str(cfg))
    models = RW.builtin_rewards(None)
    hps, pick, clip = (models[k] for k in RW.KINDS[:1] + RW.KINDS[2:] + RW.KINDS[1:2])
    assert made == [("vision", "/t/clip", "cpu"), ("text", "/t/clip", "cpu")]
    assert isinstance(hps.text_features, RW.TextTowerFeatures) and hps.text_features is pick.text_features
    assert hps.text_features.tokenizer == "/t/clip" and isinstance(hps.text_features.text_tower, Text)
    assert isinstance(clip.text_features, RW.TextFeatureCache) and hps.tower is clip.tower
    cfg.write_text(json.dumps({"HPSClipRewardModel": {"tower_dir": "/t/clip", "text_tower_dir": "/t/text", "tokenizer_dir": "/t/tok",
                                                      "device": "cpu"}}))
    assert RW.builtin_rewards(None)["HPSClipRewardModel"].text_features.tokenizer == "/t/tok"
    cfg.write_text(json.dumps({"HPSClipRewardModel": {"tower_dir": "/t/clip"}}))
    with pytest.raises(ValueError, match=r"HPSClipRewardModel lacks \['text_features'\]"):
        RW.builtin_rewards(None)
