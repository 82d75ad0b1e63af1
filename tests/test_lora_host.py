"""Host side of LoRA fine-tuning (no GPU): target-name resolution against the parameter layout, refusal of unsupported names,
adapter state-dict keys and shapes, the `lora_config.json` round trip, the trainer's flags and the workspace size of
`mgx_lora_wgrad` (host code of the C ABI)."""
import json

import pytest

from mixgrpo_amd import lora as LR
from mixgrpo_amd.flux import FluxConfig, param_layout

CFG = FluxConfig(num_layers=2, num_single_layers=3, attention_head_dim=128, num_attention_heads=4, joint_attention_dim=64,
                 pooled_projection_dim=32)
D = CFG.dim


def test_default_targets_are_the_eight_attention_projections():
    assert LR.parse_target_modules(None) == LR.DEFAULT_TARGETS == LR.parse_target_modules("")
    assert len(LR.DEFAULT_TARGETS) == 8 and set(LR.DEFAULT_TARGETS) <= set(LR.SUPPORTED_TARGETS)
    got = LR.resolve_targets(param_layout(CFG), None)
    names = [m for m, _, _ in got]
    # 8 per double block; the single blocks' to_q / to_k / to_v match the same suffixes (peft's rule)
    assert len(names) == 2 * 8 + 3 * 3
    assert "transformer_blocks.1.attn.to_add_out" in names and "single_transformer_blocks.2.attn.to_v" in names
    assert all((N, K) == (D, D) for _, N, K in got)
    # layout order, which is the order of the adapters in the flat store
    order = [n[:-len(".weight")] for n, _ in param_layout(CFG)]
    assert names == [n for n in order if n in set(names)]


def test_every_supported_name_resolves_to_its_linears():
    layout = param_layout(CFG)
    for t, count, shape in (("to_out.0", 2, (D, D)), ("ff.net.0.proj", 2, (4 * D, D)), ("ff_context.net.0.proj", 2, (4 * D, D)),
                            ("proj_mlp", 3, (4 * D, D)), ("add_k_proj", 2, (D, D)), ("to_k", 5, (D, D))):
        got = LR.resolve_targets(layout, t)
        assert len(got) == count and all((N, K) == shape for _, N, K in got), (t, got)
    assert all(".ff_context." not in m for m, _, _ in LR.resolve_targets(layout, "ff.net.0.proj"))
    assert LR.parse_target_modules(" to_q, to_v ,to_q") == ("to_q", "to_v")


@pytest.mark.parametrize("name", ["ff.net.2", "ff_context.net.2", "proj_out", "norm1.linear", "x_embedder", "linear_1", "qkv"])
def test_unsupported_names_are_refused_by_name(name):
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        LR.parse_target_modules(f"to_q,{name}")
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        LR.resolve_targets(param_layout(CFG), [name])


def test_unsupported_rank_is_refused():
    with pytest.raises(ValueError, match="24"):
        LR.LoraStore(CFG, "cpu", 24, 24, allocate=False)


def test_store_layout_keys_and_shapes():
    lo = LR.LoraStore(CFG, "cpu", 32, 64, "to_q,proj_mlp,to_add_out", allocate=False)
    assert lo.scale == 2.0 and lo.rank == 32
    ks = lo.key_shapes()
    assert ks["transformer.transformer_blocks.0.attn.to_q.lora_A.weight"] == (32, D)
    assert ks["transformer.transformer_blocks.0.attn.to_q.lora_B.weight"] == (D, 32)
    assert ks["transformer.single_transformer_blocks.2.proj_mlp.lora_A.weight"] == (32, D)
    assert ks["transformer.single_transformer_blocks.2.proj_mlp.lora_B.weight"] == (4 * D, 32)
    assert len(ks) == 2 * (2 + 3 + 3 + 2)
    assert all(k.startswith("transformer.") and k.endswith((".lora_A.weight", ".lora_B.weight")) for k in ks)
    # flat layout: 64-aligned, disjoint, A and Bt adjacent, numel covers everything
    end = 0
    for key, (off, shape) in lo.index.items():
        assert off % 64 == 0 and off >= end and shape[0] == 32
        end = off + shape[0] * shape[1]
    assert lo.numel == end
    # one contiguous range per block, covering the store in order (the buckets of the DP reduction)
    rg = lo.block_ranges()
    assert rg["head"] == (0, 0) and rg["tail"] == (lo.numel, lo.numel)
    pos = 0
    for p in [f"transformer_blocks.{i}" for i in range(2)] + [f"single_transformer_blocks.{i}" for i in range(3)]:
        assert rg[p][0] == pos and rg[p][1] > pos
        pos = rg[p][1]
    assert pos == lo.numel
    only_out = LR.LoraStore(CFG, "cpu", 16, 16, "to_out.0", allocate=False).block_ranges()
    assert only_out["single_transformer_blocks.0"][0] == only_out["single_transformer_blocks.0"][1]


def test_members_of_fused_projections():
    from mixgrpo_amd.arch import describe
    arch = describe(CFG)
    lo = LR.LoraStore(CFG, "cpu", 16, 16, "to_q,to_v,proj_mlp,add_k_proj", allocate=False)
    p, s = "transformer_blocks.0.attn", "single_transformer_blocks.1"
    txt, img = arch.double[0].streams
    assert lo.members(img.qkv) == [(f"{p}.to_q", 0, D), (f"{p}.to_v", 2 * D, D)]
    assert lo.members(txt.qkv) == [(f"{p}.add_k_proj", D, D)]
    assert lo.members(arch.single[1].qkv_mlp) == [(f"{s}.attn.to_q", 0, D), (f"{s}.attn.to_v", 2 * D, D),
                                                  (f"{s}.proj_mlp", 3 * D, 4 * D)]
    assert lo.members(img.out) == [] and lo.members(arch.proj_out) == []


def test_lora_config_round_trip(tmp_path):
    cfg = LR.lora_config(64, 128, "to_q,to_out.0", step=30)
    assert cfg == {"step": 30, "lora_params": {"lora_rank": 64, "lora_alpha": 128.0, "target_modules": ["to_q", "to_out.0"]}}
    LR.write_lora_config(str(tmp_path), cfg)
    with open(tmp_path / "lora_config.json") as f:
        assert json.load(f) == cfg
    assert LR.read_lora_config(str(tmp_path)) == (64, 128.0, ("to_q", "to_out.0"), 30)
    assert not LR.is_lora_dir(str(tmp_path))          # no weights file yet
    (tmp_path / "pytorch_lora_weights.safetensors").write_bytes(b"")
    assert LR.is_lora_dir(str(tmp_path)) and not LR.is_lora_dir(None)


def test_trainer_flags():
    from mixgrpo_amd import train_grpo_flux as TG
    p = TG.build_parser()
    a = p.parse_args(["--data_json_path", "x"])
    assert a.use_lora is False and a.lora_rank == 16 and a.lora_alpha is None and a.lora_target_modules is None
    a = p.parse_args(["--data_json_path", "x", "--use_lora", "--lora_rank", "64", "--lora_alpha", "128",
                      "--lora_target_modules", "to_q,to_k,proj_mlp"])
    assert a.use_lora and a.lora_rank == 64 and a.lora_alpha == 128.0
    assert LR.parse_target_modules(a.lora_target_modules) == ("to_q", "to_k", "proj_mlp")
    assert {"lora_rank", "lora_alpha", "lora_target_modules"} <= {f[0] for f in TG._ENGINE_FLAGS}


def test_wgrad_workspace_is_host_code():
    from mixgrpo_amd import ops
    for r in (16, 32, 64, 128):
        assert ops.lora_wgrad_workspace(1, 64, r) == r * 64                       # one chunk
    n = ops.lora_wgrad_workspace(1100, 512, 64)
    assert n % (64 * 512) == 0 and 1 < n // (64 * 512) <= (1100 + 63) // 64       # several chunks, never more than 64-row tiles
    big = ops.lora_wgrad_workspace(4 * 4608, 3072, 64)
    assert big % (64 * 3072) == 0 and big * 4 < 64 << 20                           # the headline shape stays under 64 MiB
    for bad in ((0, 512, 16), (64, 96, 16), (64, 0, 16), (64, 512, 8), (64, 512, 48), (1 << 31, 512, 16)):
        with pytest.raises(ValueError):
            ops.lora_wgrad_workspace(*bad)
