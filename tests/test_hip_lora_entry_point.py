"""`python -m mixgrpo_amd.train_grpo_flux --use_lora ...` end to end on the GPU: three adapter train steps with an adapter
checkpoint (`lora-checkpoint-3-0`: adapter weights, `lora_config.json`, the adapters' AdamW moments and the resume state, no
base weights), then a second launch that resumes from that directory and reproduces the uninterrupted third step."""
import json
import os

import pytest

from test_hip_entry_point import _flags, _run, _setup

pytestmark = pytest.mark.gpu


def test_main_with_use_lora_checkpoints_adapters_and_resumes(tmp_path):
    from safetensors.torch import load_file
    tmp = str(tmp_path)
    _setup(tmp)
    lora = ["--use_lora", "--lora_rank", "16", "--lora_alpha", "32", "--lora_target_modules", "to_q,to_v,to_out.0,proj_mlp"]
    logs = _run(_flags(tmp, ["--max_train_steps", "3", "--checkpointing_steps", "3"] + lora), tmp)
    assert [l["step"] for l in logs] == [1, 2, 3]
    assert all(l["grad_norm"] == l["grad_norm"] and l["grad_norm"] > 0 for l in logs)
    run_dir = os.path.join(tmp, "outputs", "part_cli")
    ck = os.path.join(run_dir, "lora-checkpoint-3-0")
    assert sorted(os.listdir(ck)) == ["lora_config.json", "optimizer.safetensors", "pytorch_lora_weights.safetensors",
                                      "rng_state_rank0.json", "rng_state_rank0.safetensors", "trainer_state.json"]
    assert not os.path.exists(os.path.join(run_dir, "checkpoint-3-0"))
    cfg = json.load(open(os.path.join(ck, "lora_config.json")))
    assert cfg == {"step": 3, "lora_params": {"lora_rank": 16, "lora_alpha": 32.0,
                                              "target_modules": ["to_q", "to_v", "to_out.0", "proj_mlp"]}}
    sd = load_file(os.path.join(ck, "pytorch_lora_weights.safetensors"))
    assert tuple(sd["transformer.transformer_blocks.0.attn.to_q.lora_A.weight"].shape) == (16, 512)
    assert tuple(sd["transformer.single_transformer_blocks.0.proj_mlp.lora_B.weight"].shape) == (2048, 16)
    assert len(sd) == 2 * (3 + 3)                                  # double: to_q, to_v, to_out.0; single: to_q, to_v, proj_mlp
    assert sd["transformer.transformer_blocks.0.attn.to_q.lora_B.weight"].abs().max() > 0     # B has left zero after two steps
    n_adapter = sum(v.numel() for v in sd.values())
    assert load_file(os.path.join(ck, "optimizer.safetensors"))["m"].numel() == n_adapter      # moments of the adapters only

    again = _run(_flags(tmp, ["--max_train_steps", "3", "--checkpointing_steps", "3", "--resume_from_checkpoint", ck,
                              "--experiment_name", "cli_resumed"]), tmp)
    assert [l["step"] for l in again] == [3] and again[0]["global_step"] == 2
    assert again[0]["timesteps_train"] == logs[2]["timesteps_train"]
    for k in ("train_loss", "grad_norm", "clip_frac", "reward_SyntheticReward"):
        assert again[0][k] == pytest.approx(logs[2][k], rel=1e-6, abs=1e-9), k

    # an unsupported target name fails before any weight is read, naming it
    import subprocess
    import sys
    from test_hip_entry_point import ROOT
    bad = subprocess.run([sys.executable, "-m", "mixgrpo_amd.train_grpo_flux"] +
                         _flags(tmp, ["--max_train_steps", "1", "--use_lora", "--lora_target_modules", "to_q,ff.net.2"]),
                         cwd=tmp, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "ff.net.2" in bad.stderr
