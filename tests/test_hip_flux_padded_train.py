"""The padded TRAINING path of the FLUX MMDiT (ops.ATTN_PAD_KV / MGX_ATTN_PAD_KV=1): the training forward, its block recompute
and the backward of a sequence off 256 run at the next multiple of 256 with the padding masked in the attention forward
(mgx_attn_fwd_log2_kv) and backward (mgx_attn_bwd_kv) -- the same kernels on the same padded shape as the padded rollout.
(a) the parameter gradients against torch autograd of the CPU oracle (oracle/mmdit.py) on the UNPADDED problem, switch off and
on, at the bounds of tests/test_hip_mmdit.py::test_backward_vs_oracle_autograd; (b) BASELINE.json configs[0] as
tests/test_hip_config0.py runs it, at 240 x 240 (a 15 x 15 packed latent + 512 text tokens: S = 737 -> Sa = 768): the first
replay chunk's log-probs against the rollout's.  The calls replaced are the reference's rollout forward and
`loss.backward()` through diffusers' FluxTransformer2DModel (fastvideo/train_grpo_flux.py:341-624)."""
import math

import pytest
import torch

from oracle import mmdit as OM
from test_hip_mmdit import build_pair, make_inputs, rel_err, small_cfg

pytestmark = pytest.mark.gpu

B, HG, WG, L = 2, 15, 15, 256           # S = 256 + 225 = 481 -> Sa = 512
COS_MIN, WORST_MAX = 0.999, 4e-2        # test_backward_vs_oracle_autograd's own bounds; the off arm (unchanged code) meets them at
                                        # this shape -- measured: 1 - cos 1.77e-5, worst tensor 1.18e-2 (on: 1.79e-5, 1.25e-2)


@pytest.mark.parametrize("switch", [False, True], ids=["off", "on"])
def test_gradients_vs_oracle_autograd(switch, monkeypatch):
    """d(sum(out * R)) / d(params) through the HIP training forward + backward against torch autograd of the oracle."""
    from mixgrpo_amd import ops
    monkeypatch.setattr(ops, "ATTN_PAD_KV", switch)
    ocfg, P, m = build_pair(small_cfg(1, 1))
    x, ehs, pooled, ids, tids, t, gd = make_inputs(B, HG, WG, L, seed=3)
    N, S = HG * WG, L + HG * WG
    assert S == 481
    R = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(9))
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = OM.forward(Pg, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids)
    (ref * R).sum().backward()
    m.train()
    args = (x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())
    calls = m.padded_kv_train_calls
    out = m(*args)[0]
    assert out.requires_grad and out.shape == (B, N, 64)
    (out.float() * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    g = m.store.g32
    assert m.flat_param.grad is g
    if switch:
        assert m.last_train_route == "padded_kv" and m.padded_kv_train_calls == calls + 1, "the padded training route was not taken"
        assert all(w.kv_len is None for w in m._work.values())
        tr = m._work[(L, 512 - L)].train
        for name in ("dQ", "dK", "dV"):       # of the last block walked: the padding tokens' rows are exactly zero
            assert bool((getattr(tr, name)[:B, :, S:].view(torch.int16) & 0x7FFF == 0).all()), name
            assert bool(getattr(tr, name)[:B, :, :S].float().abs().sum() > 0)
    else:
        assert m.last_train_route == "plain" and m.padded_kv_train_calls == calls
    dots = nh = no = 0.0
    worst = []
    mine = {}
    for k in P:
        gh = m.store.view(g, k).float().cpu()
        go = Pg[k].grad
        mine[k] = gh.clone()
        dots += (gh * go).sum().item()
        nh += gh.pow(2).sum().item()
        no += go.pow(2).sum().item()
        worst.append((((gh - go).norm() / (go.norm() + 1e-9)).item(), k))
    worst.sort(reverse=True)
    cos = dots / math.sqrt(nh * no)
    print(f"\nswitch {'on' if switch else 'off'}: cosine {cos:.6f} (1 - cos {1 - cos:.3e}), worst tensors {worst[:3]}")
    if switch:                                # recorded, not asserted: the padded route against the plain one, same weights
        monkeypatch.setattr(ops, "ATTN_PAD_KV", False)
        m0 = build_pair(small_cfg(1, 1))[2]
        m0.train()
        (m0(*args)[0].float() * R.cuda()).sum().backward()
        assert m0.last_train_route == "plain"
        off = {k: m0.store.view(m0.store.g32, k).float().cpu() for k in P}
        monkeypatch.setattr(ops, "ATTN_PAD_KV", True)
        rels = sorted(((rel_err(mine[k], off[k]), k) for k in P), reverse=True)
        a, b = (torch.cat([g_[k].flatten() for k in P]).double() for g_ in (mine, off))
        print(f"on versus off: worst per-tensor rel L2 {rels[0][0]:.3e} ({rels[0][1]}), cosine {torch.dot(a, b) / (a.norm() * b.norm()):.7f}")
    assert cos > COS_MIN, (cos, worst[:5])
    assert worst[0][0] < WORST_MAX, worst[:8]
    # a second forward + backward accumulates (gradient accumulation over replayed steps)
    out = m(*args)[0]
    (out.float() * R.cuda()).sum().backward()
    k0 = "transformer_blocks.0.ff.net.2.weight"
    assert rel_err(m.store.view(g, k0), 2 * Pg[k0].grad) < WORST_MAX
    if switch:
        assert m.padded_kv_train_calls == calls + 2 and all(w.kv_len is None for w in m._work.values())


@pytest.mark.parametrize("stream_k", [False, True])
def test_rollout_and_replay_run_the_same_kernels(stream_k, monkeypatch):
    """tests/test_hip_config0.py's configuration at 240 x 240 with the switch on: rollout and training route are both padded,
    and the first replay chunk -- the rollout policy itself -- gives the rollout's log-probs: bit for bit with every GEMM tile
    computed whole (the same kernels on the same padded shape, each output row the same K-loop whatever M is, the fused
    projections bit-identical to the two-pass forms), within the project's 2e-5 with the stream-K tail."""
    from mixgrpo_amd import ops
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.grpo_states import GRPOTrainingStates
    from mixgrpo_amd.optim import ConstantWithWarmup, FusedAdamW
    monkeypatch.setattr(ops, "GEMM_STREAM_K", stream_k)
    monkeypatch.setattr(ops, "ATTN_PAD_KV", True)
    dev = torch.device("cuda", 0)
    m = FluxTransformer2DModel(FluxConfig(num_layers=1, num_single_layers=1), device=dev).init_synthetic(seed=0, std=0.02)
    opt = FusedAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    args = TG.default_args(h=240, w=240, sampling_steps=8, num_generations=4, gradient_accumulation_steps=2)
    states = GRPOTrainingStates(iters_per_group=25, group_size=2, max_timesteps=8 - 2, prog_overlap=True,
                                prog_overlap_step=1, roll_back=True)
    window = states.get_current_timesteps()
    g = torch.Generator().manual_seed(714)
    batch = ((0.1 * torch.randn(1, 512, 4096, generator=g)).bfloat16().to(dev), torch.randn(1, 768, generator=g).bfloat16().to(dev),
             torch.zeros(1, 3, device=dev), ["a prompt"])
    torch.manual_seed(714)

    def const_reward(latents, captions):
        assert latents.shape == (4, 225, 64)                                  # G samples of a 30 x 30 latent, packed 15 x 15
        return [0.5] * 4, {"Const": [0.5] * 4}

    trace = {}
    TG.train_one_step(args, dev, m, None, const_reward, opt, ConstantWithWarmup(opt, 0), iter([batch]), None, 1.0,
                      window, 0, {"Const": 1.0}, trace=trace)
    torch.cuda.synchronize()
    assert m.last_route == "padded_kv" and m.padded_kv_calls > 0, "the rollout did not take the padded route"
    assert m.last_train_route == "padded_kv" and m.padded_kv_train_calls > 0, "the replay did not take the padded route"
    assert all(w.kv_len is None for w in m._work.values())
    assert torch.isfinite(trace["log_probs"][:, [0, 1]]).all()
    pairs, new_lp = trace["new_log_probs"][0]
    old = torch.stack([trace["log_probs"][i, t] for i, t in pairs])
    diff = (new_lp - old).abs().max().item()
    print(f"\nstream-K {stream_k}: first replay chunk vs rollout log-probs, max |diff| = {diff:.3e}")
    if not stream_k:
        assert torch.equal(new_lp, old)
    else:
        assert diff < 2e-5
