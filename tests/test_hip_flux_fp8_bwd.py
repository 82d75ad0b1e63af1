"""The FLUX MMDiT with attention_dtype="fp8" trained through the e4m3 attention backward (ops.ATTN_FP8_BWD /
MGX_ATTN_FP8_BWD=1, csrc/attention_fp8_bwd.hip), on the tiny 1 + 1-block model of tests/test_hip_attention_fp8.py.
  * switch on: every parameter gradient against the switch-off run (the bf16 backward on the bf16 operands) by cosine.  The two
    are different gradients by design (the e4m3 one differentiates the quantised function the forward ran), so the bound is the
    measured minimum minus a quarter of its 1 - cos.  Measured on an MI355X: MEASURED_COS_MIN below;
  * an lr = 0 train step still replays the rollout's log-probs bit for bit (the forward is untouched) with a positive gradient norm;
  * switch off: the gradients are bit-identical before and after the model has run the new path."""
import pytest
import torch

from test_hip_attention_fp8 import CFG

pytestmark = pytest.mark.gpu

MEASURED_COS_MIN = 0.994293   # smallest per-parameter cosine, on versus off (single_transformer_blocks.0.attn.to_k.bias; the whole
                              # gradient: 0.999923; 58 of the 66 tensors differ)
COS_BOUND = MEASURED_COS_MIN - 0.25 * (1.0 - MEASURED_COS_MIN)


def _model_and_inputs():
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    m8 = FluxTransformer2DModel(FluxConfig(**CFG), device=dev, attention_dtype="fp8").init_synthetic(seed=5, std=0.05, bias_std=0.02)
    B, N, L = 2, 48 * 4, 16
    xs = torch.randn(B, N, 64, generator=g).to(dev)
    ehs = torch.randn(B, L, 64, generator=g).bfloat16().to(dev)
    pooled = torch.randn(B, 32, generator=g).bfloat16().to(dev)
    ids = torch.zeros(12, 16, 3)
    ids[..., 1] += torch.arange(12)[:, None]
    ids[..., 2] += torch.arange(16)[None]
    ids = ids.reshape(N, 3).to(dev)
    t = torch.tensor([0.954, 0.5]).to(dev)
    gd = torch.tensor([3.5]).bfloat16().to(dev)
    txt = torch.zeros(L, 3, device=dev)
    Rw = torch.randn(B, N, 64, generator=g).to(dev)
    return m8, (xs, ehs, t, gd, txt, pooled, ids), Rw, ehs, pooled


def _grads(m, args, Rw):
    """Parameter gradients of sum(out * Rw) through the training forward + backward, per name, on the CPU."""
    if m.store.g32 is not None:
        m.store.g32.zero_()
    m.train()
    (m(*args)[0].float() * Rw).sum().backward()
    torch.cuda.synchronize()
    return {k: m.store.view(m.store.g32, k).float().cpu().clone() for k in m.store.index}


def _used_fp8_backward(m):
    return any(w._f8_bwd is not None for w in m._work.values())


def test_gradients_on_versus_off_and_off_is_untouched(monkeypatch):
    from mixgrpo_amd import ops
    m, args, Rw, _, _ = _model_and_inputs()
    monkeypatch.setattr(ops, "ATTN_FP8_BWD", False)
    off = _grads(m, args, Rw)
    assert not _used_fp8_backward(m)
    monkeypatch.setattr(ops, "ATTN_FP8_BWD", True)
    on = _grads(m, args, Rw)
    assert _used_fp8_backward(m), "the e4m3 backward was not taken"
    monkeypatch.setattr(ops, "ATTN_FP8_BWD", False)
    off2 = _grads(m, args, Rw)
    for k in off:                                                             # switch off: the instructions it ran before
        assert torch.equal(off[k], off2[k]), k
    coss, differ = [], 0
    for k in off:
        assert torch.isfinite(on[k]).all(), k
        no, nn = off[k].double().norm().item(), on[k].double().norm().item()
        if no == 0.0:
            assert nn == 0.0, k
            continue
        coss.append(((off[k].double() * on[k].double()).sum().item() / (no * nn), k))
        differ += int(not torch.equal(off[k], on[k]))
    coss.sort()
    a, b = (torch.cat([g[k].flatten() for k in off]).double() for g in (on, off))
    print(f"\non versus off: smallest per-parameter cosines {coss[:4]}, whole gradient {(a @ b / (a.norm() * b.norm())).item():.6f}, "
          f"{differ} of {len(coss)} tensors differ")
    assert differ > 0, "the switch changed nothing"
    assert coss[0][0] >= COS_BOUND, coss[:6]


def test_lr0_step_replays_the_rollout_bit_for_bit(monkeypatch):
    from mixgrpo_amd import ops
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd.optim import ConstantWithWarmup, FusedAdamW
    monkeypatch.setattr(ops, "ATTN_FP8_BWD", True)
    dev = torch.device("cuda", 0)
    m8, _, _, ehs, pooled = _model_and_inputs()
    opt = FusedAdamW(m8, lr=0.0)                                              # weights unchanged -> ratio must be exactly 1
    args = TG.default_args(h=48, w=64, sampling_steps=6, num_generations=4, gradient_accumulation_steps=2)
    loader = iter([(ehs[:1], pooled[:1], torch.zeros(1, 3, device=dev), ["p"])])

    def reward(lat, cap):
        r = torch.tensor([0.1, 0.4, 0.2, 0.9])
        return r, {"Synthetic": r}

    trace = {}
    res = TG.train_one_step(args, dev, m8, None, reward, opt, ConstantWithWarmup(opt, 0), loader, None, 1.0, [1, 2], 0,
                            {"Synthetic": 1.0}, trace=trace)
    lp = trace["log_probs"]
    for pairs, new in trace["new_log_probs"]:
        old = torch.stack([lp[i, tt] for i, tt in pairs])
        assert torch.equal(new, old)
    assert _used_fp8_backward(m8), "the e4m3 backward was not taken"
    gn = trace["grad_norms"][0].item()
    assert res[4] == 0.0 and gn > 0 and gn == gn                              # nothing clipped, finite gradients flow
