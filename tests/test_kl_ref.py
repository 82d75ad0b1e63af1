"""`--kl_ref_coeff` without a GPU: the restatement of the KL term (tests/kl_ref.py) against torch.distributions, the flag and
the argument check."""
from argparse import Namespace

import pytest
import torch

import kl_ref as KR
from oracle import solver as O


def _step_inputs(seed, shape=(3, 64, 64), T=8, index=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    v = torch.randn(*shape, generator=g).bfloat16()
    v_ref = (v.float() + 0.3 * torch.randn(*shape, generator=g)).bfloat16()
    sig = O.sd3_time_shift(3.0, torch.linspace(1, 0, T + 1))
    prev = O.flow_grpo_step(v, x, 0.7, sig, index, None, noise=torch.randn(*shape, generator=g).bfloat16())[0]
    return x, v, v_ref, sig, index, prev


def test_restatement_is_the_kl_of_the_two_gaussians():
    x, v, v_ref, sig, index, prev = _step_inputs(1)
    _, _, _, mean, sd = O.flow_grpo_step(v, x, 0.7, sig, index, prev)
    mean_ref = O.flow_grpo_step(v_ref, x, 0.7, sig, index, prev)[3]
    mean, mean_ref, sd = mean.double(), mean_ref.double(), sd.double()
    N = torch.distributions.Normal
    want = torch.distributions.kl_divergence(N(mean, sd), N(mean_ref, sd)).mean(dim=(1, 2))
    got = KR.kl_to_reference(mean, mean_ref, sd)
    assert got.dtype == torch.float64 and (got > 0).all()
    assert ((got - want).abs() <= 1e-12 * want.abs()).all(), (got, want)


def test_restatement_is_zero_when_the_policy_is_the_reference_and_has_the_expected_gradient():
    x, v, v_ref, sig, index, prev = _step_inputs(2)
    lp, kl = KR.flow_grpo_step_kl(v, v.clone(), x, 0.7, sig, index, prev)
    assert torch.equal(kl, torch.zeros(3))
    assert torch.equal(lp, O.flow_grpo_step(v, x, 0.7, sig, index, prev)[2])
    # the reference output takes no gradient, and the term's gradient vanishes at the reference
    v_g, r_g = v.clone().requires_grad_(True), v.clone().requires_grad_(True)
    KR.flow_grpo_step_kl(v_g, r_g, x, 0.7, sig, index, prev)[1].sum().backward()
    assert r_g.grad is None and torch.equal(v_g.grad, torch.zeros_like(v))
    v_g = v.clone().requires_grad_(True)
    KR.flow_grpo_step_kl(v_g, v_ref, x, 0.7, sig, index, prev)[1].sum().backward()
    assert v_g.grad.abs().max() > 0


def test_parser_has_the_flag_with_default_zero():
    from mixgrpo_amd import train_grpo_flux as TG
    p = TG.build_parser()
    a = p.parse_args(["--data_json_path", "x"])
    assert a.kl_ref_coeff == 0.0 and isinstance(a.kl_ref_coeff, float)
    assert p.parse_args(["--data_json_path", "x", "--kl_ref_coeff", "0.25"]).kl_ref_coeff == 0.25
    assert "kl_ref_coeff" in {f[0] for f in TG._ENGINE_FLAGS}
    assert TG.default_args().kl_ref_coeff == 0.0


def _args(**kw):
    a = dict(kl_ref_coeff=0.1, flow_grpo_sampling=True, dpm_algorithm_type="null", dpm_apply_strategy="post")
    a.update(kw)
    return Namespace(**a)


def test_check_ref_kl_args():
    from mixgrpo_amd.train_grpo_flux import check_ref_kl_args
    # the good ones: adapters and the Flow-GRPO step (plain, or behind a DPM rollout compressed "post")
    check_ref_kl_args(_args(), True)
    check_ref_kl_args(_args(dpm_algorithm_type="dpmsolver++", dpm_apply_strategy="post"), True)
    # off: nothing is asked of the other flags
    for lora in (False, True):
        check_ref_kl_args(_args(kl_ref_coeff=0.0, flow_grpo_sampling=False, dpm_algorithm_type="dpmsolver", dpm_apply_strategy="all"),
                          lora)
    bad = ((_args(), False),                                                                    # no adapters
           (_args(flow_grpo_sampling=False), True),                                             # the dance replay
           (_args(dpm_algorithm_type="dpmsolver++", dpm_apply_strategy="all"), True))           # the DPM replay
    for a, lora in bad:
        with pytest.raises(ValueError, match="kl_ref_coeff"):
            check_ref_kl_args(a, lora)
    with pytest.raises(ValueError, match="kl_ref_coeff"):
        check_ref_kl_args(_args(kl_ref_coeff=-1.0), True)
