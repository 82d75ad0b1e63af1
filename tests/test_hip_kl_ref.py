"""`--kl_ref_coeff` on the GPU: the KL penalty of a replayed Flow-GRPO step to the frozen base policy under the adapters.

Kernels (`mgx_flow_kl_fwd`, `mgx_flow_step_kl_bwd`) against the CPU restatement tests/kl_ref.py at the standard of
tests/test_hip_solver.py -- kl at the log-prob tolerance, dv bit for bit against the oracle's autograd --, the model's
`reference_policy()`, the term inside `train_one_step`, the entry point, and one recorded (not asserted) cost measurement."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import kl_ref as KR
from oracle import solver as O
from test_hip_entry_point import ROOT, _flags, _run, _setup
from test_hip_lora import TARGETS, _cuda, _randomise
from test_hip_mmdit import build_pair, make_inputs, small_cfg
from test_hip_solver import close_lp, dev, eq

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
RECORD_DIR = os.environ.get("MGX_RECORD_DIR")          # set: the measured figures also go to ref_kl.json in that directory


def _bits(a, b):
    """Same bits, signed zeros and NaN payloads included."""
    view = {BF16: torch.int16, F32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---------------------------------------------------------------------------------------------------- kernels
SHAPES = [(3, 64, 64), (3, 257, 8), (3, 1, 8)]        # n = 4096: two full blocks; 2056: the second nearly empty; 8: one vector
STEPS = [(8, 1), (8, 3), (25, 2), (25, 12)]           # (T, index) of test_hip_solver.py::test_flow_replay_backward_vs_oracle_autograd
W_LP, W_KL = torch.tensor([0.3, -1.7, 2.5]), torch.tensor([0.8, 0.05, 1.9])


def _case(shape, T, index):
    from mixgrpo_amd import sampling_utils as SU
    g = torch.Generator().manual_seed(5 + index + shape[1])
    x = torch.randn(*shape, generator=g)
    v = torch.randn(*shape, generator=g).bfloat16()
    v_ref = (v.float() + 0.5 * torch.randn(*shape, generator=g)).bfloat16()
    sig = SU.sd3_time_shift(3.0, torch.linspace(1, 0, T + 1))
    prev = O.flow_grpo_step(v, x, 0.7, sig, index, None, noise=torch.randn(*shape, generator=g).bfloat16())[0]
    return x, v, v_ref, sig, prev


def _hip(x, v, v_ref, sig, index, prev, w_lp, w_kl):
    """(log_prob, kl, dv) of `sampling_utils.flow_grpo_step_kl` under the loss (lp * w_lp + kl * w_kl).sum()."""
    from mixgrpo_amd import sampling_utils as SU
    v_h = dev(v).requires_grad_(True)
    lp, kl = SU.flow_grpo_step_kl(v_h, dev(v_ref), dev(x), 0.7, sig, index, dev(prev))
    (lp * dev(w_lp) + kl * dev(w_kl)).sum().backward()
    return lp.detach(), kl.detach(), v_h.grad


def _plain_dv(x, v, sig, index, prev, w_lp):
    """dv of `mgx_flow_step_bwd`, the kernel without the term."""
    from mixgrpo_amd import sampling_utils as SU
    v_h = dev(v).requires_grad_(True)
    lp = SU.flow_grpo_step(v_h, dev(x), 0.7, sig, index, dev(prev), want_x0=False, want_mean=False)[2]
    (lp * dev(w_lp)).sum().backward()
    return lp.detach(), v_h.grad


@pytest.mark.parametrize("T,index", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kl_and_fused_backward_vs_oracle_autograd(shape, T, index):
    x, v, v_ref, sig, prev = _case(shape, T, index)
    v_o = v.clone().requires_grad_(True)
    lp_o, kl_o = KR.flow_grpo_step_kl(v_o, v_ref, x, 0.7, sig, index, prev)
    (lp_o * W_LP + kl_o * W_KL).sum().backward()
    lp_h, kl_h, dv = _hip(x, v, v_ref, sig, index, prev, W_LP, W_KL)
    print(f"shape {shape} T {T} index {index}: kl {kl_h.tolist()} oracle {kl_o.tolist()}")
    assert (kl_o > 0).all()
    close_lp(kl_h, kl_o.detach())
    close_lp(lp_h, lp_o.detach())
    eq(dv, v_o.grad)
    # the same call again: the same bits (no atomics, a fixed-order reduction)
    lp2, kl2, dv2 = _hip(x, v, v_ref, sig, index, prev, W_LP, W_KL)
    assert _bits(kl_h, kl2) and _bits(lp_h, lp2) and _bits(dv, dv2)
    # without the term's gradient, or at the reference: mgx_flow_step_bwd's bits
    lp_p, dv_p = _plain_dv(x, v, sig, index, prev, W_LP)
    assert _bits(lp_h, lp_p) and not _bits(dv, dv_p)
    assert _bits(_hip(x, v, v_ref, sig, index, prev, W_LP, torch.zeros(3))[2], dv_p)
    lp_s, kl_s, dv_s = _hip(x, v, v.clone(), sig, index, prev, W_LP, W_KL)
    assert _bits(kl_s, torch.zeros(3, device="cuda")) and _bits(dv_s, dv_p) and _bits(lp_s, lp_p)


def test_kl_kernels_refuse_bad_arguments():
    import ctypes as C
    from mixgrpo_amd import sampling_utils as SU
    from mixgrpo_amd._lib import MgxError, check, lib, logp_workspace, ptr, stream
    sig = SU.sd3_time_shift(3.0, torch.linspace(1, 0, 9))
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="cuda")
    with pytest.raises(ValueError):                               # the replay form only
        SU.flow_grpo_step_kl(z(2, 16, dtype=BF16), z(2, 16, dtype=BF16), z(2, 16), 0.7, sig, 1, None)
    B, n = 2, 16
    k = SU.flow_coeffs(sig, 1, 0.7)
    x, prev, v, v_ref, dv = z(B, n), z(B, n), z(B, n, dtype=BF16), z(B, n, dtype=BF16), z(B, n, dtype=BF16)
    kl, g = z(B), z(B)
    ws = logp_workspace(B, n, x.device)
    fwd = [ptr(x), ptr(v), ptr(v_ref), ptr(kl), ptr(ws)]
    bwd = [ptr(x), ptr(v), ptr(v_ref), ptr(prev), ptr(g), ptr(g), ptr(dv)]
    check(lib().mgx_flow_kl_fwd(*fwd, B, n, C.byref(k), stream()))
    check(lib().mgx_flow_step_kl_bwd(*bwd, B, n, C.byref(k), stream()))
    for i in range(len(fwd)):
        with pytest.raises(MgxError, match="null"):
            check(lib().mgx_flow_kl_fwd(*(fwd[:i] + [None] + fwd[i + 1:]), B, n, C.byref(k), stream()))
    for i in range(len(bwd)):
        with pytest.raises(MgxError, match="null"):
            check(lib().mgx_flow_step_kl_bwd(*(bwd[:i] + [None] + bwd[i + 1:]), B, n, C.byref(k), stream()))
    with pytest.raises(MgxError, match="null"):
        check(lib().mgx_flow_kl_fwd(*fwd, B, n, None, stream()))
    with pytest.raises(MgxError, match="empty"):
        check(lib().mgx_flow_step_kl_bwd(*bwd, 0, n, C.byref(k), stream()))
    for call, ptrs in ((lib().mgx_flow_kl_fwd, fwd), (lib().mgx_flow_step_kl_bwd, bwd)):
        with pytest.raises(MgxError, match="multiple of 8"):        # n = 12 (refused before any launch)
            check(call(*ptrs, 1, 12, C.byref(k), stream()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def pair():
    ocfg, P, m = build_pair(small_cfg(2, 2))
    return m, _cuda(make_inputs(2, 8, 12, 40, seed=3))


def test_reference_policy_is_the_base_and_leaves_the_compute_copy_as_it_was(pair):
    from mixgrpo_amd._lib import MgxError
    m, args = pair
    m.unload_lora()
    m.add_lora(rank=16, alpha=32, target_modules=TARGETS)
    _randomise(m.lora, 1)
    m.merge_lora()
    w16 = m.store.w16.clone()
    m.train()
    policy = m(*args)[0].detach().clone()
    assert m.reference_policy_bytes == 0                                    # nothing is held before the first use
    with m.reference_policy():
        assert not torch.equal(m.store.w16, w16)
        out = m(*args)[0]                                                   # training mode, gradients on: the training route
        assert not out.requires_grad
        ref_tr = out.clone()
        with torch.no_grad():
            ref_ng = m(*args)[0].clone()                                    # the no-grad route
        with pytest.raises(MgxError, match="already"):
            with m.reference_policy():
                pass
    assert _bits(m.store.w16, w16)
    assert m.reference_policy_bytes == 2 * sum(N * K for _, N, K in m.lora.targets)
    assert not torch.equal(ref_tr, policy)
    out = m(*args)[0]                                                       # outside: the policy again, with its graph
    assert out.requires_grad and _bits(out.detach(), policy)
    m.unload_lora()
    assert m.reference_policy_bytes == 0
    base_tr = m(*args)[0].detach().clone()
    with torch.no_grad():
        base_ng = m(*args)[0].clone()
    assert _bits(ref_tr, base_tr) and _bits(ref_ng, base_ng)
    with pytest.raises(MgxError, match="no adapters"):
        with m.reference_policy():
            pass


def test_fresh_adapters_make_the_reference_pass_the_policys_bit_for_bit(pair):
    m, args = pair
    m.unload_lora()
    m.add_lora(rank=16, alpha=32, target_modules=TARGETS)                   # B = 0: the merged weights are the base's
    m.train()
    for grad in (True, False):                                              # the training route and the no-grad route
        with torch.set_grad_enabled(grad):
            with m.reference_policy():
                v_ref = m(*args)[0].clone()
            v = m(*args)[0].detach()
        assert _bits(v, v_ref), grad
    m.unload_lora()


def _train_step(kl_ref_coeff, randomise, accum=4, trace=None, G=4):
    """tests/test_hip_lora.py::_lora_train_step with the flag: one train step of a 1 + 1 block model with adapters, one group
    of G.  accum = G: a single chunk, every replay before the only optimizer step; accum > G: a leftover chunk, whose
    gradients stay in the buffer and are never applied."""
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.optim import ConstantWithWarmup, FusedAdamW
    dev_ = torch.device("cuda", 0)
    m = FluxTransformer2DModel(FluxConfig(**small_cfg(1, 1)), device=dev_).init_synthetic(seed=5, std=0.05, bias_std=0.02)
    m.add_lora(16, 32, "to_q,to_k,to_v,to_out.0,proj_mlp", seed=1)
    if randomise:
        _randomise(m.lora, 8, std=0.05)
        m.merge_lora()
    opt = FusedAdamW(m, lr=1e-3)
    args = TG.default_args(h=48, w=64, sampling_steps=8, num_generations=G, gradient_accumulation_steps=accum,
                           share_rollout_prefix=False, kl_ref_coeff=kl_ref_coeff)
    g = torch.Generator().manual_seed(1)
    batch = ((0.1 * torch.randn(1, 16, 64, generator=g)).bfloat16().to(dev_), torch.randn(1, 32, generator=g).bfloat16().to(dev_),
             torch.zeros(1, 3, device=dev_), ["p"])
    args.injected_noise = {"x_T": torch.randn(1, 16, 6, 8, generator=torch.Generator().manual_seed(77)).bfloat16(),
                           "steps": [torch.randn(G, 12, 64, generator=g).bfloat16() for _ in range(8)]}
    r = torch.tensor([0.1, 0.4, 0.2, 0.9][:G])
    res = TG.train_one_step(args, dev_, m, None, lambda lat, cap: (r, {"Synthetic": r}), opt, ConstantWithWarmup(opt, 0),
                            iter([batch]), None, 1.0, [1, 2], 0, {"Synthetic": 1.0}, trace=trace)
    torch.cuda.synchronize()
    return res, m, args


def test_train_step_with_fresh_adapters_is_the_step_without_the_term():
    res0, m0, _ = _train_step(0.0, randomise=False)
    res1, m1, _ = _train_step(0.5, randomise=False)
    print("off:", res0, "on:", res1, "ref_kl", m1.last_ref_kl)
    assert len(res1) == 6 and res1 == res0
    assert res0[1] > 0                                                       # the step did move the adapters
    assert _bits(m1.lora.w32, m0.lora.w32) and _bits(m1.store.w16, m0.store.w16)
    assert m1.last_ref_kl == 0.0 and m0.last_ref_kl is None


def test_loss_accounting_with_randomised_adapters():
    """One chunk (G = accum = 4): the policy loss, the kl_loss and the clip fraction do not see the flag; the total gains
    kl_ref_coeff * sum(kl) / denom, held to the fp32 rounding of the total (1e-6 relative); the logged mean is sum(kl) / pairs."""
    coeff = 0.5
    res0, m0, _ = _train_step(0.0, randomise=True)
    trace = {}
    res1, m1, args = _train_step(coeff, randomise=True, trace=trace)
    recs = trace["ref_kl_replays"]
    assert len(recs) == 1 and len(recs[0]["pairs"]) == 8                     # 4 samples x 2 window steps, one micro-batch
    kl = recs[0]["kl"].double().cpu()
    denom = 4 * 2
    term = coeff * kl.sum().item() / denom
    print(f"off {res0}\non  {res1}\nkl {kl.tolist()} term {term:.6e} total on - off {res1[0] - res0[0]:.6e}")
    assert (kl > 0).all() and m1.last_ref_kl > 0
    assert res1[2:5] == res0[2:5]                                            # policy loss, kl_loss, clip fraction: bit-identical
    assert res1[0] == pytest.approx(res0[0] + term, rel=1e-6)
    assert res1[0] != res0[0]
    assert m1.last_ref_kl == pytest.approx(kl.mean().item(), rel=1e-6) and trace["ref_kl"] == m1.last_ref_kl
    assert not torch.equal(m1.lora.w32, m0.lora.w32)                          # the term reached the adapters
    assert _bits(recs[0]["g_kl"], torch.full((8,), coeff / denom, device="cuda"))


def test_replay_gradients_are_the_fused_backward_through_the_model():
    """The plumbing, with no tolerance: a leftover chunk (accum 8 > G 4) leaves the replay's adapter gradients in the buffer.
    dv rebuilt from the captured operands by `flow_grpo_step_kl` alone, pushed through an identical second forward, gives the
    same gradients bit for bit.  (What ties adapter gradients for a given dv to the oracle: tests/test_hip_lora.py.)"""
    from mixgrpo_amd import sampling_utils as SU
    trace = {}
    res, m, args = _train_step(0.5, randomise=True, accum=8, trace=trace)
    assert res[1] is None                                                    # no optimizer step: the adapters are the replay's
    rec, = trace["ref_kl_replays"]
    g_replay = m.lora.g32.clone()
    assert g_replay.abs().max() > 0
    sig = SU.sd3_time_shift(args.shift, torch.linspace(1, 0, args.sampling_steps + 1))
    x, steps = rec["fwd_kw"]["hidden_states"], [p[1] for p in rec["pairs"]]
    assert steps == sorted(steps) and set(steps) == {1, 2}
    dv, kl = torch.empty_like(rec["v"]), torch.empty_like(rec["kl"])
    for t in (1, 2):
        rows = [i for i, s in enumerate(steps) if s == t]
        lo, hi = rows[0], rows[-1] + 1
        v = rec["v"][lo:hi].clone().requires_grad_(True)
        lp, kl_s = SU.flow_grpo_step_kl(v, rec["v_ref"][lo:hi], x[lo:hi], args.eta, sig, t, rec["prev"][lo:hi])
        (lp * rec["g_logp"][lo:hi] + kl_s * rec["g_kl"][lo:hi]).sum().backward()
        dv[lo:hi], kl[lo:hi] = v.grad, kl_s.detach()
    assert _bits(kl, rec["kl"]) and _bits(dv, rec["dv"])
    plain = torch.empty_like(dv)                                             # and the term is in it
    for t in (1, 2):
        rows = [i for i, s in enumerate(steps) if s == t]
        lo, hi = rows[0], rows[-1] + 1
        v = rec["v"][lo:hi].clone().requires_grad_(True)
        lp = SU.flow_grpo_step(v, x[lo:hi], args.eta, sig, t, rec["prev"][lo:hi], want_x0=False, want_mean=False)[2]
        (lp * rec["g_logp"][lo:hi]).sum().backward()
        plain[lo:hi] = v.grad
    assert not _bits(plain, dv)
    m.lora.g32.zero_()
    m.train()
    with torch.autocast("cuda", torch.bfloat16):
        pred = m(**rec["fwd_kw"])[0]
    assert _bits(pred.detach(), rec["v"])
    pred.backward(dv)
    assert _bits(m.lora.g32, g_replay)


# ---------------------------------------------------------------------------------------------------- entry point
def test_main_logs_ref_kl_and_refuses_the_flag_without_adapters(tmp_path):
    tmp = str(tmp_path)
    _setup(tmp)
    lora = ["--use_lora", "--lora_rank", "16", "--lora_alpha", "32", "--lora_target_modules", "to_q,to_v,to_out.0,proj_mlp"]
    logs = _run(_flags(tmp, ["--max_train_steps", "2", "--checkpointing_steps", "100", "--kl_ref_coeff", "0.1"] + lora), tmp)
    assert [l["step"] for l in logs] == [1, 2]
    assert all("ref_kl" in l and math.isfinite(l["ref_kl"]) and l["ref_kl"] >= 0 for l in logs), logs
    assert logs[1]["ref_kl"] > 0                                             # two optimizer steps in: the policy has left the base
    with open(os.path.join(tmp, "outputs", "part_cli", "train_log.jsonl")) as f:
        assert all("ref_kl" in json.loads(ln) for ln in f)
    bad = subprocess.run([sys.executable, "-m", "mixgrpo_amd.train_grpo_flux"] +
                         _flags(tmp, ["--max_train_steps", "1", "--kl_ref_coeff", "0.1"]),
                         cwd=tmp, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "kl_ref_coeff" in bad.stderr
    assert "loading model" not in bad.stdout                                 # before any weight is read


# ---------------------------------------------------------------------------------------------------- cost
def _record(**kw):
    print(json.dumps(kw))
    if not RECORD_DIR:
        return
    os.makedirs(RECORD_DIR, exist_ok=True)
    path = os.path.join(RECORD_DIR, "ref_kl.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d.update(kw)
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _ms(call, reps):
    call()                                                                   # warm-up: buffers, kernel loads
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def test_ref_kl_timing_is_recorded():
    """Milliseconds per replay of one micro-batch (2 pairs, 512 text + 1024 image tokens) of a 1 + 1 block model at FLUX.1-dev's
    full width, rank-16 adapters on the default targets (11 Linears of 3072 x 3072), device events around 5 calls after a
    warm-up one: the replay with the flag off and on, the reference pass alone, what `reference_policy()` does to the weights
    alone (save, unmerge, restore), the unmerge + merge pair it was chosen over, and the bytes it holds.  Recorded, no
    threshold: nobody has measured the term."""
    from mixgrpo_amd import sampling_utils as SU
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.latents import prepare_latent_image_ids
    REPS, G, L, T = 5, 2, 512, 8
    d0 = torch.device("cuda", 0)
    m = FluxTransformer2DModel(FluxConfig(num_layers=1, num_single_layers=1), device=d0).init_synthetic(seed=5, std=0.02)
    m.add_lora(rank=16, alpha=32)
    _randomise(m.lora, 8, std=0.02)
    m.merge_lora()
    m.train()
    g = torch.Generator(device=d0).manual_seed(0)
    N = 32 * 32
    lat_steps = torch.randn(T + 1, G, N, 64, device=d0, generator=g)
    logp, adv = -torch.rand(G, T, device=d0, generator=g), torch.tensor([1.0, -1.0], device=d0)
    ehs = (0.1 * torch.randn(G, L, 4096, device=d0, generator=g)).to(BF16)
    pooled = torch.randn(G, 768, device=d0, generator=g).to(BF16)
    txt_ids, img_ids = torch.zeros(L, 3, device=d0), prepare_latent_image_ids(1, 32, 32, d0, BF16)
    guidance = torch.tensor([3.5], device=d0, dtype=BF16)
    sig = SU.sd3_time_shift(3.0, torch.linspace(1, 0, T + 1))
    tv = [int(s * 1000) for s in sig][:T]
    pairs = [(0, 1), (1, 1)]

    def replay(coeff):
        args = TG.default_args(sampling_steps=T, kl_ref_coeff=coeff)
        log = torch.zeros(5 if coeff > 0 else 4, device=d0)
        TG._replay_backward(args, m, pairs, lat_steps, logp, adv, ehs, pooled, txt_ids, img_ids, guidance, tv, sig, 2.0, log, None)
        return log

    def ref_pass():
        with torch.autocast("cuda", torch.bfloat16), m.reference_policy():
            return m(lat_steps[1], ehs, torch.tensor([0.5, 0.5], device=d0), guidance, txt_ids, pooled, img_ids)[0]

    def swap_only():
        with m.reference_policy():
            pass

    def unmerge_merge():
        m.lora.unmerge(m.store)
        m.lora.merge(m.store)

    fig = {"replay_ms_flag_off": _ms(lambda: replay(0.0), REPS), "replay_ms_flag_on": _ms(lambda: replay(0.5), REPS),
           "reference_pass_ms": _ms(ref_pass, REPS), "reference_policy_weights_only_ms": _ms(swap_only, REPS),
           "unmerge_merge_pair_ms": _ms(unmerge_merge, REPS), "reference_policy_bytes": m.reference_policy_bytes,
           "bf16_base_copy_bytes": 2 * m.store.numel, "targets": len(m.lora.targets), "pairs": len(pairs), "S": L + N}
    log = replay(0.5)
    assert all(math.isfinite(v) and v > 0 for v in fig.values())
    assert torch.isfinite(log).all() and log[4] > 0
    _record(full_width_1plus1_blocks=fig)
