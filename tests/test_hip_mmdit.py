"""GPU parity of the HIP FLUX MMDiT against the CPU oracle (oracle/mmdit.py; MMDiT parity is UNPINNED with
respect to diffusers, see that file's header).  Tolerances: activations are bf16 with fp32 accumulation in a
different summation order, so stages are compared by relative L2 error (<= 8e-3) and max-abs in bf16 ulps."""
import math

import pytest
import torch

from helpers import make_inputs, small_cfg
from oracle import mmdit as OM

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def build_pair(cfgkw, seed=1):
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    ocfg = OM.FluxConfig(**cfgkw)
    P = OM.init_params(ocfg, seed=seed, std=0.05, bias_std=0.05)
    m = FluxTransformer2DModel(FluxConfig(**cfgkw), device="cuda")
    m.load_state_dict({k: v.cuda() for k, v in P.items()})
    return ocfg, P, m


@pytest.mark.parametrize("B,hg,wg,L", [(1, 8, 8, 64), (2, 8, 12, 40), (3, 5, 7, 24)])
def test_forward_stages_vs_oracle(B, hg, wg, L):
    ocfg, P, m = build_pair(small_cfg(2, 2))
    x, ehs, pooled, ids, tids, t, gd = make_inputs(B, hg, wg, L)
    col_o, col_h = {}, {}
    with torch.no_grad():
        ref = OM.forward(P, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids, collect=col_o)
        m.eval()
        out = m._forward_nograd(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda(),
                                collect=col_h)
    for k in ("temb", "x_embed", "ctx_embed", "double0_h", "double0_c", "double1_h", "double1_c", "single0_x",
              "single1_x"):
        e = rel_err(col_h[k], col_o[k])
        assert e < 8e-3, (k, e)
    assert out.dtype == torch.bfloat16 and out.shape == (B, hg * wg, 64)
    assert rel_err(out, ref) < 1e-2


def test_call_signature_and_state_dict_roundtrip(tmp_path):
    ocfg, P, m = build_pair(small_cfg(1, 1))
    x, ehs, pooled, ids, tids, t, gd = make_inputs(1, 4, 4, 16)
    m.eval()
    out = m(hidden_states=x.cuda(), encoder_hidden_states=ehs.cuda(), timestep=t[:1].cuda(), guidance=gd.cuda(),
            txt_ids=tids.cuda(), pooled_projections=pooled.cuda(), img_ids=ids.cuda(), joint_attention_kwargs=None,
            return_dict=False)[0]
    sd = m.state_dict()
    assert set(sd) == set(OM.param_shapes(ocfg))
    for k, shp in OM.param_shapes(ocfg).items():
        assert tuple(sd[k].shape) == shp
    m.save_pretrained(str(tmp_path / "checkpoint-0-0"))
    from mixgrpo_amd.flux import FluxTransformer2DModel
    m2 = FluxTransformer2DModel.from_pretrained(str(tmp_path / "checkpoint-0-0"))
    m2.eval()
    out2 = m2(x.cuda(), ehs.cuda(), t[:1].cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    assert torch.equal(out, out2)
    assert dict(m2.config)["num_attention_heads"] == 4


def test_attention_kernel_vs_torch():
    """Flash attention forward alone at FLUX head geometry (S=4608 would be the full size; 1100 exercises masking)."""
    from mixgrpo_amd import ops
    B, H, S = 2, 3, 1100
    Sp = (S + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    vt = torch.zeros(B, H, 128, Sp, device="cuda", dtype=torch.bfloat16)
    vt[..., :S] = v.transpose(-1, -2)
    O = torch.empty(B, S, H * 128, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device="cuda")
    ops.attn_fwd(q, k, vt, O, lse, B, H, S, Sp, H * 128, S * H * 128, 1 / math.sqrt(128))
    s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(128)
    ref = (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(B, S, H * 128)
    assert rel_err(O, ref) < 6e-3
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,hg,wg,L", [(1, 8, 8, 64), (2, 6, 10, 24)])
def test_backward_vs_oracle_autograd(B, hg, wg, L):
    """d(sum(out * R))/d(params) through the HIP backward (block recompute) vs torch autograd of the oracle.
    Activation grads are bf16 on both sides (different rounding points): per-tensor relative L2 error <= 4e-2,
    and the global gradient direction must agree to cosine >= 0.999."""
    ocfg, P, m = build_pair(small_cfg(2, 2))
    x, ehs, pooled, ids, tids, t, gd = make_inputs(B, hg, wg, L, seed=3)
    R = torch.randn(B, hg * wg, 64, generator=torch.Generator().manual_seed(9))
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = OM.forward(Pg, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids)
    (ref * R).sum().backward()
    m.train()
    out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    assert out.requires_grad
    (out.float() * R.cuda()).sum().backward()
    g = m.store.g32
    assert m.flat_param.grad is g
    dots = nh = no = 0.0
    worst = []
    for k in P:
        gh = m.store.view(g, k).float().cpu()
        go = Pg[k].grad
        dots += (gh * go).sum().item()
        nh += gh.pow(2).sum().item()
        no += go.pow(2).sum().item()
        e = ((gh - go).norm() / (go.norm() + 1e-9)).item()
        worst.append((e, k))
    worst.sort(reverse=True)
    cos = dots / math.sqrt(nh * no)
    assert cos > 0.999, (cos, worst[:5])
    assert worst[0][0] < 4e-2, worst[:8]
    # a second backward accumulates (gradient accumulation over replayed steps)
    out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    (out.float() * R.cuda()).sum().backward()
    k0 = "transformer_blocks.0.ff.net.2.weight"
    assert rel_err(m.store.view(g, k0), 2 * Pg[k0].grad) < 4e-2


@pytest.mark.parametrize("growth", [0.0, 3.0, 40.0])
def test_attention_deferred_rescale_paths(growth):
    """The forward's online softmax raises its running maximum only when a row outgrows it by 2^6 (attention.hip,
    DEFER): keys whose scores GROW along the sequence force, per 64-key tile, either the deferred path with P > 1
    (growth 3: ~2^0.3 per tile) or the rescale branch over and over (growth 40), at a ragged length; a random-data check
    alone never leaves the first-tile rescale.  Tolerances as test_attention_kernel_vs_torch."""
    from mixgrpo_amd import ops
    B, H, S = 1, 3, 1000
    Sp = (S + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(2)
    q = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    base = torch.randn(B, H, S, 128, device="cuda", generator=g)
    ramp = torch.linspace(0, 1, S, device="cuda").view(1, 1, S, 1)
    k = (base + growth * ramp * q.float().mean(dim=2, keepdim=True).sign()).bfloat16()   # scores drift upwards with the key index
    v = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    vt = torch.cat([v.transpose(-1, -2), torch.zeros(B, H, 128, Sp - S, device="cuda", dtype=v.dtype)], -1).contiguous()
    O = torch.empty(B, S, H * 128, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device="cuda")
    ops.attn_fwd(q, k, vt, O, lse, B, H, S, Sp, H * 128, S * H * 128, 1 / math.sqrt(128))
    s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(128)
    ref = (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(B, S, H * 128)
    assert torch.isfinite(O.float()).all()
    assert rel_err(O, ref) < 6e-3
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-4, atol=1e-4)


# the kernel mgx_attn_fwd* takes with MGX_ATTN_W64 unset or 1 (ops.attn_fwd_path): S % 256 == 0 is not enough, the persistent
# walk needs stride / nq < H (csrc/attention.hip).  (1, 1, 256): one block, stride 1, 1 / 1 < 1 fails; (2, 3, 768): 18 blocks, not
# a multiple of 8, stride 18, 18 / 3 < 3 fails -- both are 8-wave cases on either setting of the switch.
FWD64_PATH = {(1, 1, 256): 0, (2, 3, 768): 0, (1, 24, 1536): 1, (2, 4, 512): 1, (3, 8, 512): 1}


@pytest.mark.parametrize("B,H,S,ldo_mult", [(1, 1, 256, 1), (2, 3, 768, 5), (1, 24, 1536, 1), (2, 4, 512, 1), (3, 8, 512, 5)])
def test_attention_fwd64_vs_torch_and_vs_the_8_wave_kernel(B, H, S, ldo_mult, monkeypatch):
    """The 64-query-wave forward (generated instruction stream, csrc/gen/attn_fwd64.py; shapes with FWD64_PATH 1: B > 1, a walk
    that carries into the next batch) against an fp32 torch softmax(Q K^T / sqrt(d)) V, and against the 8-wave kernel on the same
    operands (MGX_ATTN_W64=0): same tolerance to the reference, agreement between the two within bf16 rounding of O, columns
    beyond the head block untouched.  (1, 1, 256) and (2, 3, 768) have S % 256 == 0 but take the 8-wave kernel on both legs
    (FWD64_PATH 0): for them the comparison of the two legs is a comparison of that kernel with itself.  Each leg asserts the
    kernel it ran; tests/test_hip_attention_kernels.py holds the per-row float64 checks."""
    from mixgrpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(S + H)
    q, k, v = (torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16() for _ in range(3))
    vt = v.transpose(-1, -2).contiguous()
    ldo = H * 128 * ldo_mult
    outs = []
    for w64 in ("1", "0"):
        monkeypatch.setenv("MGX_ATTN_W64", w64)
        assert ops.attn_fwd_path(B, H, S, S, ldo, S * ldo) == (FWD64_PATH[(B, H, S)] if w64 == "1" else 0)
        O = torch.zeros(B, S, ldo, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, H, S, device="cuda")
        ops.attn_fwd(q, k, vt, O, lse, B, H, S, S, ldo, S * ldo, 1 / math.sqrt(128))
        outs.append((O, lse))
    s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(128)
    ref = (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(B, S, H * 128)
    for O, lse in outs:
        assert rel_err(O[:, :, :H * 128], ref) < 6e-3
        assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-4, atol=1e-4)
        assert not O[:, :, H * 128:].any()
    assert rel_err(outs[0][0], outs[1][0].float()) < 4e-3
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=2e-5)


def test_attention_fwd64_rescale_path():
    """The 64-query-wave forward keeps the FIRST tile's row maximum and only rescales when a tile's row sum passes 2^40
    (csrc/gen/attn_fwd64.py).  Keys that outscore their query's first-tile maximum by ~90 and ~65 nats force that rare
    path (fp32 overflow of the tile's row sum -> fix-up) in a middle tile and in the last one; a query in each of the two
    chains of a wave is hit.  Full-tensor fp32 reference (MI355X guide, rule 26)."""
    from mixgrpo_amd import ops
    B, H, S = 1, 2, 1024
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16() for _ in range(3))
    k[:, :, 200] = (8 * q[:, :, 70].float()).bfloat16()        # query 70: wave 1, chain A of the first query block
    k[:, :, S - 3] = (6 * q[:, :, 100].float()).bfloat16()     # query 100: wave 1, chain B; last tile
    k[:, :, 333] = (7 * q[:, :, 700].float()).bfloat16()       # third query block
    O = torch.empty(B, S, H * 128, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device="cuda")
    assert ops.attn_fwd_path(B, H, S, S, H * 128, S * H * 128) == 1           # the 64-query kernel: the fix-up is its code
    ops.attn_fwd(q, k, v.transpose(-1, -2).contiguous(), O, lse, B, H, S, S, H * 128, S * H * 128, 1 / math.sqrt(128))
    s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(128)
    ref = (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(B, S, H * 128)
    assert torch.isfinite(O.float()).all()
    assert rel_err(O, ref) < 6e-3
    got = O.view(B, S, H, 128).permute(0, 2, 1, 3)
    refh = ref.view(B, S, H, 128).permute(0, 2, 1, 3)
    for row in (70, 100, 700):                                  # the spiked rows themselves: O = the spiked key's V row
        assert rel_err(got[:, :, row], refh[:, :, row]) < 6e-3
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("B,H,S,ldo_mult", [(1, 2, 256, 1), (2, 3, 768, 5), (1, 6, 1536, 1)])
def test_attention_bwd64_vs_autograd_and_vs_the_8_wave_kernels(B, H, S, ldo_mult, monkeypatch):
    """The 64-wide backward kernels (S % 256 == 0: generated instruction streams, csrc/gen/attn_bwd_*64.py) against torch
    autograd of softmax(Q K^T / sqrt(d)) V in fp32, and against the 8-wave kernels on the same operands (MGX_ATTN_W64=0)."""
    from mixgrpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(S + 7 * H)
    q, k, v = (torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16() for _ in range(3))
    ldo = H * 128 * ldo_mult
    do = torch.randn(B, S, ldo, device="cuda", generator=g).bfloat16()
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) / math.sqrt(128)
    o_ref = (torch.softmax(s, -1) @ vf).transpose(1, 2).reshape(B, S, H * 128)
    o_ref.backward(do[:, :, :H * 128].float())
    tr = lambda t: t.transpose(-1, -2).contiguous()
    vt, qt, kt = tr(v), tr(q), tr(k)
    outs = []
    for w64 in ("1", "0"):
        monkeypatch.setenv("MGX_ATTN_W64", w64)
        assert ops.attn_bwd_path(B, H, S, S, ldo, S * ldo) == int(w64)        # the backward has no walk: every S % 256 == 0 shape
        O = torch.zeros(B, S, ldo, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, H, S, device="cuda")
        ops.attn_fwd(q, k, vt, O, lse, B, H, S, S, ldo, S * ldo, 1 / math.sqrt(128))
        dQ, dK, dV = (torch.full_like(q, float("nan")) for _ in range(3))
        delta = torch.empty(B, H, S, device="cuda")
        dOt = torch.zeros(B, H, 128, S, device="cuda", dtype=torch.bfloat16)
        ops.attn_bwd(q, k, v, qt, kt, O, do, lse, delta, dOt, dQ, dK, dV, B, H, S, S, ldo, S * ldo, 1 / math.sqrt(128))
        assert rel_err(dV, vf.grad) < 1e-2
        assert rel_err(dK, kf.grad) < 1.5e-2
        assert rel_err(dQ, qf.grad) < 1.5e-2
        outs.append((dQ, dK, dV))
    for a_, b_ in zip(*outs):
        assert rel_err(a_, b_.float()) < 8e-3


def test_selective_saving_is_bit_identical_to_full_recompute(monkeypatch):
    """The training forward keeps the attention output / LSE and the pre-gate outputs of to_out, ff.net.2 and proj_out so
    that the recompute pass skips attention and those GEMMs (flux_backward._Train.keep).  The kept values are the very
    values a recompute would produce, so the gradients must be bit-identical to full block recompute."""
    from mixgrpo_amd import flux_backward as FB
    grads = []
    # (True, "3"): additionally the FF pre-activation of the first three blocks (two double + one single) is kept and their
    # d -> 4d GEMM is replaced by an elementwise GELU in the recompute (FB.KEEP_FF)
    # (..., "2") / (..., "99"): additionally the QKV projection's output of the first two / of all blocks is kept and the
    # recompute skips the d -> 3d GEMM (FB.KEEP_QKV); with ("99", "99") the recompute pass runs no GEMM at all
    for keep, keep_ff, keep_qkv in ((True, "0", "0"), (False, "0", "0"), (True, "3", "0"), (True, "99", "0"), (True, "1", "2"),
                                    (True, "99", "99")):
        monkeypatch.setattr(FB, "KEEP_ACTS", keep)
        monkeypatch.setattr(FB, "KEEP_FF", keep_ff)
        monkeypatch.setattr(FB, "KEEP_QKV", keep_qkv)
        ocfg, P, m = build_pair(small_cfg(2, 2))
        x, ehs, pooled, ids, tids, t, gd = make_inputs(2, 6, 10, 24, seed=3)
        R = torch.randn(2, 60, 64, generator=torch.Generator().manual_seed(9)).cuda()
        m.train()
        out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
        (out.float() * R).sum().backward()
        w = next(iter(m._work.values()))
        assert (w.train.keep is not None) == keep
        if keep:
            assert w.train.ff_kept() == min(int(keep_ff), 4)
            assert w.train.qkv_kept() == min(int(keep_qkv), 4)
        grads.append((out.detach().clone(), m.store.g32.clone()))
    for other in grads[1:]:
        assert torch.equal(grads[0][0], other[0])
        assert torch.equal(grads[0][1], other[1])


@pytest.mark.parametrize("keep,keep_ff,keep_qkv,gelu,gate_res,attn", [
    (False, "0", "0", 2 * 2 + 2, 4 * 2 + 2, 4),      # full recompute: every block's ff.net.0 / proj_mlp, to_out / ff.net.2 / proj_out, attention
    (True, "0", "0", 2 * 2 + 2, 0, 0),               # kept O / lse / y_attn / y_ff / x_mid: only the up-projections run again
    (True, "99", "99", 0, 0, 0)])                    # everything kept: the recompute pass runs no GEMM and no attention
def test_recompute_pass_runs_only_what_was_not_kept(monkeypatch, keep, keep_ff, keep_qkv, gelu, gate_res, attn):
    """What `backward()` launches again of the forward at 2 + 2 blocks, counted per GEMM epilogue (the backward's own GEMMs
    are EPI_BIAS / EPI_DGELU / EPI_F32_ACC) and per attention forward."""
    from mixgrpo_amd import flux_backward as FB
    from mixgrpo_amd import ops
    from mixgrpo_amd.flux import FluxTransformer2DModel
    monkeypatch.setattr(FB, "KEEP_ACTS", keep)
    monkeypatch.setattr(FB, "KEEP_FF", keep_ff)
    monkeypatch.setattr(FB, "KEEP_QKV", keep_qkv)
    ocfg, P, m = build_pair(small_cfg(2, 2))
    x, ehs, pooled, ids, tids, t, gd = make_inputs(2, 6, 10, 24, seed=3)
    m.train()
    out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    counts = {"attn": 0}
    gemm, attn_fwd = ops.gemm, FluxTransformer2DModel._attn

    def counted_gemm(A, W, bias, C, N, K, epi=ops.EPI_BIAS, **kw):
        counts[epi] = counts.get(epi, 0) + 1
        return gemm(A, W, bias, C, N, K, epi, **kw)

    def counted_attn(self, *a, **kw):
        counts["attn"] += 1
        return attn_fwd(self, *a, **kw)

    monkeypatch.setattr(ops, "gemm", counted_gemm)
    monkeypatch.setattr(FluxTransformer2DModel, "_attn", counted_attn)
    out.float().sum().backward()
    assert (counts.get(ops.EPI_BIAS_GELU, 0), counts.get(ops.EPI_BIAS_GATE_RES, 0), counts["attn"]) == (gelu, gate_res, attn), counts


def test_attention_backward_vs_torch():
    from mixgrpo_amd import ops
    B, H, S = 1, 2, 700
    Sp = (S + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, S, H * 128, device="cuda", generator=g).bfloat16()
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) / math.sqrt(128)
    o_ref = (torch.softmax(s, -1) @ vf).transpose(1, 2).reshape(B, S, H * 128)
    o_ref.backward(do.float())
    pad = lambda t: torch.cat([t.transpose(-1, -2), torch.zeros(B, H, 128, Sp - S, device="cuda", dtype=t.dtype)], -1).contiguous()
    vt, qt, kt = pad(v), pad(q), pad(k)
    O = torch.empty(B, S, H * 128, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device="cuda")
    ops.attn_fwd(q, k, vt, O, lse, B, H, S, Sp, H * 128, S * H * 128, 1 / math.sqrt(128))
    dQ, dK, dV = (torch.empty_like(q) for _ in range(3))
    delta = torch.empty(B, H, S, device="cuda")
    dOt = torch.zeros(B, H, 128, Sp, device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(q, k, v, qt, kt, O, do, lse, delta, dOt, dQ, dK, dV, B, H, S, Sp, H * 128, S * H * 128, 1 / math.sqrt(128))
    assert rel_err(dV, vf.grad) < 1e-2
    assert rel_err(dK, kf.grad) < 1.5e-2
    assert rel_err(dQ, qf.grad) < 1.5e-2


def test_attention_full_size_properties():
    """BASELINE-size attention (H = 24, S = 4608 = 512 text + 4096 image tokens, head_dim 128) through properties that do
    not need a full-size reference: rows of P sum to one (V = 1 gives O = 1 exactly), sampled query rows against an fp32
    torch reference, invariance under a joint permutation of the keys and values, and for the backward the scale identity
    sum_i <q_i, dq_i> = sum_j <k_j, dk_j> (both equal sum_ij P_ij dS_ij s_ij) plus sampled rows of dV."""
    from mixgrpo_amd import ops
    B, H, S = 1, 24, 4608
    Sp = S
    sc = 1 / math.sqrt(128)
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()

    def fwd(q_, k_, v_):
        O = torch.empty(B, S, H * 128, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, H, S, device="cuda")
        ops.attn_fwd(q_, k_, v_.transpose(-1, -2).contiguous(), O, lse, B, H, S, Sp, H * 128, S * H * 128, sc)
        return O.view(B, S, H, 128).permute(0, 2, 1, 3), lse

    ones = torch.ones_like(v)
    O1, _ = fwd(q, k, ones)
    assert torch.equal(O1.float(), torch.ones_like(O1).float())                    # sum_j P_ij = 1, exactly 1.0 in bf16
    O, lse = fwd(q, k, v)
    rows = torch.randint(0, S, (96,), generator=torch.Generator().manual_seed(1)).cuda()
    s = (q[:, :, rows].float() @ k.float().transpose(-1, -2)) * sc                 # [B, H, 96, S]
    ref = torch.softmax(s, -1) @ v.float()
    assert rel_err(O[:, :, rows], ref) < 6e-3
    assert torch.allclose(lse[:, :, rows], torch.logsumexp(s, -1), rtol=1e-4, atol=1e-4)
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(2)).cuda()
    Op, lsep = fwd(q, k[:, :, perm].contiguous(), v[:, :, perm].contiguous())
    assert rel_err(Op, O.float()) < 4e-3 and torch.allclose(lsep, lse, rtol=1e-5, atol=1e-5)   # only the summation order moved

    do = torch.randn(B, S, H * 128, device="cuda", generator=g).bfloat16()
    Oc = O.permute(0, 2, 1, 3).reshape(B, S, H * 128).contiguous()
    tr = lambda t: t.transpose(-1, -2).contiguous()
    dQ, dK, dV = (torch.empty_like(q) for _ in range(3))
    delta = torch.empty(B, H, S, device="cuda")
    dOt = torch.zeros(B, H, 128, Sp, device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(q, k, v, tr(q), tr(k), Oc, do, lse, delta, dOt, dQ, dK, dV, B, H, S, Sp, H * 128, S * H * 128, sc)
    torch.cuda.synchronize()
    lhs = (q.double() * dQ.double()).sum(dim=(2, 3))
    rhs = (k.double() * dK.double()).sum(dim=(2, 3))
    assert torch.allclose(lhs, rhs, rtol=2e-2, atol=2e-2 * lhs.abs().mean().item()), (lhs - rhs).abs().max()
    # dV[j] = sum_i P_ij dO_i on sampled keys (P from the fp32 reference scores of ALL queries against those keys)
    keys = rows[:32]
    dOh = do.view(B, S, H, 128).permute(0, 2, 1, 3).float()
    sk = (q.float() @ k[:, :, keys].float().transpose(-1, -2)) * sc                # [B, H, S, 32]
    Pk = torch.exp(sk - lse.unsqueeze(-1))
    assert rel_err(dV[:, :, keys], Pk.transpose(-1, -2) @ dOh) < 1.5e-2


def test_full_width_blocks_vs_oracle():
    """BASELINE.json configs[0] geometry at FULL width: d = 3072 (24 heads x 128), joint_attention_dim 4096, pooled 768,
    1 double + 1 single block, N = 1024 image tokens (64x64 latent) + 512 text tokens.  Everything the FLUX.1-dev step
    runs is on this path at its real width (persistent 256x256 GEMM with every epilogue, fused QKV views, full RoPE axes,
    24-head attention forward / backward, wgrad / dgrad shapes); forward and parameter gradients against the CPU oracle."""
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    kw = dict(num_layers=1, num_single_layers=1)                     # every other field: the FLUX.1-dev default
    ocfg = OM.FluxConfig(**kw)
    P = OM.init_params(ocfg, seed=2, std=0.02, bias_std=0.02)
    m = FluxTransformer2DModel(FluxConfig(**kw), device="cuda")
    m.load_state_dict({k: v.cuda() for k, v in P.items()})
    g = torch.Generator().manual_seed(4)
    B, hg, wg, L = 1, 32, 32, 512
    N = hg * wg
    x = torch.randn(B, N, 64, generator=g)
    ehs = (0.1 * torch.randn(B, L, 4096, generator=g)).bfloat16()
    pooled = torch.randn(B, 768, generator=g).bfloat16()
    ids = torch.zeros(hg, wg, 3)
    ids[..., 1] += torch.arange(hg)[:, None]
    ids[..., 2] += torch.arange(wg)[None]
    ids = ids.reshape(N, 3)
    tids, t, gd = torch.zeros(L, 3), torch.tensor([0.954]), torch.tensor([3.5]).bfloat16()
    R = torch.randn(B, N, 64, generator=g)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = OM.forward(Pg, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids)
    (ref * R).sum().backward()
    m.train()
    out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    assert rel_err(out, ref) < 1e-2
    (out.float() * R.cuda()).sum().backward()
    gbuf = m.store.g32
    dots = nh = no = 0.0
    worst = []
    for k in P:
        gh = m.store.view(gbuf, k).float().cpu()
        go = Pg[k].grad
        dots += (gh * go).sum().item()
        nh += gh.pow(2).sum().item()
        no += go.pow(2).sum().item()
        worst.append((((gh - go).norm() / (go.norm() + 1e-9)).item(), k))
    worst.sort(reverse=True)
    assert dots / math.sqrt(nh * no) > 0.999, (dots / math.sqrt(nh * no), worst[:5])
    assert worst[0][0] < 5e-2, worst[:8]


# measured (profiles/r03_depth_parity.json): forward rel-L2 5.9e-3 / 8.0e-3 / 1.03e-2 / 1.69e-2, gradient cosine
# 0.99998 / 0.99996 / 0.99993 / 0.99981, worst single tensor 1.3e-2 / 1.7e-2 / 2.0e-2 / 3.2e-2: the bounds sit ~1.5 x above
DEPTH_BOUNDS = {(1, 1): (9e-3, 0.99995, 2.5e-2), (2, 2): (1.2e-2, 0.9999, 3e-2), (4, 8): (1.6e-2, 0.9998, 3.5e-2),
                (19, 38): (2.5e-2, 0.9995, 5e-2)}


@pytest.mark.parametrize("nd,ns", [(1, 1), (2, 2), (4, 8), pytest.param(19, 38, id="flux1dev_full_depth_19+38")])
def test_full_width_error_vs_depth(nd, ns):
    """Forward rel-L2 and parameter-gradient cosine against the CPU oracle at FULL width (d = 3072) for 1+1, 2+2, 4+8 blocks
    and FLUX.1-dev's FULL depth, 19 + 38 blocks = 11.9 B parameters (round 3 ran that case as a one-off script; it is in the
    driver-run suite now; its oracle pass runs on the device, see below), 64 image + 32 text tokens
    (the CPU oracle's time is the weights'): how the bf16 error compounds with depth.  Numbers go to
    gpurun_out/r04_depth_parity.json; DESIGN.md section 2 quotes them."""
    import json
    import os
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    if (nd, ns) == (19, 38):
        torch.set_num_threads(max(torch.get_num_threads(), min(16, os.cpu_count() or 1)))
    kw = dict(num_layers=nd, num_single_layers=ns)
    ocfg = OM.FluxConfig(**kw)
    # the weights are drawn ON THE DEVICE (the product's `init_synthetic`: N(0, 0.02^2) matrices and biases, norm weights
    # 1 + N(0, 0.02^2)) and handed to the oracle: both sides hold the same fp32 values, and 11.9 B normals take a second
    # instead of the minutes a host generator needs.
    # Where the oracle runs: 1+1 / 2+2 / 4+8 on the host CPU like every other oracle test.  At 19 + 38 the oracle's (device-
    # agnostic, plain fp32 torch) code runs with its tensors ON THE GPU: the same restatement, executed by torch's own fp32
    # kernels instead of the host's BLAS -- the host pass took 130-290 s depending on the box's cores (round 3's one-off:
    # 131 s), too much of the driver's 900 s suite limit; on the device it takes seconds.  Nothing of the product is on the
    # oracle's side either way.
    m = FluxTransformer2DModel(FluxConfig(**kw), device="cuda").init_synthetic(seed=2, std=0.02, bias_std=0.02)
    odev = "cuda" if (nd, ns) == (19, 38) else "cpu"
    P = {k: (v.detach().clone() if odev == "cuda" else v.detach().cpu()) for k, v in m.state_dict().items()}
    assert set(P) == set(OM.param_shapes(ocfg))
    g = torch.Generator().manual_seed(4)
    B, hg, wg, L = 1, 8, 8, 32
    N = hg * wg
    x = torch.randn(B, N, 64, generator=g)
    ehs = (0.1 * torch.randn(B, L, 4096, generator=g)).bfloat16()
    pooled = torch.randn(B, 768, generator=g).bfloat16()
    ids = torch.zeros(hg, wg, 3)
    ids[..., 1] += torch.arange(hg)[:, None]
    ids[..., 2] += torch.arange(wg)[None]
    ids = ids.reshape(N, 3)
    tids, t, gd = torch.zeros(L, 3), torch.tensor([0.954]), torch.tensor([3.5]).bfloat16()
    R = torch.randn(B, N, 64, generator=g)
    Pg = {k: v.requires_grad_(True) for k, v in P.items()}
    to = lambda a: a.to(odev)
    ref = OM.forward(Pg, ocfg, to(x), to(ehs.float()), to(t), to(gd.float()), to(tids), to(pooled.float()), to(ids))
    (ref * to(R)).sum().backward()
    ref = ref.detach().cpu()
    m.train()
    out = m(x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())[0]
    fwd = rel_err(out, ref)
    (out.float() * R.cuda()).sum().backward()
    # the comparison runs on the device in fp64 (the oracle's gradient is copied over tensor by tensor): five passes over
    # 2 x 47.6 GB are seconds there
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    worst = torch.zeros((), dtype=torch.float64, device="cuda")
    for k in P:
        gh = m.store.view(m.store.g32, k).double()
        go = Pg[k].grad.cuda().double()
        acc += torch.stack([(gh * go).sum(), gh.pow(2).sum(), go.pow(2).sum()])
        worst = torch.maximum(worst, (gh - go).norm() / (go.norm() + 1e-9))
        Pg[k].grad = None
    dots, nh, no = acc.tolist()
    worst = worst.item()
    cos = dots / math.sqrt(nh * no)
    os.makedirs("gpurun_out", exist_ok=True)
    path = os.path.join("gpurun_out", "r04_depth_parity.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[f"fwd_bwd_{nd}+{ns}"] = dict(forward_rel_l2=fwd, grad_cosine=cos, worst_tensor_rel=worst)
    json.dump(old, open(path, "w"), indent=1)
    b_fwd, b_cos, b_worst = DEPTH_BOUNDS[(nd, ns)]
    assert fwd < b_fwd, fwd
    assert cos > b_cos, cos
    assert worst < b_worst, worst
    del Pg, P, ref, m                                    # (19 + 38: ~150 GB of host memory and 120 GB of HBM go back now)
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def test_second_forward_before_backward_is_refused():
    """The training forward keeps its activations in the model's shared workspace: a second grad-enabled forward before the
    first one's backward overwrites them, so that backward must fail loudly instead of returning wrong gradients."""
    from mixgrpo_amd._lib import MgxError
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    cfg = FluxConfig(**small_cfg(1, 1))
    m = FluxTransformer2DModel(cfg, device="cuda").init_synthetic(seed=1, std=0.05)
    m.train()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 16, 64, generator=g).cuda()
    kw = dict(encoder_hidden_states=(0.1 * torch.randn(1, 8, 64, generator=g)).bfloat16().cuda(),
              timestep=torch.tensor([0.5]).cuda(), guidance=torch.tensor([3.5]).bfloat16().cuda(),
              txt_ids=torch.zeros(8, 3).cuda(), pooled_projections=torch.randn(1, 32, generator=g).bfloat16().cuda(),
              img_ids=torch.zeros(16, 3).cuda(), joint_attention_kwargs=None, return_dict=False)
    out1 = m(hidden_states=x, **kw)[0]
    out2 = m(hidden_states=x * 0.5, **kw)[0]
    with pytest.raises(MgxError, match="overwritten"):
        out1.float().sum().backward()
    out2.float().sum().backward()                         # the latest forward's backward is fine
    assert m.flat_param.grad is not None and torch.isfinite(m.flat_param.grad).all()
