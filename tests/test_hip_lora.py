"""LoRA fine-tuning on the GPU: the rank-r kernels of csrc/lora.hip against fp64, the merged forward, the adapter gradients
against torch autograd of the oracle with parameters W0 + s B A, the optimizer step, adapter files, a train step and two-rank
data parallelism.

Exact cases use operands on a grid whose every partial sum is exact in fp32 (activations randint(-4, 5) / 8, adapters
randint(-2, 3) / 4, power-of-two scales), so any summation order gives the fp64 result bit for bit."""
import math
import os

import pytest
import torch

from oracle import mmdit as OM
from helpers import grid as _grid, run_ranks
from test_hip_mmdit import build_pair, make_inputs, small_cfg

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _operand(M, Kin, layout, gen, make):
    """An [M, Kin] activation as `ops.Rows` in one of the layouts the backward uses, and the same values as a plain matrix.
    "plain"; "cols": the column slice at offset Kin of a [M, 3 Kin] matrix (ld = 3 Kin); "batched": 3 batches of rows inside a larger
    buffer with a batch stride (rows per batch < M)."""
    from mixgrpo_amd.ops import Rows
    if layout == "plain":
        t = make((M, Kin))
        return Rows.of(t), t
    if layout == "cols":
        big = make((M, 3 * Kin))
        return Rows(big.view(-1)[Kin:], M, 3 * Kin), big[:, Kin:2 * Kin]
    assert layout == "batched" and M % 3 == 0
    rpb, pad = M // 3, 5
    big = make((3, rpb + pad, Kin))
    return Rows(big[0, pad:], M, Kin, rpb, (rpb + pad) * Kin), big[:, pad:].reshape(M, Kin)


EXACT_CASES = [(1, 512, 16, "plain"), (63, 512, 64, "plain"), (177, 2048, 128, "plain"), (1100, 512, 16, "plain"),
               (1100, 2048, 64, "plain"), (1100, 512, 128, "plain"), (177, 512, 64, "cols"), (177, 512, 16, "batched"),
               # Kin = 64: proj has 2 K-steps for its 4 waves, and the only 128-column block of the wgrad is half empty
               (63, 64, 16, "plain"),
               # r = 32: lora_proj_kernel<32> / lora_wgrad_kernel<32> (their own small_stride, 48, and staging count);
               # Kin % 128 = 64: the last column block of the wgrad is half empty (`c0 + ch*8 < Kin`, `col < Kin`)
               (177, 192, 32, "plain"), (1100, 512, 32, "plain"), (177, 192, 32, "cols"), (177, 64, 32, "batched"),
               (177, 192, 128, "plain")]


@pytest.mark.parametrize("M,Kin,r,layout", EXACT_CASES)
def test_proj_and_wgrad_exact_on_the_grid_and_deterministic(M, Kin, r, layout):
    from mixgrpo_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(M * 7 + Kin + r)
    rows, X = _operand(M, Kin, layout, gen, lambda s: _grid(s, -4, 5, 8, gen))
    P = _grid((r, Kin), -2, 3, 4, gen)
    small = _grid((M, r), -4, 5, 8, gen)
    scale = 0.25
    ref_proj = (scale * (X.double() @ P.double().t())).to(BF16)
    ref_g = small.double().t() @ X.double()
    G0 = _grid((r, Kin), -4, 5, 8, gen, dtype=F32)
    outs = []
    for _ in range(2):
        out = torch.empty(M, r, dtype=BF16, device="cuda")
        ops.lora_proj(rows, P, out, Kin, r, scale)
        g_new = torch.full((r, Kin), float("nan"), device="cuda")          # beta = 0 must not read G
        ops.lora_wgrad(small, rows, g_new, Kin, r, beta=0.0)
        g_acc = G0.clone()
        ops.lora_wgrad(small, rows, g_acc, Kin, r, beta=1.0)
        outs.append((out, g_new, g_acc))
    out, g_new, g_acc = outs[0]
    assert torch.equal(out, ref_proj)
    assert torch.equal(g_new.double(), ref_g)
    assert torch.equal(g_acc.double(), G0.double() + ref_g)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    if M == 1100:
        assert ops.lora_wgrad_workspace(M, Kin, r) > r * Kin                # several row chunks: the second stage really adds


@pytest.mark.parametrize("M,Kin,r", [(177, 512, 16), (1100, 2048, 64), (1100, 512, 128), (1100, 192, 32)])
def test_proj_and_wgrad_random_vs_fp64(M, Kin, r):
    from mixgrpo_amd import ops
    from mixgrpo_amd.ops import Rows
    gen = torch.Generator(device="cuda").manual_seed(11)
    X = torch.randn(M, Kin, device="cuda", generator=gen).to(BF16)
    P = torch.randn(r, Kin, device="cuda", generator=gen).to(BF16)
    small = torch.randn(M, r, device="cuda", generator=gen).to(BF16)
    out = torch.empty(M, r, dtype=BF16, device="cuda")
    ops.lora_proj(Rows.of(X), P, out, Kin, r, 0.7)
    G = torch.zeros(r, Kin, device="cuda")
    ops.lora_wgrad(small, Rows.of(X), G, Kin, r, beta=0.0)
    e_proj = _rel(out, 0.7 * (X.double() @ P.double().t()))
    e_wgrad = _rel(G, small.double().t() @ X.double())
    print(f"M {M} Kin {Kin} r {r}: proj rel-L2 {e_proj:.3e}  wgrad rel-L2 {e_wgrad:.3e}")
    assert e_wgrad < 1e-5          # the bound of tests/test_hip_gemm.py::test_gemm_f32_accumulate on the same arithmetic
    assert e_proj < 2.0e-3         # one RNE rounding <= 2^-9 per element + the accumulation bound above


def test_kernels_refuse_unsupported_sizes():
    from mixgrpo_amd import ops
    from mixgrpo_amd._lib import MgxError
    from mixgrpo_amd.ops import Rows
    X = torch.zeros(64, 96, dtype=BF16, device="cuda")
    with pytest.raises(MgxError):
        ops.lora_proj(Rows.of(X), torch.zeros(16, 96, dtype=BF16, device="cuda"), torch.zeros(64, 16, dtype=BF16, device="cuda"), 96, 16, 1.0)
    X = torch.zeros(64, 128, dtype=BF16, device="cuda")
    with pytest.raises(MgxError):
        ops.lora_proj(Rows.of(X), torch.zeros(24, 128, dtype=BF16, device="cuda"), torch.zeros(64, 24, dtype=BF16, device="cuda"), 128, 24, 1.0)
    with pytest.raises(ValueError):
        ops.lora_wgrad_workspace(64, 128, 24)


def test_merge_exact_on_the_grid():
    from mixgrpo_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(3)
    N, K, r = 200, 512, 32
    W0 = _grid((N, K), -4, 5, 8, gen, dtype=F32)
    Bt = _grid((r, N), -2, 3, 4, gen, dtype=F32)
    A = _grid((r, K), -2, 3, 4, gen, dtype=F32)
    W16 = torch.empty(N, K, dtype=BF16, device="cuda")
    ops.lora_merge(W0, Bt, A, W16, N, K, r, 0.5)
    assert torch.equal(W16, (W0.double() + 0.5 * (Bt.double().t() @ A.double())).to(BF16))


@pytest.mark.parametrize("N,K,r", [(512, 512, 16), (1536, 512, 64), (2048, 512, 128)])
def test_merge_random_within_one_ulp(N, K, r):
    from mixgrpo_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(4)
    W0, Bt, A = (torch.randn(s, device="cuda", generator=gen) * 0.05 for s in ((N, K), (r, N), (r, K)))
    W16 = torch.empty(N, K, dtype=BF16, device="cuda")
    ops.lora_merge(W0, Bt, A, W16, N, K, r, 2.0)
    ref = (W0.double() + 2.0 * (Bt.double().t() @ A.double())).to(BF16)
    # bf16 neighbours of the reference: a differing element must be one of them
    bits, rbits = W16.view(torch.int16).to(torch.int32), ref.view(torch.int16).to(torch.int32)
    diff = bits != rbits
    share = diff.float().mean().item()
    print(f"N {N} K {K} r {r}: share of elements off bf16(fp64) {share:.2e}")
    assert ((bits - rbits).abs() <= 1).all()                                # same sign near zero is implied: |W| >> 0 where they differ
    assert share <= 1e-3


# ---------------------------------------------------------------------------------------------------- model
TARGETS = ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out", "proj_mlp",
           "ff.net.0.proj")
B_, HG, WG, L_ = 2, 8, 12, 40


@pytest.fixture(scope="module")
def pair():
    """One model pair and one set of inputs for the model tests (the oracle's parameters are never modified)."""
    ocfg, P, m = build_pair(small_cfg(2, 2))
    return ocfg, P, m, make_inputs(B_, HG, WG, L_, seed=3)


def _cuda(inputs):
    x, ehs, pooled, ids, tids, t, gd = inputs
    return x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda()


def _randomise(lo, seed, std=0.05):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo.w32.normal_(0.0, std, generator=g)
    lo.sync_bf16()


def test_fresh_adapters_change_no_output_bit_and_unload_restores(pair):
    ocfg, P, m, inputs = pair
    m.unload_lora()
    args = _cuda(inputs)
    w16 = m.store.w16.clone()
    m.eval()
    with torch.no_grad():
        ref_ng = m._forward_nograd(*args).clone()
    m.train()
    ref_tr = m(*args)[0].detach().clone()
    m.add_lora(rank=16, alpha=32, target_modules=TARGETS)
    assert m.lora_param.requires_grad and not m.flat_param.requires_grad
    assert torch.equal(m.store.w16, w16)                                    # B = 0: bf16(W0 + 0)
    with torch.no_grad():
        assert torch.equal(m._forward_nograd(*args), ref_ng)
    out = m(*args)[0]
    assert out.requires_grad and torch.equal(out.detach(), ref_tr)
    _randomise(m.lora, 1)
    m.merge_lora()
    assert not torch.equal(m.store.w16, w16)
    m.unload_lora()
    assert torch.equal(m.store.w16, w16) and m.lora is None and m.flat_param.requires_grad


def test_adapter_gradients_vs_oracle_autograd(pair):
    """d(sum(out * R)) / d(A, B) through the low-rank backward vs torch autograd of the oracle with parameters W0 + s B A.
    Tolerances of test_hip_mmdit.py::test_backward_vs_oracle_autograd: global cosine > 0.999, worst tensor rel-L2 < 4e-2."""
    from mixgrpo_amd.optim import FusedAdamW
    ocfg, P, m, inputs = pair
    m.unload_lora()
    m.store.g32 = None
    m.add_lora(rank=16, alpha=32, target_modules=TARGETS)
    lo = m.lora
    _randomise(lo, 2)
    m.merge_lora()
    x, ehs, pooled, ids, tids, t, gd = inputs
    R = torch.randn(B_, HG * WG, 64, generator=torch.Generator().manual_seed(9))
    leaves, Pm = {}, dict(P)
    for module, N, K in lo.targets:
        A = lo.view(lo.w32, f"{module}.lora_A").cpu().clone().requires_grad_(True)
        Bm = lo.view(lo.w32, f"{module}.lora_Bt").cpu().t().clone().requires_grad_(True)
        leaves[module] = (A, Bm)
        Pm[f"{module}.weight"] = P[f"{module}.weight"] + lo.scale * (Bm @ A)
    ref = OM.forward(Pm, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids)
    (ref * R).sum().backward()
    m.train()
    out = m(*_cuda(inputs))[0]
    (out.float() * R.cuda()).sum().backward()
    g = lo.g32
    assert m.lora_param.grad is g

    def compare(factor):
        dots = nh = no = 0.0
        worst = []
        for module, (A, Bm) in leaves.items():
            for gh, go, key in ((lo.view(g, f"{module}.lora_A").cpu(), factor * A.grad, "A"),
                                (lo.view(g, f"{module}.lora_Bt").cpu().t(), factor * Bm.grad, "B")):
                dots += (gh * go).sum().item()
                nh += gh.pow(2).sum().item()
                no += go.pow(2).sum().item()
                worst.append((((gh - go).norm() / (go.norm() + 1e-9)).item(), f"{module}.{key}"))
        worst.sort(reverse=True)
        cos = dots / math.sqrt(nh * no)
        print(f"x{factor}: cosine {cos:.6f} worst {worst[:3]}")
        assert cos > 0.999, (cos, worst[:5])
        assert worst[0][0] < 4e-2, worst[:8]

    compare(1.0)
    out = m(*_cuda(inputs))[0]                                              # a second backward accumulates
    (out.float() * R.cuda()).sum().backward()
    compare(2.0)
    assert m.store.g32 is None and m.flat_param.grad is None               # the base's gradient buffer is never allocated
    opt = FusedAdamW(m, lr=1e-3)
    assert opt.m.numel() == lo.numel and opt.store is lo


def test_adamw_step_merge_and_adapter_files(pair, tmp_path):
    from mixgrpo_amd.checkpoint import save_lora_checkpoint
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.optim import FusedAdamW
    ocfg, P, m, inputs = pair
    m.unload_lora()
    m.add_lora(rank=16, alpha=32, target_modules=TARGETS)
    lo = m.lora
    _randomise(lo, 5)
    m.merge_lora()
    lr, wd = 1e-3, 1e-2
    opt = FusedAdamW(m, lr=lr, weight_decay=wd)
    gen = torch.Generator(device="cuda").manual_seed(6)
    lo.ensure_grad().normal_(0.0, 1e-3, generator=gen)
    ref_p = torch.nn.Parameter(lo.w32.clone())
    ref_p.grad = lo.g32.clone()
    ref = torch.optim.AdamW([ref_p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref.step()
    w32_base = m.store.w32.clone()
    opt.step()
    m.merge_lora()
    assert _rel(lo.w32, ref_p.data) < 1e-6 and (lo.w32 - ref_p.data).abs().max().item() < 1e-7   # tests/test_hip_optim.py
    assert torch.equal(lo.w16, lo.w32.to(BF16))
    assert torch.equal(m.store.w32, w32_base)                               # the base never moves
    name = "transformer_blocks.1.attn.to_q"
    got = m.store.view(m.store.w16, name + ".weight").clone()
    m.merge_lora()
    assert torch.equal(got, m.store.view(m.store.w16, name + ".weight"))
    want = (m.store.view(m.store.w32, name + ".weight").double() + lo.scale *
            (lo.view(lo.w32, name + ".lora_Bt").double().t() @ lo.view(lo.w32, name + ".lora_A").double())).to(BF16)
    assert (got.view(torch.int16).to(torch.int32) - want.view(torch.int16).to(torch.int32)).abs().max().item() <= 1
    # save -> load into a second model -> same outputs
    d = save_lora_checkpoint(m, 0, str(tmp_path), 7, 0)
    assert os.path.basename(d) == "lora-checkpoint-7-0"
    assert sorted(os.listdir(d)) == ["lora_config.json", "pytorch_lora_weights.safetensors"]
    m2 = FluxTransformer2DModel(FluxConfig(**small_cfg(2, 2)), device="cuda")
    m2.load_state_dict({k: v.cuda() for k, v in P.items()})
    m2.load_lora(d)
    assert m2.lora.rank == 16 and m2.lora.alpha == 32.0 and m2.lora.target_modules == TARGETS
    args = _cuda(inputs)
    m.eval(), m2.eval()
    with torch.no_grad():
        assert torch.equal(m(*args)[0], m2(*args)[0])
    m.unload_lora()


def _lora_train_step(seed_prompts, G, accum, lr=1e-3, overlap=False):
    """One train step of a 1 + 1 block model with adapters on the prompts `seed_prompts` (one group of G each)."""
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.optim import ConstantWithWarmup, FusedAdamW
    dev = torch.device("cuda", 0)
    m = FluxTransformer2DModel(FluxConfig(**small_cfg(1, 1)), device=dev).init_synthetic(seed=5, std=0.05, bias_std=0.02)
    pargs = TG.build_parser().parse_args(["--data_json_path", "x", "--use_lora", "--lora_rank", "16", "--lora_alpha", "32",
                                          "--lora_target_modules", "to_q,to_k,to_v,to_out.0,proj_mlp"])
    assert pargs.use_lora
    m.add_lora(pargs.lora_rank, pargs.lora_alpha, pargs.lora_target_modules, seed=1)
    _randomise(m.lora, 8, std=0.02)
    m.merge_lora()
    m.dp_grad_dtype, m.dp_overlap = "fp32", overlap
    opt = FusedAdamW(m, lr=lr)
    args = TG.default_args(h=48, w=64, sampling_steps=8, num_generations=G, gradient_accumulation_steps=accum,
                           share_rollout_prefix=False)
    embeds, pooled, steps = [], [], []
    for s in seed_prompts:
        g = torch.Generator().manual_seed(s)
        embeds.append((0.1 * torch.randn(1, 16, 64, generator=g)).bfloat16())
        pooled.append(torch.randn(1, 32, generator=g).bfloat16())
        steps.append([torch.randn(G, 12, 64, generator=g).bfloat16() for _ in range(8)])
    n = len(seed_prompts)
    batch = (torch.cat(embeds).to(dev), torch.cat(pooled).to(dev), torch.zeros(n, 3, device=dev), ["p"] * n)
    args.injected_noise = {"x_T": torch.randn(1, 16, 6, 8, generator=torch.Generator().manual_seed(77)).bfloat16(),
                           "steps": [torch.cat([st[i] for st in steps]) for i in range(8)]}
    base = torch.tensor([0.1, 0.4, 0.2, 0.9, 0.3, 0.6][:G])

    def reward(lat, cap):
        r = torch.cat([base + 0.05 * s * torch.arange(G) for s in seed_prompts])
        return r, {"Synthetic": r}

    w32_base = m.store.w32.clone()
    res = TG.train_one_step(args, dev, m, None, reward, opt, ConstantWithWarmup(opt, 0), iter([batch]), None, 1.0, [1, 2], 0,
                            {"Synthetic": 1.0})
    torch.cuda.synchronize()
    assert torch.equal(m.store.w32, w32_base) and m.store.g32 is None
    return res, m


def test_train_one_step_with_adapters():
    """One optimizer step (a single chunk: G = accumulation steps = 4): finite loss and gradient norm, and the replay of the
    rollout policy reproduces its log-probs -- the logged KL term < 1e-8, the bound of tests/test_hip_config0.py."""
    res, m = _lora_train_step([1], G=4, accum=4)
    print("train step:", res)
    assert all(math.isfinite(v) for v in res[:5])
    assert res[1] > 0
    assert 0.0 <= res[3] < 1e-8
    lo = m.lora
    name = "transformer_blocks.0.attn.to_q"
    got = m.store.view(m.store.w16, name + ".weight").clone()
    m.merge_lora()
    assert torch.equal(got, m.store.view(m.store.w16, name + ".weight"))   # the step left the compute copy merged


def _dp_worker(rank, world, port, q, seeds_by_rank, accum, overlap=False):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res, m = _lora_train_step(seeds_by_rank[rank], G=2, accum=accum, overlap=overlap)
    w = m.lora.w32.detach().cpu()
    red = m._mgx_grad_reducer if world > 1 else None
    assert red is None or (red.flat.numel() == m.lora.numel and red.overlap == overlap and not red.pending and not red.launched)
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, res[1], w.tolist()))


_one_rank = {}


@pytest.mark.parametrize("overlap", [False, True])
def test_two_ranks_step_the_adapters_in_lockstep(overlap):
    """Two ranks on one GPU (gloo; one group of 2 each, one optimizer step), the adapter gradient reduced after the backward
    or block by block during it: identical adapters on both ranks, and equal to one rank stepping on the concatenated batch
    (accumulation 4) within the tolerances tests/test_hip_dp.py puts on two ways of summing the same gradient: first AdamW
    steps are sign-like, so <= 4 lr per weight and < 0.02 lr on average."""
    lr = 1e-3
    two = run_ranks(_dp_worker, 2, timeout=300, extra=(([1], [2]), 2, overlap))
    if not _one_rank:
        _one_rank["out"] = run_ranks(_dp_worker, 1, timeout=300, extra=(([1, 2],), 4))
    one = _one_rank["out"]
    w0, w1, w = torch.tensor(two[0][2]), torch.tensor(two[1][2]), torch.tensor(one[0][2])
    assert torch.equal(w0, w1)
    assert two[0][1] == two[1][1] and two[0][1] > 0
    print(f"overlap {overlap}: grad norm 2 ranks {two[0][1]:.6e} 1 rank {one[0][1]:.6e}; max |dw| {(w0 - w).abs().max().item():.3e} "
          f"mean {(w0 - w).abs().mean().item():.3e}")
    assert two[0][1] == pytest.approx(one[0][1], rel=1e-2)
    assert (w0 - w).abs().max().item() <= 4.0 * lr
    assert (w0 - w).abs().mean().item() < 0.02 * lr


def test_optimizer_built_before_the_adapters_is_refused():
    from mixgrpo_amd import train_grpo_flux as TG
    from mixgrpo_amd._lib import MgxError
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    from mixgrpo_amd.optim import FusedAdamW
    m = FluxTransformer2DModel(FluxConfig(**small_cfg(1, 1)), device="cuda").init_synthetic(seed=5, std=0.05)
    opt = FusedAdamW(m, lr=1e-3)
    m.add_lora(rank=16)
    with pytest.raises(MgxError, match="another store"):
        TG._fused_step(m, opt, 1.0)
    assert m.store.g32 is None
