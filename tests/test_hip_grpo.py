"""Direct tests of csrc/grpo.hip -- mgx_group_advantage, mgx_global_advantage, mgx_grpo_loss -- called through `_lib.lib()` the
way train_grpo_flux.py calls them, against plain torch fp64 restatements of the reference's formulas
(fastvideo/train_grpo_flux.py:440-501 advantages, :560-583 loss) on the same fp32 inputs.

The GPU tests carry `@gpu`; the module has no `pytestmark`, because the premises the bounds rest on are checked in this same
file on the CPU (`test_cpu_*`): a serial-fp32 numpy / fp32 torch evaluation of each formula stays inside the bound, and the
bound is at least 100 times smaller than what one trimmed element more or fewer does to a group.

ADVANTAGE BOUND.  u = 2^-24.  The kernel adds serially in fp32, so a sum of n terms is off by at most (n-1) u sum|x|:
  mean:  |mean32 - mean| <= n u mean|x|                       (n-1 adds + the division), i.e. n u mean|r| / std in the advantage;
  std:   q = sum d^2 has relative error <= (n+2) u            (n-1 adds, d's rounding twice, the square; the shift of every d
         by the mean's error moves q only in second order, since sum d = 0 -- given std >> n u mean|r|, which every group
         here meets except the all-equal ones, whose sums are exact: see TIE_VALUES), the square root halves it and adds u,
         the division by n-1 and the + 1e-8 add u each: (n/2 + 4) u, which multiplies |adv|;
  adv:   the subtraction and the division add 2 u |adv|.
Together |adv - ref| <= n u mean|r|/std + (n/2 + 6) u |ref| <= 2 G u (mean|r|/std + |ref|) + 4 u |ref| with n <= G: the
issue's bound, a factor of two above the worst case.  mean|r| and std are those of the elements the statistics run over.
With `weight` and `accumulate` the kernel rounds a*w and the sum once each: |w| bound + 2 u (|w ref| + |out0|).
CPU-measured (test_cpu_serial_fp32_stays_inside_the_advantage_bound): the serial-fp32 evaluation uses at most 0.147 of the
bound over every case below; (test_cpu_one_trimmed_element_dwarfs_the_advantage_bound): the smallest shift of an advantage by
one trimmed element more or fewer is 1725 bounds.

LOSS BOUND, in fp32 ulps (2^-23 of a term's magnitude; |diff| <= 2 in every case):
  ratio:   diff = new - old is rounded (u |diff| <= 1 ulp of ratio after exp), expf is documented at 1 ulp: 2 ulps;
  policy:  -a * ratio (or * the clamp bound, 1 -+ c formed in fp32: 1 ulp) and / denom, half an ulp each: 3, held to 4 ulps;
  kl:      diff^2 carries diff's rounding twice (1 ulp), the product and the division half an ulp each: 2, held to 3 ulps;
  loss:    policy + kl_coeff * kl: 4 ulps of |policy| + 4 of kl_coeff kl + half an ulp of the sum <= 10 ulps of the larger term;
  g_logp:  (1/denom * w) * (-a) * ratio is 1/denom, two products and ratio: 3.5 ulps; (kl_coeff/denom * 0.5) * (2 diff) is
           2 ulps; the sum adds half an ulp: <= 10 ulps of the larger of |policy gradient| and kl_coeff |diff| / denom.
clip_frac is exact: no case puts |ratio - 1| within 10 % of clip_range (asserted on the CPU).
CPU-measured (test_cpu_fp32_torch_stays_inside_the_loss_bound): fp32 torch uses at most 0.19 / 0.29 / 0.11 / 0.11 of the
policy / kl / loss / g_logp bounds."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ULP = 2.0 ** -23

GROUP_SIZES = (1, 2, 3, 63, 64, 65, 100, 1000, 1024)      # one lane, the 64-thread stride edge, the LDS array's limit
# Tied rewards: 5 values, the upper ones rarer so that the top 16 % of a group (ratio 0.84) still holds two of them.  They are
# multiples of 1/8: a group that draws one value only (G = 2, 3) then sums exactly, its mean is that value and its advantages
# are exactly 0 on both sides.  (With an inexact mean such a group's std is rounding noise over 1e-8 -- in the reference's fp32
# too -- and no bound holds; the derivation below needs std >> G u mean|r|.)
TIE_VALUES, TIE_PROBS = (-1.5, -0.25, 0.125, 0.75, 2.0), (0.3, 0.3, 0.2, 0.1, 0.1)
# (G, trimmed_ratio): the four pairs at which a float product gives another count than the reference's double one, the
# trainer test's pair, ratios >= 1 (clamped to G - 1: one element, std NaN like torch.std) and ratios whose count is 0
TRIM_CASES = ((50, 0.58), (75, 0.84), (100, 0.29), (100, 0.59), (6, 0.25), (5, 1.0), (64, 1.5), (65, 0.01), (3, 0.3))
REFERENCE_TRIM = {(50, 0.58): 28, (75, 0.84): 63, (100, 0.29): 28, (100, 0.59): 59, (6, 0.25): 1, (5, 1.0): 4, (64, 1.5): 63,
                  (65, 0.01): 0, (3, 0.3): 0}
# the rank sort at the stride edge and at the LDS limit; G this large is not a statement about +-1 element (see the premise)
SORT_CASES = ((63, 0.3), (1000, 0.37), (1024, 0.5))
VARIANTS = ((0, 1.0), (0, 0.5), (1, 1.0), (1, 0.5), (1, -2.0))   # (accumulate, weight)
NAN_BITS = 0x7FC12345                                            # the pre-fill of accumulate = 0 outputs: a NaN with a payload


def trim_count(G, ratio):
    from mixgrpo_amd import train_grpo_flux as TG
    return TG.trim_count(G, ratio)


def rewards(G, kind, seed=0):
    """3 groups of G and a ragged tail of G - 1, on the host (the same numbers on every machine)."""
    n = 3 * G + G - 1
    g = torch.Generator().manual_seed(1000 * seed + G)
    if kind == "normal":
        return torch.randn(n, generator=g)
    if kind == "ties":
        return torch.tensor(TIE_VALUES)[torch.multinomial(torch.tensor(TIE_PROBS), n, replacement=True, generator=g)]
    assert kind == "const"
    r = torch.randn(n, generator=g)
    r[G:2 * G] = 0.5                                            # the middle group is constant: std 1e-8, advantages exactly 0
    return r


def ref_stats(stat):
    """fp64 mean, unbiased std + 1e-8 (0 / 0 = NaN for one element, like torch.std) and mean|x| / std of [rows, cnt]."""
    cnt = stat.shape[1]
    mean = stat.mean(1, keepdim=True)
    std = (((stat - mean) ** 2).sum(1, keepdim=True) / (cnt - 1)).sqrt() + 1e-8
    return mean, std, stat.abs().mean(1, keepdim=True) / std


def ref_group(r, G, trim):
    """The reference's lines 447-461 / 474-489 in fp64 on the fp32 rewards: advantages of the whole groups, and the bound."""
    g = r.double()[:r.numel() // G * G].view(-1, G)
    stat = torch.sort(g, dim=1)[0][:, trim:] if trim >= 0 else g
    mean, std, scale = ref_stats(stat)
    adv = (g - mean) / std
    bound = 2 * G * U * (scale + adv.abs()) + 4 * U * adv.abs()
    return adv.reshape(-1), bound.reshape(-1)


def ref_global(r, gathered):
    mean, std, scale = ref_stats(gathered.double()[None])
    adv = ((r.double() - mean) / std)[0]
    return adv, 2 * gathered.numel() * U * (scale[0] + adv.abs()) + 4 * U * adv.abs()


def _serial32(src, x):
    """(x - mean) / (std + 1e-8) with the statistics of `src` added serially in fp32, in the kernel's order."""
    with np.errstate(all="ignore"):
        n = np.float32(len(src))
        mean = np.float32(np.cumsum(src, dtype=np.float32)[-1] / n)
        d = (src - mean).astype(np.float32)
        q = np.cumsum((d * d).astype(np.float32), dtype=np.float32)[-1]
        std = np.float32(np.sqrt(np.float32(q / (n - np.float32(1)))) + np.float32(1e-8))
        return ((x - mean).astype(np.float32) / std).astype(np.float32)


def serial32_group(r, G, trim):
    r = r.numpy().astype(np.float32)
    out = []
    for b in range(len(r) // G):
        g = r[b * G:(b + 1) * G]
        out.append(_serial32(np.sort(g, kind="stable")[trim:] if trim >= 0 else g, g))
    return torch.from_numpy(np.concatenate(out))


def assert_within(out, ref, tol, what):
    out = out.detach().double().cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out), nan), (what, "NaN pattern")
    err, tol = (out - ref).abs()[~nan], tol[~nan]
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), (err / tol.clamp_min(1e-300)).max().item(), err.max().item())


def group_cases():
    for G in GROUP_SIZES:
        for kind in ("normal", "ties"):
            yield G, 0.0, kind
    yield 64, 0.0, "const"
    yield 65, 0.4, "const"
    for G, ratio in TRIM_CASES + SORT_CASES:
        for kind in ("normal", "ties"):
            yield G, ratio, kind


# ------------------------------------------------------------------------------------------------ CPU premises

def test_cpu_trim_count_is_the_reference_double_product():
    """train_grpo_flux.trim_count == min(int(G * ratio), G - 1) in Python double for every G in 2..1024 and ratio k/100,
    among them the 107 pairs at which the former kernel-side `(int)((float)G * ratio)` gave another count."""
    mismatching = []
    for G in range(2, 1025):
        for k in range(1, 100):
            ratio = k / 100
            want = min(int(G * ratio), G - 1)
            assert trim_count(G, ratio) == want, (G, ratio)
            was = min(int(np.float32(G) * np.float32(ratio)), G - 1)
            if was != want:
                mismatching.append((G, ratio, want, was))
    assert len(mismatching) == 107
    for case in ((50, 0.58, 28, 29), (75, 0.84, 63, 62), (100, 0.29, 28, 29), (100, 0.59, 59, 58)):
        assert case in mismatching
    for (G, ratio), want in REFERENCE_TRIM.items():
        assert trim_count(G, ratio) == want
    assert trim_count(8, 0.0) == -1 and trim_count(8, -0.5) == -1 and trim_count(8, float("nan")) == -1
    assert trim_count(1, 0.5) == 0 and trim_count(1024, 7.0) == 1023


def test_cpu_serial_fp32_stays_inside_the_advantage_bound():
    worst = 0.0
    for G, ratio, kind in group_cases():
        r = rewards(G, kind)
        trim = trim_count(G, ratio)
        ref, bound = ref_group(r, G, trim)
        got = serial32_group(r, G, trim)
        assert_within(got, ref, bound, (G, ratio, kind))
        ok = ~torch.isnan(ref)
        if ok.any():
            worst = max(worst, ((got.double() - ref).abs()[ok] / bound[ok]).max().item())
        if kind == "const":
            assert torch.equal(got[G:2 * G], torch.zeros(G)) and torch.equal(ref[G:2 * G], torch.zeros(G, dtype=F64))
    for n_all in (2, 5, 64, 1000):
        buf = torch.randn(n_all + 8, generator=torch.Generator().manual_seed(n_all))
        ref, bound = ref_global(buf[3:8], buf[:n_all])
        got = torch.from_numpy(_serial32(buf[:n_all].numpy(), buf[3:8].numpy()))
        assert_within(got, ref, bound, n_all)
        worst = max(worst, ((got.double() - ref).abs() / bound).max().item())
    print(f"serial fp32 / bound: {worst:.3f}")
    assert 0 < worst < 0.5


def test_cpu_one_trimmed_element_dwarfs_the_advantage_bound():
    """In every trimmed case with finite advantages, trimming one element more or fewer moves some advantage by >= 100 bounds:
    a kernel with the wrong count cannot pass.  (A ratio >= 1 leaves one element: there the NaN pattern is the witness.)"""
    smallest = float("inf")
    for G, ratio in TRIM_CASES:
        trim = REFERENCE_TRIM[(G, ratio)]
        if trim == G - 1:
            continue
        for kind in ("normal", "ties"):
            r = rewards(G, kind)
            ref, bound = ref_group(r, G, trim)
            for other in (trim - 1, trim + 1):
                if 0 <= other < G - 1:
                    shift = (ref_group(r, G, other)[0] - ref).abs()
                    ratio_ = (shift / bound).max().item()
                    smallest = min(smallest, ratio_)
                    assert ratio_ >= 100, (G, ratio, kind, other, ratio_)
    print(f"smallest trim shift / bound: {smallest:.0f}")


# ------------------------------------------------------------------------------------------------ loss: inputs, reference

LOSS_B = (1, 63, 64, 65, 200)
LOSS_SETTINGS = [(c, kc, denom) for c in (1e-4, 0.2) for kc in (0.0, 0.01) for denom in (1.0, 6.0)]
ADV_CLIP_MAX = 5.0


def loss_inputs(B, c):
    """Row b takes combination (b + B) % 63 of the full cross diff x advantage: +-{0, c/2, 2c, 0.3, 2.0} x {0, +-0.5, +-3, +-7}.
    old_logp runs over multiples of 1/64 in [-4, 4), so new = old + diff keeps diff to 5e-7."""
    diffs = [0.0] + [s * x for x in (c / 2, 2 * c, 0.3, 2.0) for s in (1.0, -1.0)]
    advs = [0.0, 0.5, -0.5, 3.0, -3.0, 7.0, -7.0]
    combos = torch.tensor([(d, a) for d in diffs for a in advs], dtype=F64)
    pick = combos[(torch.arange(B) + B) % len(combos)]
    old = ((torch.arange(B) * 37 % 512) - 256).double() / 64
    return (old + pick[:, 0]).float(), old.float(), pick[:, 1].float()


def ref_loss(new, old, adv, c, kc, denom, dtype=F64):
    """Lines 560-583 with one row per loss (the means run over one element), autograd for d loss / d new_logp.  Returns
    (loss, policy, kl, clip_frac, g_logp) and, for fp64, their tolerances (None for clip_frac: exact)."""
    new = new.to(dtype).requires_grad_(True)
    old, adv = old.to(dtype), adv.to(dtype)
    a = torch.clamp(adv, -ADV_CLIP_MAX, ADV_CLIP_MAX)
    diff = new - old
    ratio = torch.exp(diff)
    unclipped = -a * ratio
    clipped = -a * torch.clamp(ratio, 1.0 - c, 1.0 + c)
    clip_frac = ((ratio - 1.0).abs() > c).to(dtype)
    policy = torch.maximum(unclipped, clipped) / denom
    kl = 0.5 * diff ** 2 / denom
    loss = policy + kc * kl
    loss.sum().backward()
    g = new.grad
    outs = tuple(t.detach() for t in (loss, policy, kl, clip_frac, g))
    if dtype != F64:
        return outs
    with torch.no_grad():
        kl_term, kl_grad = kc * kl, kc * diff / denom
        tols = (10 * ULP * torch.maximum(policy.abs(), kl_term), 4 * ULP * policy.abs(), 3 * ULP * kl, None,
                10 * ULP * torch.maximum((g - kl_grad).abs(), kl_grad.abs()))
    return outs, tols


NAMES = ("loss", "policy", "kl", "clip_frac", "g_logp")


def assert_loss_outputs(outs, refs, tols, what):
    for name, out, ref, tol in zip(NAMES, outs, refs, tols):
        if tol is None:
            assert torch.equal(out.detach().double().cpu(), ref), (what, name)
        else:
            assert_within(out, ref, tol, (what, name))


def test_cpu_fp32_torch_stays_inside_the_loss_bound():
    worst = dict.fromkeys(NAMES, 0.0)
    seen = set()
    for B in LOSS_B:
        for c, kc, denom in LOSS_SETTINGS:
            new, old, adv = loss_inputs(B, c)
            r = torch.exp(new.double() - old.double())
            assert not (((r - 1).abs() > 0.9 * c) & ((r - 1).abs() < 1.1 * c)).any()      # clip_frac cannot flip in fp32
            refs, tols = ref_loss(new, old, adv, c, kc, denom)
            outs = ref_loss(new, old, adv, c, kc, denom, dtype=F32)
            assert_loss_outputs(outs, refs, tols, (B, c, kc, denom))
            for name, out, ref, tol in zip(NAMES, outs, refs, tols):
                if tol is not None and (tol > 0).any():
                    worst[name] = max(worst[name], ((out.double() - ref).abs()[tol > 0] / tol[tol > 0]).max().item())
            # every branch is crossed: the ratio inside / above / below the range for each sign of the advantage, the ties
            a, inside = adv.clamp(-5, 5), (r - 1).abs() <= c
            seen |= {((x > 0) - (x < 0), "in" if i else ("hi" if y > 1 else "lo"), y == 1)
                     for x, y, i in zip(a.tolist(), r.tolist(), inside.tolist())}
    assert len(seen) == 3 * 3 + 3, sorted(seen)
    print("fp32 torch / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v < 1 for v in worst.values())


# ------------------------------------------------------------------------------------------------ GPU: group advantage

def _launch_group(r, out, G, ratio, weight, accumulate):
    """As train_grpo_flux.compute_advantages calls it: the count is formed on the host."""
    from mixgrpo_amd import _lib as L
    return L.lib().mgx_group_advantage(L.ptr(r), L.ptr(out), r.numel(), G, trim_count(G, ratio), weight, accumulate, L.stream())


def _check_group(G, ratio, kind):
    r = rewards(G, kind)
    trim = trim_count(G, ratio)
    ref, bound = ref_group(r, G, trim)
    nfull = ref.numel()
    rd = r.cuda()
    for accumulate, weight in VARIANTS:
        if accumulate:
            out0 = torch.randn(r.numel(), generator=torch.Generator().manual_seed(7)) + 3.0
            base = out0.double()[:nfull]
        else:
            out0 = torch.full((r.numel(),), NAN_BITS, dtype=torch.int32).view(F32)
            base = torch.zeros(nfull, dtype=F64)
        out = out0.cuda()
        assert _launch_group(rd, out, G, ratio, weight, accumulate) == 0
        out = out.cpu()
        assert torch.equal(out.view(torch.int32)[nfull:], out0.view(torch.int32)[nfull:]), "the ragged tail was written"
        assert_within(out[:nfull], base + ref * weight, abs(weight) * bound + 2 * U * ((ref * weight).abs() + base.abs()),
                      (G, ratio, kind, accumulate, weight))
        if kind == "const" and not accumulate:
            assert torch.equal(out[G:2 * G], torch.zeros(G) * weight)


@gpu
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_group_advantage_untrimmed(G):
    """Every group size class, random and tied rewards, overwrite onto NaN and accumulate with weights onto a non-zero output;
    G = 1 is NaN on both sides (unbiased std of one element)."""
    for kind in ("normal", "ties"):
        _check_group(G, 0.0, kind)
    if G == 1:
        out = torch.zeros(3).cuda()
        assert _launch_group(rewards(1, "normal").cuda(), out, 1, 0.0, 1.0, 0) == 0
        assert torch.isnan(out).all()


@gpu
@pytest.mark.parametrize("G,ratio", TRIM_CASES + SORT_CASES, ids=lambda v: str(v))
def test_group_advantage_trimmed(G, ratio):
    """The statistics run over the sorted group without its min(int(G * ratio), G - 1) smallest rewards, the count taken in
    double like the reference; tied rewards must all be placed by the rank sort."""
    for kind in ("normal", "ties"):
        _check_group(G, ratio, kind)
    if REFERENCE_TRIM.get((G, ratio)) == G - 1:
        out = torch.zeros(4 * G - 1).cuda()
        assert _launch_group(rewards(G, "normal").cuda(), out, G, ratio, 1.0, 0) == 0
        assert torch.isnan(out[:3 * G]).all() and not torch.isnan(out[3 * G:]).any()


@gpu
def test_group_advantage_constant_group_is_exactly_zero():
    _check_group(64, 0.0, "const")
    _check_group(65, 0.4, "const")


@gpu
def test_group_advantage_refuses_bad_group_sizes():
    """G = 0, G = 1025 (the LDS array holds 1024) and a trim count that leaves no reward: an error, nothing written."""
    from mixgrpo_amd import _lib as L
    r = torch.randn(4100).cuda()
    out0 = torch.full((4100,), NAN_BITS, dtype=torch.int32)
    out = out0.view(F32).cuda()
    for G, trim in ((0, -1), (1025, -1), (1025, 3), (8, 8), (1, 1)):
        rc = L.lib().mgx_group_advantage(L.ptr(r), L.ptr(out), r.numel(), G, trim, 1.0, 0, L.stream())
        assert rc != 0, (G, trim)
        with pytest.raises(L.MgxError):
            L.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), out0)


# ------------------------------------------------------------------------------------------------ GPU: global advantage

@gpu
@pytest.mark.parametrize("n_all", (2, 5, 64, 1000))
def test_global_advantage(n_all):
    """use_group=False: the local rewards normalised by the gathered ones' statistics; `rewards` is a slice at offset 3 of the
    buffer `gathered` starts, the output is over-allocated."""
    from mixgrpo_amd import _lib as L
    for n in (1, 64, 65, 300):
        buf = torch.randn(max(n_all, n + 3), generator=torch.Generator().manual_seed(n_all * 1000 + n))
        bd = buf.cuda()
        r, ga = bd[3:3 + n], bd[:n_all]
        out0 = torch.full((n + 8,), NAN_BITS, dtype=torch.int32)
        out = out0.view(F32).cuda()
        assert L.lib().mgx_global_advantage(L.ptr(r), L.ptr(ga), L.ptr(out), n, n_all, L.stream()) == 0
        ref, bound = ref_global(buf[3:3 + n], buf[:n_all])
        out = out.cpu()
        assert_within(out[:n], ref, bound, (n_all, n))
        assert torch.equal(out.view(torch.int32)[n:], out0[n:])


@gpu
def test_global_advantage_of_one_gathered_reward_is_nan():
    from mixgrpo_amd import _lib as L
    bd = torch.randn(8).cuda()
    out = torch.zeros(5).cuda()
    assert L.lib().mgx_global_advantage(L.ptr(bd[1:6]), L.ptr(bd[:1]), L.ptr(out), 5, 1, L.stream()) == 0
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ GPU: loss

def _launch_loss(new, old, adv, B, c, kc, denom):
    """Five over-allocated rows (loss, policy, kl, clip_frac, g_logp) as train_grpo_flux passes them; 8 sentinel columns."""
    from mixgrpo_amd import _lib as L
    out0 = torch.full((5, B + 8), NAN_BITS, dtype=torch.int32)
    out = out0.view(F32).cuda()
    L.check(L.lib().mgx_grpo_loss(L.ptr(new), L.ptr(old), L.ptr(adv), B, c, ADV_CLIP_MAX, kc, denom, out[0].data_ptr(),
                                  out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), L.stream()))
    out = out.cpu()
    assert torch.equal(out.view(torch.int32)[:, B:], out0[:, B:]), "rows >= B were written"
    return out[:, :B]


@gpu
@pytest.mark.parametrize("B", LOSS_B)
def test_grpo_loss_every_branch(B):
    """One block, the block edge, a second block with one row, several blocks; every combination of ratio inside / above /
    below the clip range, advantage sign, the 0.5 / 0.5 ties at advantage 0 and diff 0, and the advantage clamp."""
    for c, kc, denom in LOSS_SETTINGS:
        new, old, adv = loss_inputs(B, c)
        refs, tols = ref_loss(new, old, adv, c, kc, denom)
        outs = _launch_loss(new.cuda(), old.cuda(), adv.cuda(), B, c, kc, denom)
        assert_loss_outputs(outs, refs, tols, (B, c, kc, denom))


@gpu
@pytest.mark.parametrize("which", ("new_logp", "old_logp", "advantage"))
def test_grpo_loss_nan_stays_in_its_row(which):
    """A NaN the reference produces must not become a number, nor reach a neighbour: rows 3, 63 and 64 (both sides of the
    block edge) take a NaN in one input; their loss and gradient are NaN, every other row is bit-identical to the clean run."""
    B, (c, kc, denom) = 65, (0.2, 0.01, 6.0)
    ins = list(loss_inputs(B, c))
    clean = _launch_loss(*(t.cuda() for t in ins), B, c, kc, denom)
    rows = torch.tensor([3, 63, 64])
    ins[("new_logp", "old_logp", "advantage").index(which)][rows] = float("nan")
    outs = _launch_loss(*(t.cuda() for t in ins), B, c, kc, denom)
    refs, _ = ref_loss(*ins, c, kc, denom)
    keep = torch.ones(B, dtype=torch.bool)
    keep[rows] = False
    for name, out, ref, was in zip(NAMES, outs, refs, clean):
        assert torch.equal(out[keep].view(torch.int32), was[keep].view(torch.int32)), name
        assert torch.equal(torch.isnan(out), torch.isnan(ref)), name
    assert torch.isnan(outs[0][rows]).all() and torch.isnan(outs[1][rows]).all() and torch.isnan(outs[4][rows]).all()
