"""Direct parity of the fused optimizer kernels (csrc/optim.hip: mgx_sqnorm_f32, mgx_adamw_step) with what the reference
runs per optimizer step -- `transformer.clip_grad_norm_(max_grad_norm)` then `torch.optim.AdamW.step()`
(fastvideo/train_grpo_flux.py:606-607, optimizer built at :715-721: betas (0.9, 0.999), eps 1e-8, weight decay) -- over
several steps on a random ~1 M-element buffer: clip active and inactive, the data-parallel `grad_scale` 1 and 1/8, weight
decay on.  Masters and moments <= 1e-6 relative (fp32 both sides, different operation order), the bf16 compute mirror
exactly bf16(master)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("max_norm,grad_scale,gstd", [(1.0, 1.0, 1e-2),      # |g| ~ 10: clip active (coef ~ 0.1)
                                                       (1.0, 0.125, 1e-5),    # |g/8| << 1: clip inactive, DP scale 1/8
                                                       (0.05, 0.125, 1e-3),   # both: scale then clip
                                                       (None, 1.0, 1e-3)])    # no clipping at all
def test_adamw_and_sqnorm_vs_torch(max_norm, grad_scale, gstd):
    from mixgrpo_amd import ops
    n = 1 << 20
    lr, b1, b2, eps, wd = 2e-4, 0.9, 0.999, 1e-8, 1e-2
    g0 = torch.Generator(device="cuda").manual_seed(5)
    w = torch.randn(n, device="cuda", generator=g0) * 0.02
    ref_p = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    w16 = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    nsq = torch.zeros(1, device="cuda")
    for step in range(1, 4):                                   # bias corrections at steps 1, 2, 3
        g = torch.randn(n, device="cuda", generator=g0) * gstd * step
        # reference: the summed gradient is averaged over ranks first (grad_scale = 1 / world), then clipped, then stepped
        ref_p.grad = (g * grad_scale).clone()
        total = None
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
        # product: sum g^2 of the UNSCALED local buffer, scale + clip folded into the AdamW pass
        ops.sqnorm(g, nsq)
        if total is not None:
            assert abs(nsq.sqrt().item() * grad_scale - total.item()) <= 2e-6 * total.item(), (nsq.sqrt().item() * grad_scale, total.item())
        ops.adamw_step(w, w16, g, m, v, lr, b1, b2, eps, wd, step, nsq if max_norm is not None else None,
                       0.0 if max_norm is None else max_norm, grad_scale)
        st = opt.state[ref_p]
        assert _rel(w, ref_p.data) < 1e-6, (step, _rel(w, ref_p.data))
        assert _rel(m, st["exp_avg"]) < 1e-6 and _rel(v, st["exp_avg_sq"]) < 2e-6
        assert (w - ref_p.data).abs().max().item() < 1e-7      # lr * O(1) update, fp32 rounding only
        assert torch.equal(w16, w.to(torch.bfloat16))
    assert not torch.equal(w, torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 0.02)


def test_sqnorm_accumulates_with_beta():
    from mixgrpo_amd import ops
    g = torch.randn(3 * 4096 + 4, device="cuda")
    out = torch.full((1,), 2.0, device="cuda")
    ops.sqnorm(g, out, beta=1.0)
    assert abs(out.item() - (2.0 + g.double().pow(2).sum().item())) < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# Edges of csrc/optim.hip: the scalar tail and the finish loop of mgx_sqnorm_f32, the capped multi-trip grids (4096 blocks
# for sqnorm, 8192 for AdamW and scale: what the production store runs), the host-side bias corrections at large step
# counts, the bf16 mirror's rounding, and a non-finite gradient norm.  References: fp64 sums; the fp64 AdamW recurrence with
# its elementwise budget (tests/optim_refs.py, where the budget is derived; its premise is measured on the CPU in
# tests/test_optim_host.py); torch.optim.AdamW / clip_grad_norm_ on the device.

import optim_refs as R                                                                             # noqa: E402

SQNORM_CAP = 2 * 4096 * 8192 + 3 * 1024 + 3      # 4096 blocks x 2 full trips, a partial third trip, a scalar tail of 3
ADAMW_CAP = 2 * 8192 * 4096 + 3 * 4096 + 4       # 8192 blocks x 2 full trips, a partial third trip ending in one float4
PAD = 64
F32_SENTINEL, BF16_SENTINEL = 0x7FC12345, 0x7FC1                     # NaNs with a payload: any write or read shows


def _padded(x, dtype=torch.float32):
    """x followed by PAD sentinel elements; returns (whole buffer, the view of x's elements)."""
    n = x.numel()
    if dtype == torch.float32:
        buf = torch.full((n + PAD,), F32_SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        buf = torch.full((n + PAD,), BF16_SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    buf[:n] = x
    return buf, buf[:n]


def _pad_intact(buf, n):
    ints = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)[n:]
    return bool((ints == (F32_SENTINEL if buf.dtype == torch.float32 else BF16_SENTINEL)).all())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8191, 8193, 256 * 8192 + 8192 + 5, SQNORM_CAP])
def test_sqnorm_sizes(n):
    """The scalar tail alone (1, 3) and after vectors (5, 8191, 8193: two blocks), 258 partials in the finish kernel's loop,
    and the capped grid with a partial last trip plus the tail; beta = 0 onto a stale value."""
    from mixgrpo_amd import ops
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
    out = torch.full((1,), 123.0, device="cuda")
    ops.sqnorm(g, out)
    ref = g.double().pow(2).sum().item()
    assert abs(out.item() - ref) <= 2e-6 * ref, (n, out.item(), ref)


def test_sqnorm_counts_every_element_once():
    """A relative bound cannot see one dropped or doubled float4 among 6.7e7.  With g = 1 on a window of <= 2^23 elements and
    0 elsewhere every partial sum is an integer below 2^24, so the result is the window's length EXACTLY; the windows sweep
    the whole capped-grid buffer and the last one ends at n: it holds the scalar tail."""
    from mixgrpo_amd import ops
    n, win = SQNORM_CAP, 1 << 23
    g = torch.zeros(n, device="cuda")
    los = list(range(0, n, win))
    outs = torch.full((len(los),), -1.0, device="cuda")
    for k, lo in enumerate(los):
        hi = min(lo + win, n)
        g[lo:hi] = 1.0
        ops.sqnorm(g, outs[k:k + 1])
        g[lo:hi] = 0.0
    assert los[-1] + win > n and n % 4 == 3
    assert outs.tolist() == [float(min(lo + win, n) - lo) for lo in los], outs.tolist()


def test_sqnorm_beta_zero_never_reads_the_old_value():
    """FusedAdamW.grad_sqnorm reuses one device scalar with beta = 0: after one overflowing or NaN norm the next one must be
    the plain sum again (0 * inf and 0 * NaN are NaN).  beta = 1 still accumulates."""
    from mixgrpo_amd import ops
    g = torch.randn(8193, device="cuda")
    ref = g.double().pow(2).sum().item()
    for stale in (float("nan"), float("inf"), -float("inf")):
        out = torch.full((1,), stale, device="cuda")
        ops.sqnorm(g, out)
        assert abs(out.item() - ref) <= 2e-6 * ref, (stale, out.item(), ref)
    out = torch.full((1,), 2.0, device="cuda")
    ops.sqnorm(g, out, beta=1.0)
    assert abs(out.item() - (2.0 + ref)) <= 2e-6 * (2.0 + ref)
    out = torch.full((1,), float("inf"), device="cuda")
    ops.sqnorm(g, out, beta=1.0)
    assert out.item() == float("inf")


def test_sqnorm_refuses_a_misaligned_gradient():
    from mixgrpo_amd import _lib, ops
    g = torch.randn(4100, device="cuda")
    out = torch.full((1,), 7.0, device="cuda")
    with pytest.raises(_lib.MgxError, match="aligned"):
        ops.sqnorm(g[1:], out)
    assert out.item() == 7.0


def _adamw_launch(w, w16, g, m, v, step, hp, nsq=None, max_norm=0.0):
    from mixgrpo_amd import ops
    ops.adamw_step(w, w16, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, nsq, max_norm, 1.0)


def _assert_budget(got, ref, tol, what, scale=1.0):
    frac = ((got.double() - ref).abs() / (scale * tol).clamp_min(1e-300)).max().item()
    assert frac <= 1.0, (what, frac)


@pytest.mark.parametrize("n", [4, ADAMW_CAP])
def test_adamw_capped_grid_two_steps(n):
    """Every element is updated exactly once per launch at the size where the grid is capped and threads loop: two steps at
    lr = 1e-2 against the fp64 recurrence, elementwise inside the derived budget (~1e-8; a skipped element is off by 1e-2, a
    twice-updated one shows in m and v), w16 == bf16(w) bit for bit, and the 64 elements behind every buffer untouched."""
    w0, g = R.adamw_data(0, n, "cuda")
    (wb, w), (mb, m), (vb, v) = _padded(w0), _padded(torch.zeros_like(w0)), _padded(torch.zeros_like(w0))
    w16b, w16 = _padded(torch.zeros(n, device="cuda", dtype=torch.bfloat16), torch.bfloat16)
    w16b[:n] = w16b[n]                                                              # nothing valid in the mirror yet
    gb, g = _padded(g)
    del w0
    chunk = 1 << 24
    for step in (1, 2):
        _adamw_launch(w, w16, g, m, v, step, R.HP)
        assert torch.equal(w16.view(torch.int16), w.to(torch.bfloat16).view(torch.int16)), step
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            w_ref, g_ref = (t.double() for t in R.adamw_data(lo, hi, "cuda"))
            ref, tol = [w_ref, torch.zeros_like(w_ref), torch.zeros_like(w_ref)], R.zeros_like3(w_ref)
            for s in range(1, step + 1):
                R.adamw_ref_step(*ref, tol, g_ref, step=s, **R.HP)
            for name, got, r, t in zip("wmv", (w, m, v), ref, tol):
                _assert_budget(got[lo:hi], r, t, (step, lo, name))
    for buf in (wb, mb, vb, w16b, gb):
        assert _pad_intact(buf, n)


@pytest.mark.parametrize("step,wd", [(1, 1e-2), (2, 1e-2), (2, 0.0), (1000, 1e-2), (100000, 1e-2)])
def test_adamw_step_counts_vs_torch(step, wd):
    """The host-side bias corrections 1 - beta^step at small and large step counts, from non-zero moments, with and without
    weight decay: against torch.optim.AdamW with its state's `step` set.  Both sides are fp32 evaluations inside the budget
    around the fp64 recurrence (the kernel: asserted here; torch: measured on the CPU), so they differ by at most two."""
    n = 4096
    hp = dict(R.HP, wd=wd)
    w0, g = R.adamw_data(0, n, "cuda")
    m0, v0 = R.hashed(0, n, 3, "cuda") * 0.01, (R.hashed(0, n, 4, "cuda") + 0.5) * 1e-4
    w, m, v = w0.clone(), m0.clone(), v0.clone()
    w16 = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    _adamw_launch(w, w16, g, m, v, step, hp)
    ref, tol = [w0.double(), m0.double(), v0.double()], R.zeros_like3(w0)
    R.adamw_ref_step(*ref, tol, g.double(), step=step, **hp)
    theirs = R.torch_adamw_step(w0, m0, v0, g, step, **hp)
    for name, got, r, t, th in zip("wmv", (w, m, v), ref, tol, theirs):
        _assert_budget(got, r, t, (step, name))
        _assert_budget(got, th.double(), t, (step, name, "torch"), scale=2.0)
    assert torch.equal(w16.view(torch.int16), w.to(torch.bfloat16).view(torch.int16))


def test_adamw_lr_zero_is_the_identity_and_w16_rounds_to_nearest_even():
    """lr = 0 with zero g, m, v: w bit-identical.  Its bits are chosen so that the mirror is a rounding test: the 16 dropped
    bits just below, at and just above one half, both parities of the kept mantissa's last bit, both signs."""
    bits = [(s << 31) | ((0x3F80 | parity) << 16) | low for s in (0, 1) for parity in (0, 1) for low in (0x7FFF, 0x8000, 0x8001)]
    w0 = torch.tensor([b - (1 << 32) if b >> 31 else b for b in bits], dtype=torch.int32).view(torch.float32).cuda()
    n = w0.numel()
    assert n % 4 == 0
    w, z = w0.clone(), torch.zeros(n, device="cuda")
    m, v = z.clone(), z.clone()
    w16 = torch.full((n,), BF16_SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    _adamw_launch(w, w16, z, m, v, 1, dict(R.HP, lr=0.0))
    assert torch.equal(w.view(torch.int32), w0.view(torch.int32))
    assert torch.equal(w16.view(torch.int16), w0.to(torch.bfloat16).view(torch.int16))
    # and with the rule itself: up above one half, and at one half when the kept mantissa is odd
    want = [(b >> 16) + ((b & 0xFFFF) > 0x8000 or ((b & 0xFFFF) == 0x8000 and (b >> 16) & 1 == 1)) for b in bits]
    assert [x & 0xFFFF for x in w16.view(torch.int16).tolist()] == want
    assert not m.any() and not v.any()


def _clip_then_step(w0, g, max_norm, hp):
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt.step()
    return total, p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_adamw_non_finite_norm_follows_clip_grad_norm(bad):
    """clip_grad_norm_'s coefficient is clamp(max_norm / (norm + 1e-6), max=1): a NaN norm makes it NaN and every gradient and
    weight NaN -- it must not become 1 (clipping silently off); an infinite norm makes it 0: gradients vanish, the weights
    only decay."""
    from mixgrpo_amd import ops
    n = 4096
    w0, g = R.adamw_data(0, n, "cuda")
    if bad == "nan":
        g[5] = float("nan")
    else:
        g[5] = g[6] = 3e38                                         # the norm itself exceeds fp32: inf however it is summed
    total, w_t, m_t, v_t = _clip_then_step(w0, g, 1.0, R.HP)
    nsq = torch.zeros(1, device="cuda")
    ops.sqnorm(g, nsq)
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    w16 = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    _adamw_launch(w, w16, g, m, v, 1, R.HP, nsq, 1.0)
    if bad == "nan":
        assert torch.isnan(total) and torch.isnan(nsq).all()
        assert torch.isnan(w_t).all() and torch.isnan(w).all() and torch.isnan(w16).all()
        # the norm alone decides: a NaN norm over finite gradients (another rank's) does the same
        w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
        _adamw_launch(w, w16, R.adamw_data(0, n, "cuda")[1], m, v, 1, R.HP, nsq, 1.0)
        assert torch.isnan(w).all()
    else:
        assert torch.isinf(total) and torch.isinf(nsq).all()
        assert not m_t.any() and not v_t.any() and not m.any() and not v.any()
        assert torch.isfinite(w).all()
        assert ((w.double() - w_t.double()).abs() <= 2 * R.ULP * w0.double().abs()).all()      # the decay's two roundings
        assert torch.equal(w16.view(torch.int16), w.to(torch.bfloat16).view(torch.int16))


class _Store:
    """What FusedAdamW needs of a flat store."""

    def __init__(self, w):
        self.device, self.numel = w.device, w.numel()
        self.w32, self.w16, self.g32 = w, w.to(torch.bfloat16), torch.zeros_like(w)

    def ensure_grad(self):
        return self.g32


def test_fused_adamw_recovers_from_an_overflowing_gradient():
    """One step whose gradient norm overflows (one element 1e20), then a normal one: the second step's clip coefficient is
    the one torch computes from that step's gradient alone -- not NaN, and not 1."""
    from mixgrpo_amd.optim import FusedAdamW
    n = 4096
    hp = dict(R.HP, lr=1e-3)
    w0, g2 = R.adamw_data(0, n, "cuda")
    g2 = g2 * 50                                                   # |g2| ~ 18: the clip is active
    g1 = g2.flip(0).clone()
    g1[7] = 1e20
    p = torch.nn.Parameter(w0.clone())
    ref = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    store = _Store(w0.clone())
    opt = FusedAdamW(None, lr=hp["lr"], betas=(hp["b1"], hp["b2"]), weight_decay=hp["wd"], eps=hp["eps"], store=store)
    totals = []
    for g in (g1, g2):
        p.grad = g.clone()
        totals.append(torch.nn.utils.clip_grad_norm_([p], 1.0))
        ref.step()
        store.g32.copy_(g)
        opt.step(max_grad_norm=1.0)
    assert torch.isinf(totals[0])
    coef_ref = torch.clamp(1.0 / (totals[1] + 1e-6), max=1.0).item()
    coef = torch.clamp(1.0 / (opt.gnorm_sq.sqrt() + 1e-6), max=1.0).item()
    assert 0 < coef_ref < 0.5
    assert abs(coef - coef_ref) <= 2e-6 * coef_ref, (coef, coef_ref)
    # lr 1e-3 x an O(1) update, fp32 rounding on both sides (the bound form of test_adamw_and_sqnorm_vs_torch)
    assert torch.isfinite(store.w32).all() and (store.w32 - p.data).abs().max().item() < 1e-7
    assert torch.equal(store.w16.view(torch.int16), store.w32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("n", [4, ADAMW_CAP])
def test_scale_f32_is_bit_equal_to_torch(n):
    from mixgrpo_amd import _lib as L
    x0 = R.hashed(0, n, 5, "cuda")
    buf, x = _padded(x0)
    L.check(L.lib().mgx_scale_f32(L.ptr(x), n, 0.3, L.stream()))
    assert torch.equal(x.view(torch.int32), (x0 * 0.3).view(torch.int32))
    assert _pad_intact(buf, n)
