"""CPU checks of tests/attn_refs.py: the closed-form backward equals float64 autograd, the rounding model passes every predicate
at the chosen constants (the calibration of attn_refs.C), the input families are what they claim, and every predicate rejects
the faults it is there for.

Faults and who sees them (S = 300, one batch, two heads; test_predicates_reject_*):
  a masked key leaking with score 0       lse (O moves by less than its bf16 rounding: rows_close(O) passes, asserted)
  32 queries of dQ without the last tile  rows_close(dQ)
  32 keys of dK / dV without the last     rows_close(dK), rows_close(dV)
    32-query tile
  two heads swapped                       every rows_close, lse
  O rounded through fp16, then bf16       rounded_once (the last mantissa bit's bias; rows_close passes, asserted)
  delta from an fp32 O                    passes (allowed to: it is the better value; the dQ / dK budgets carry eps for it);
                                          delta_close against the bf16 O rejects it, which is how the kernel test pins the
                                          contract"""
import math

import pytest
import torch

import attn_refs as A
from attn_refs import assert_ok

S0 = 300


def _case(family="uniform", S=S0, seed=1, log2=False, H=2):
    q, k, v, do = A.make_inputs(family, 1, H, S, seed)
    sc = A.SCALE
    if log2:
        q, sc = A.to_log2(q), A.LN2
    return q, k, v, do, sc


def test_closed_form_backward_equals_float64_autograd():
    q, k, v, do, sc = _case("peaked", S=200, seed=3)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(qd @ kd.transpose(-1, -2) * sc, -1) @ vd
    gq, gk, gv = torch.autograd.grad(o, (qd, kd, vd), do.double())
    dQ, dK, dV, dS = A.attention_bwd_ref(q, k, v, do, sc)
    O, lse, P = A.attention_ref(q, k, v, sc)
    for a, b in ((dQ, gq), (dK, gk), (dV, gv), (O, o.detach())):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())
    assert torch.allclose(P.sum(-1), torch.ones_like(lse), rtol=0, atol=1e-13)
    assert torch.allclose(lse, torch.logsumexp(qd.detach() @ kd.detach().transpose(-1, -2) * sc, -1), rtol=0, atol=1e-12)
    ref, _ = A.reference(q, k, v, do, sc)
    assert torch.equal(ref["dQ"], dQ) and torch.equal(ref["O"], O)
    assert torch.equal((dS * dS).sum(), (dS ** 2).sum())


@pytest.mark.parametrize("S", [300, 1024, 2048])
def test_rounding_model_passes_every_predicate(S):
    """The calibration: the worst row of the rounding model is printed (run with -s) and must lie within MEASURED x 1.5 = C,
    every family, both scales."""
    for fi, fam in enumerate(A.FAMILIES):
        for log2 in (False, True):
            q, k, v, do, sc = _case(fam, S, seed=S + 17 * fi, log2=log2, H=8)
            ref, bud = A.reference(q, k, v, do, sc)
            m = A.rounding_model(q, k, v, do, sc)
            for n in ("O", "dV", "dQ", "dK"):
                ok, msg = A.rows_close(m[n], ref[n], bud[n], A.C[n])
                print(f"S {S} {fam} log2 {log2} {n}: {msg}")
                assert ok, (fam, log2, n, msg)
            assert_ok(A.lse_close(m["lse"].float(), ref["lse"]))
            assert_ok(A.delta_close(m["delta"].float(), do, m["O"]))
    assert A.C == {n: 1.5 * A.MEASURED[n] for n in A.MEASURED}


HEAD_DIMS = [16, 32, 48, 64, 80, 96, 112, 128]


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_o_budget_constant_holds_at_every_head_dimension(d):
    """MEASURED["O"] was calibrated at head dimension 128 and the budget is an L2 norm over the head columns; the encoder
    attention tests (test_hip_clip.py, test_hip_text.py, test_hip_image_reward.py) use it from d = 16 on.  The rounding model
    alone against the float64 reference on randn bf16 operands, 2 x 3 heads as those tests use, at the sequence lengths around
    their blocks of 64 keys: the worst row is printed (run with -s) and must lie within MEASURED["O"], so that C["O"] keeps its
    factor of 1.5 for the kernel at every d."""
    worst = 0.0
    for S in (2, 5, 17, 64, 70, 130, 257):
        g = torch.Generator().manual_seed(1000 * d + S)
        q, k, v = (torch.randn(6, S, d, generator=g).bfloat16() for _ in range(3))
        sc = d ** -0.5
        ref = A._head(q, k, v, None, sc)
        ratio = A.row_ratio(A._head(q, k, v, None, sc, model=True)["O"], ref["O"], A._head_budgets(q, k, v, None, sc, ref)["O"])
        worst = max(worst, ratio.max().item())
    print(f"d {d}: worst row of the rounding model {worst:.3g} x budget")
    assert worst <= A.MEASURED["O"]


def test_families_are_what_they_claim():
    for S in (300, 1024):
        med = {}
        for fam in A.FAMILIES:
            q, k, v, do, sc = _case(fam, S, seed=5)
            for t in (q, k, v, do):
                assert t.dtype == torch.bfloat16 and torch.isfinite(t.float()).all()
            q2 = A.make_inputs(fam, 1, 2, S, 5)[0]
            assert torch.equal(q, q2)                                      # seeded
            ref, _ = A.reference(q, k, v, None, sc)
            med[fam] = ref["pmax"].median().item()
        assert med["peaked"] >= 0.3 and med["uniform"] <= 0.1, med
        assert med["spike"] > med["uniform"]
    q, k, v, do, sc = _case("spike", 1024, seed=5)
    ref, _ = A.reference(q, k, v, None, sc)
    assert ref["pmax"][0, 0, 70] > 0.999                                     # a one-hot row


def _ref_and_model(family="uniform", log2=False):
    q, k, v, do, sc = _case(family, log2=log2)
    ref, bud = A.reference(q, k, v, do, sc)
    return (q, k, v, do, sc), ref, bud, A.rounding_model(q, k, v, do, sc)


def test_predicates_reject_a_leaking_masked_key():
    """One padding key taking part with score 0 (V = 0): O moves by less than the bf16 rounding, only lse can see it."""
    (q, k, v, do, sc), ref, bud, m = _ref_and_model()
    s = q.double() @ k.double().transpose(-1, -2) * sc
    s2 = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
    O2 = A.bf(torch.softmax(s2, -1)[..., :S0] @ v.double())
    lse2 = torch.logsumexp(s2, -1).float()
    assert A.rows_close(O2, ref["O"], bud["O"], A.C["O"])[0]                # invisible in O
    assert not A.lse_close(lse2, ref["lse"])[0]


@pytest.mark.parametrize("family", ["uniform", "peaked"])
def test_predicates_reject_a_lost_tile(family):
    (q, k, v, do, sc), ref, bud, m = _ref_and_model(family)
    _, _, _, dS = A.attention_bwd_ref(q, k, v, do, sc)
    _, _, P = A.attention_ref(q, k, v, sc)
    last_k = (S0 - 1) // 64 * 64                                             # first key of the last 64-key tile
    last_q = (S0 - 1) // 32 * 32                                             # first query of the last 32-query tile
    dQ = m["dQ"].clone()
    dQ[0, 1, 32:64] = A.bf(A.bf(dS[0, 1, 32:64, :last_k] * sc) @ k[0, 1, :last_k].double())
    assert A.rows_close(m["dQ"], ref["dQ"], bud["dQ"], A.C["dQ"])[0]
    ok, msg = A.rows_close(dQ, ref["dQ"], bud["dQ"], A.C["dQ"])
    assert not ok and "(0, 1, " in msg
    dK, dV = m["dK"].clone(), m["dV"].clone()
    dK[0, 0, 64:96] = A.bf(A.bf(dS[0, 0, :last_q, 64:96] * sc).transpose(-1, -2) @ q[0, 0, :last_q].double())
    dV[0, 0, 64:96] = A.bf(A.bf(P[0, 0, :last_q, 64:96]).transpose(-1, -2) @ do[0, 0, :last_q].double())
    assert not A.rows_close(dK, ref["dK"], bud["dK"], A.C["dK"])[0]
    assert not A.rows_close(dV, ref["dV"], bud["dV"], A.C["dV"])[0]


def test_predicates_reject_swapped_heads():
    _, ref, bud, m = _ref_and_model()
    for n in ("O", "dV", "dQ", "dK"):
        assert not A.rows_close(m[n].flip(1), ref[n], bud[n], A.C[n])[0]
    assert not A.lse_close(m["lse"].flip(1).float(), ref["lse"])[0]


def test_predicates_reject_non_finite_and_report_the_row():
    _, ref, bud, m = _ref_and_model()
    O = m["O"].clone()
    O[0, 1, 7, 3] = float("nan")
    assert A.rows_close(O, ref["O"], bud["O"], A.C["O"]) == (False, "non-finite output")
    O = m["O"].clone()
    O[0, 1, 7] += 1
    ok, msg = A.rows_close(O, ref["O"], bud["O"], A.C["O"])
    assert not ok and "(0, 1, 7)" in msg


def test_double_rounding_of_o_through_fp16_is_rejected():
    """O rounded to fp16 and then to bf16 instead of once to bf16: 6 % of the elements move by one ulp, the worst row moves from
    0.825 to 0.832 (uniform) / 0.972 to 0.951 (peaked) x budget against C = 2.22 -- invisible to a per-row L2 budget that admits
    one honest rounding.  `rounded_once` sees it: every value the fp16 step put on a bf16 tie goes to the even neighbour (share
    of even last bits 0.56 against 0.5 +- 0.019)."""
    for family in ("uniform", "peaked"):
        (q, k, v, do, sc), ref, bud, m = _ref_and_model(family)
        O, _, P = A.attention_ref(q, k, v, sc)
        exact = A.bf(P) @ v.double()
        once, twice = A.bf(exact), exact.to(torch.float16).to(torch.bfloat16).double()
        assert 0.03 < (once != twice).double().mean().item() < 0.1
        assert A.rows_close(once, ref["O"], bud["O"], A.C["O"])[0]
        assert A.rows_close(twice, ref["O"], bud["O"], A.C["O"])[0]         # recorded: the row budget cannot see it
        assert_ok(A.rounded_once(once))
        assert not A.rounded_once(twice)[0]
        for n in ("O", "dV", "dQ", "dK"):
            assert_ok(A.rounded_once(m[n]))


def test_delta_from_an_fp32_o_passes_the_gradient_budgets_and_fails_the_delta_bar():
    """delta formed from the unrounded O (not the contract: the prep kernel reads the bf16 O): dQ / dK get BETTER, so the row
    budgets pass -- recorded, allowed by design -- while delta_close, which is taken against the bf16 O, rejects it."""
    for family in ("uniform", "peaked"):
        (q, k, v, do, sc), ref, bud, m = _ref_and_model(family)
        _, _, P = A.attention_ref(q, k, v, sc)
        qd, kd, vd, dd = (t.double() for t in (q, k, v, do))
        delta32 = (dd * (A.bf(P) @ vd)).sum(-1)
        dSb = A.bf(P * (dd @ vd.transpose(-1, -2) - delta32[..., None]) * sc)
        dQ, dK = A.bf(dSb @ kd), A.bf(dSb.transpose(-1, -2) @ qd)
        assert A.rows_close(dQ, ref["dQ"], bud["dQ"], A.C["dQ"])[0]
        assert A.rows_close(dK, ref["dK"], bud["dK"], A.C["dK"])[0]
        assert A.delta_close(m["delta"].float(), do, m["O"])[0]
        assert not A.delta_close(delta32.float(), do, m["O"])[0]


def test_dot_exact_and_budget_shapes():
    q, k, v, do, sc = _case(S=70)
    dOt = torch.zeros(1, 2, 128, 128, dtype=torch.bfloat16)
    dOt[..., :70] = do.transpose(-1, -2)
    assert_ok(A.dot_exact(dOt, do, 70))
    bad = dOt.clone()
    bad[0, 1, 5, 100] = 1.0
    assert not A.dot_exact(bad, do, 70)[0]
    bad = dOt.clone()
    bad[0, 1, 5, 3] = -bad[0, 1, 5, 3] if bad[0, 1, 5, 3] != 0 else 1.0
    assert not A.dot_exact(bad, do, 70)[0]
    ref, bud = A.reference(q, k, v, do, sc)
    for n in ("O", "dV", "dQ", "dK"):
        assert bud[n].shape == (1, 2, 70) and (bud[n] > 0).all() and ref[n].shape == (1, 2, 70, 128)
    q1, k1, v1, do1 = A.make_inputs("spike", 2, 1, 1, 0)                     # S = 1: P = 1, dS = 0
    ref, bud = A.reference(q1, k1, v1, do1, sc)
    assert torch.equal(ref["O"], v1.double()) and (bud["dQ"] > 0).all() and (bud["dK"] > 0).all()
