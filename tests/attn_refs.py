"""float64 restatements of the bf16 attention kernels (csrc/attention.hip, csrc/attention_bwd.hip), seeded input families,
per-row error budgets and the predicates the kernel-level tests use.  Plain torch, device-agnostic: the GPU tests
(test_hip_attention_kernels.py) evaluate everything on the device in float64, the CPU test (test_attn_refs.py) checks the closed
form against autograd, calibrates the constants below and checks that every predicate can see the faults it is there for.

Layout: q, k, v, do and every output are [B, H, S, 128]; lse, delta and the budgets are [B, H, S].  Everything is computed on
chunks of (batch, head)s whose S x S float64 matrices stay below 256 MB each -- one head at a time at S = 4608 (170 MB per
matrix, about ten alive) -- so full tensors are checked at full size.

Mathematics (s = softmax scale):  P = softmax(s Q K^T), O = P V, lse = logsumexp(s Q K^T);
  dV = P^T dO, dP = dO V^T, delta_r = sum_d dO_rd O_rd, dS = P * (dP - delta) (unscaled), dQ = s dS K, dK = s dS^T Q.
The prescaled path (mgx_attn_fwd_log2, mgx_attn_bwd at scale = ln 2) is the same mathematics on q2 = bf16(q log2(e) / sqrt(128))
with s = ln 2: the reference is taken ON q2 (`to_log2`), and dQ is the gradient with respect to q2.

`rounding_model` is float64 with bf16 roundings only where the kernels' contract puts them: P before P V (against a maximum that is not the final normaliser, see below) and before P^T dO, dS
(times s) before its two products, O before delta, every bf16 output; the scores come from an fp32 matmul so that their summation
order differs from the reference's.  It is the yardstick for the constants and is never replaced by a kernel.

Per-row budgets, u = 2^-9 (half a bf16 ulp, relative), norms over the 128 head columns:
  O_r  : u (|O_r| + sqrt(sum_d sum_j P_rj^2 V_jd^2))                      output rounding + independent roundings of P_rj
  dV_j : u (|dV_j| + sqrt(sum_d sum_r P_rj^2 dO_rd^2))
  eps_r = u sqrt(sum_d dO_rd^2 O_rd^2)                                    error of delta_r caused by the bf16 O
  dQ_r : u (|dQ_r| + s sqrt(sum_d sum_j dS_rj^2 K_jd^2)) + s eps_r |sum_j P_rj K_j|
  dK_j : u (|dK_j| + s sqrt(sum_d sum_r dS_rj^2 Q_rd^2)) + s sqrt(sum_r P_rj^2 eps_r^2 |Q_r|^2)
`rows_close(out, ref, budget, c)`: |out_r - ref_r|_2 <= c budget_r for EVERY row.

Calibration (test_attn_refs.py::test_rounding_model_passes_every_predicate recomputes it): worst row of `rounding_model` against
the float64 reference over every family, S in {300, 1024, 2048}, both scales, B = 1, H = 8 (27000 rows per family and scale: the
worst of N rows grows with N, like sqrt(2 ln N), and the kernel tests check up to 130000 rows per case), in units of the budget:
  O 1.48 (spike, S = 2048)   dV 1.22 (peaked, S = 2048)   dQ 5.70 (spike, S = 2048)   dK 4.60 (peaked, S = 300)
  (uniform alone: 0.8 .. 1.0 for all four; peaked: dQ, dK 3.4 .. 4.6; ramp: dQ 1.9 .. 2.5; spike: dQ 4.2 .. 5.7.  These are
  tail statistics: other seeds of t moved the dQ / dK figures by about one unit either way.)
Without the two eps terms the dQ / dK ratios reach the hundreds on peaked rows: there dS = P (dP - delta) cancels and the error
of delta, inherited from the bf16 O, is all that is left.  What keeps peaked rows at 3 .. 6 is the share of O's error that the
budget's eps does not name: eps is the output rounding of O alone, while the rounding of the row's dominant P_rj moves O_r, and
with it delta_r, by up to u P_rj |dO_r . V_j| more.
The tests use C = 1.5 x MEASURED (O 2.22, dV 1.83, dQ 8.55, dK 6.90): the factor covers the kernels' different summation order,
the position of the running maximum, and hardware exp2.
The model rounds the forward's P as bf16(P t) / t with a seeded t in [1, 2) per row.  A first version rounded the normalised P
itself (t = 1) and was calibrated on H = 2: 1.20 / 1.21 / 4.64 / 3.39.  On the GPU the generated 64-query forward then needed
5.33 for one dK row of the peaked (3, 8, 512) case (bar 5.09) while the 8-wave forward needed 3.2.  Cause, measured there: the
64-query kernel rounds exp(s - m) against the FIRST tile's maximum, so a dominant P = 0.95 is rounded at an arbitrary mantissa
(error up to u), where the model rounded it just below 1 (error up to u / 2) and the 8-wave kernel, whose running maximum
makes the dominant entry exactly 1, does not round it at all; per row, delta's error / eps was 1.17 rms, 7.4 max (64-query),
1.14 rms, 5.7 max (model), 0.85 rms, 3.7 max (8-wave).  No extra rounding point: the model was made to match the contract (t),
and its calibration set enlarged.

Other bars: lse |lse - ref| <= 1e-4 + 1e-4 |ref| (the project's existing bar, in float64); delta within 128 * 2^-24 * sum_d |dO O|
of the float64 sum over the bf16 O that was passed in (an fp32 sum of 128 products); dOt the bit-exact transpose of the head's dO
columns with zeros in the padding columns.

`rounded_once(out)`: a bf16 tensor that was rounded ONCE to nearest-even from a wider value has an unbiased last mantissa bit.
A detour through fp16 (11 bits) lands 1/16 of the values exactly on a bf16 tie, which then all go to the even neighbour: the
share of even last bits rises from 0.5 to 0.56, while it moves the row error by less than a percent of the budget, far below
what rows_close can see.  Bar: |share - 0.5| <= 0.01 + 2.5 / sqrt(N), five binomial standard deviations plus 0.01 for the slope
of the values' density across one ulp (2^-8 relative per step; measured on the rounding model: <= 0.004 at N = 76800); N counts
the non-zero elements (an exact zero carries no rounding).

What the predicates do NOT see (test_attn_refs.py records it): delta taken from an fp32 O instead of the bf16 one changes dQ / dK
by about eps, inside their budgets by construction (it is the better value); delta_close pins that contract instead."""
import math

import torch

F64 = torch.float64
HD = 128
U = 2.0 ** -9
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
SCALE = 1 / math.sqrt(HD)
FAMILIES = ("uniform", "peaked", "ramp", "spike")
BF16_MAX = 3.3895313892515355e38          # largest finite bf16

# worst row of rounding_model / budget over the calibration set, rounded up (see the module docstring)
MEASURED = {"O": 1.48, "dV": 1.22, "dQ": 5.70, "dK": 4.60}
C = {k: 1.5 * v for k, v in MEASURED.items()}


def bf(x):
    """Round to bf16 through fp32 (as a kernel rounds its fp32 value) and return float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------------------------------------------------ input families
def make_inputs(family, B, H, S, seed, device="cpu"):
    """(q, k, v, do), bf16 [B, H, S, 128], drawn on `device` from `seed`.
    uniform: randn, scores ~ N(0, 1), row maximum of P a few percent.
    peaked : k = 0.7 q[perm] + sqrt(0.51) noise: each query has one key with score ~ 8, median row maximum of P >= 0.3.
    ramp   : keys drift along the sequence (k += 3 * j / S * sign(mean q)): the running maximum keeps growing, the forward's
             deferred-rescale path with P > 1 (test_attention_deferred_rescale_paths).
    spike  : randn with a few keys = 6..8 x some query (scores ~ 70..90 nats above the rest): the 64-query forward's overflow
             fix-up (test_attention_fwd64_rescale_path), rows whose P is one-hot."""
    assert family in FAMILIES
    g = torch.Generator(device=device).manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, S, HD, generator=g, device=device) for _ in range(4))
    q = q.bfloat16().float()
    if family == "peaked":
        perm = torch.randperm(S, generator=g, device=device)
        k = 0.7 * q[:, :, perm] + math.sqrt(0.51) * k
    elif family == "ramp":
        ramp = torch.linspace(0, 1, S, device=device).view(1, 1, S, 1)
        k = k + 3.0 * ramp * q.mean(dim=2, keepdim=True).sign()
    elif family == "spike":
        for key, row, gain in ((200, 70, 8.0), (S - 3, 100, 6.0), (333, 700, 7.0), (S // 2, S - 1, 8.0)):
            k[:, :, key % S] = gain * q[:, :, row % S]
    return tuple(t.bfloat16() for t in (q, k, v, do))


def to_log2(q):
    """q2 = bf16(q * log2(e) / sqrt(128)): what mgx_qk_norm_rope_fwd_qs hands to mgx_attn_fwd_log2 (scale = ln 2 from there on)."""
    return (q.float() * (LOG2E / math.sqrt(HD))).bfloat16()


# ------------------------------------------------------------------------------------------------------- a chunk of (batch, head)s
def _T(x):
    return x.transpose(-1, -2)


def _head(q, k, v, do, s, model=False):
    """float64 forward + closed-form backward of a chunk of heads ([n, S, 128] operands).  model=True: the rounding model."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    rnd = bf if model else (lambda t: t)
    if model:
        sc = (q.float() @ _T(k.float())).to(F64) * s
    else:
        sc = (q @ _T(k)) * s
    lse = torch.logsumexp(sc, -1)
    P = torch.exp(sc - lse[..., None])
    Pb = rnd(P)
    Pf = Pb
    if model:
        # the forward rounds exp(s - m) for a maximum m that is not the final normaliser (a running or first-tile maximum), so
        # the mantissa its rounding sees is unrelated to P's own: a seeded factor in [1, 2) per row stands for exp(lse - m)
        t = (2.0 ** torch.rand(*P.shape[:-1], 1, generator=torch.Generator().manual_seed(P.shape[-1]), dtype=F64)).to(P.device)
        Pf = bf(P * t) / t
    out = {"lse": lse, "O": rnd(Pf @ v), "P": P}
    if do is None:
        return out
    do = do.to(F64)
    out["delta"] = (do * out["O"]).sum(-1)
    dS = P * (do @ _T(v) - out["delta"][..., None])
    out["dS"] = dS
    out["dV"] = rnd(_T(Pb) @ do)
    if model:
        dSb = bf(dS * s)
        out["dQ"], out["dK"] = bf(dSb @ k), bf(_T(dSb) @ q)
    else:
        out["dQ"], out["dK"] = s * (dS @ k), s * (_T(dS) @ q)
    return out


def _head_budgets(q, k, v, do, s, r):
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    n = lambda t: t.norm(dim=-1)
    P2 = r["P"] ** 2
    b = {"O": U * (n(r["O"]) + (P2 @ v ** 2).sum(-1).sqrt())}
    if do is None:
        return b
    do = do.to(F64)
    dS2 = r["dS"] ** 2
    eps = U * ((do * r["O"]) ** 2).sum(-1).sqrt()
    b["dV"] = U * (n(r["dV"]) + (_T(P2) @ do ** 2).sum(-1).sqrt())
    b["dQ"] = U * (n(r["dQ"]) + s * (dS2 @ k ** 2).sum(-1).sqrt()) + s * eps * n(r["P"] @ k)
    b["dK"] = U * (n(r["dK"]) + s * (_T(dS2) @ q ** 2).sum(-1).sqrt()) + \
        s * (_T(P2) @ (eps ** 2 * (q ** 2).sum(-1))[..., None]).squeeze(-1).sqrt()
    return b


CHUNK_BYTES = 256 << 20            # of one [n, S, S] float64 matrix: n = 1 at S = 4608 (170 MB), every head at once when S is small


def _per_head(fn, q, *rest):
    """fn on chunks of (batch, head)s: a chunk's S x S matrices (about ten live at a time) stay within CHUNK_BYTES each."""
    B, H, S = q.shape[:3]
    flat = [None if t is None else t.reshape(B * H, *t.shape[2:]) for t in (q,) + rest]
    n = max(1, CHUNK_BYTES // (8 * S * S))
    acc = {}
    for i in range(0, B * H, n):
        for name, val in fn(*[None if t is None else t[i:i + n] for t in flat]).items():
            acc.setdefault(name, []).append(val)
    return {name: torch.cat(vals).view(B, H, *vals[0].shape[1:]) for name, vals in acc.items()}


# ------------------------------------------------------------------------------------------------------------------ references
def attention_ref(q, k, v, scale):
    """(O [B, H, S, 128], lse [B, H, S], P [B, H, S, S]) in float64 (P kept: small problems only)."""
    r = _per_head(lambda q_, k_, v_: _head(q_, k_, v_, None, scale), q, k, v)
    return r["O"], r["lse"], r["P"]


def attention_bwd_ref(q, k, v, do, scale):
    """(dQ, dK, dV, dS) in float64 from the closed form; dS = P * (dP - delta), unscaled (small problems only: dS is S x S)."""
    r = _per_head(lambda q_, k_, v_, do_: _head(q_, k_, v_, do_, scale), q, k, v, do)
    return r["dQ"], r["dK"], r["dV"], r["dS"]


def reference(q, k, v, do, scale):
    """Everything a kernel test needs, at any size: ({O, lse, delta, dQ, dK, dV, pmax}, budgets {O, dV, dQ, dK}) in float64;
    `do` may be None (forward only).  pmax is the row maximum of P.  No S x S tensor outlives its head."""
    def fn(q_, k_, v_, do_):
        r = _head(q_, k_, v_, do_, scale)
        out = {"b_" + name: val for name, val in _head_budgets(q_, k_, v_, do_, scale, r).items()}
        out["pmax"] = r["P"].max(-1).values
        out.update({name: val for name, val in r.items() if name not in ("P", "dS")})
        return out
    r = _per_head(fn, q, k, v, do)
    return ({n: t for n, t in r.items() if not n.startswith("b_")}, {n[2:]: t for n, t in r.items() if n.startswith("b_")})


def rounding_model(q, k, v, do, scale):
    """{O, lse, delta, dQ, dK, dV} of the rounding model (module docstring), float64 holding bf16 values where the kernels store
    bf16."""
    r = _per_head(lambda q_, k_, v_, do_: _head(q_, k_, v_, do_, scale, model=True), q, k, v, do)
    return {n: t for n, t in r.items() if n not in ("P", "dS")}


# ------------------------------------------------------------------------------------------------------------------ predicates
def row_ratio(out, ref, budget):
    """|out_r - ref_r|_2 / budget_r per row, float64 [B, H, S]."""
    return (out.to(F64) - ref.to(F64)).norm(dim=-1) / budget


def rows_close(out, ref, budget, c):
    """Every row of `out` [B, H, S, 128] within c * budget [B, H, S] of `ref` in L2 over the head columns.  (ok, message)."""
    if not torch.isfinite(out.to(F64)).all():
        return False, "non-finite output"
    ratio = row_ratio(out, ref, budget)
    worst = ratio.max().item()
    if not worst <= c:
        i = int(ratio.flatten().argmax())
        H, S = ratio.shape[1:]
        return False, f"row (b, h, s) = ({i // (H * S)}, {i // S % H}, {i % S}): |out - ref| = {worst:.3g} x budget (> {c:.3g})"
    return True, f"worst row {worst:.3g} x budget"


def lse_close(lse, ref):
    l, r = lse.to(F64), ref.to(F64)
    if not torch.isfinite(l).all():
        return False, "non-finite lse"
    excess = (l - r).abs() - (1e-4 + 1e-4 * r.abs())
    if (excess > 0).any():
        i = int(excess.flatten().argmax())
        return False, f"lse[{i}] = {l.flatten()[i].item()} against {r.flatten()[i].item()}"
    return True, ""


def delta_close(delta, do, o_bf16):
    """delta [B, H, S] against the float64 sum_d dO O over the bf16 O that the backward was given ([B, H, S, 128] both)."""
    prod = do.to(F64) * o_bf16.to(F64)
    d = delta.to(F64)
    if not torch.isfinite(d).all():
        return False, "non-finite delta"
    excess = (d - prod.sum(-1)).abs() - HD * 2.0 ** -24 * prod.abs().sum(-1)
    if (excess > 0).any():
        i = int(excess.flatten().argmax())
        return False, f"delta[{i}] off by {excess.flatten()[i].item():.3g} beyond 128 * 2^-24 * sum|dO O|"
    return True, ""


def rounded_once(out):
    """The last mantissa bit of a bf16 tensor is unbiased (module docstring): no second rounding through a narrower format."""
    bits = out.to(torch.bfloat16).contiguous().view(torch.int16)
    bits = bits[(bits & 0x7FFF) != 0]                      # an exact zero carries no rounding
    if bits.numel() == 0:
        return True, "all zero"
    share = ((bits & 1) == 0).to(F64).mean().item()
    bar = 0.01 + 2.5 / math.sqrt(bits.numel())
    if abs(share - 0.5) > bar:
        return False, f"{share:.4f} of the last mantissa bits are even (0.5 +- {bar:.4f}): rounded more than once?"
    return True, f"even last bits {share:.4f}"


def dot_exact(dOt, do, S):
    """dOt [B, H, 128, Sp] is the transpose of do [B, H, S, 128] bit for bit, zero in the columns S .. Sp - 1."""
    if not torch.equal(dOt[..., :S].view(torch.int16), do.transpose(-1, -2).contiguous().view(torch.int16)):
        return False, "dOt is not the transpose of dO"
    if (dOt[..., S:].view(torch.int16) != 0).any():
        return False, "dOt padding columns are not zero"
    return True, ""


def assert_ok(res):
    ok, msg = res
    assert ok, msg
