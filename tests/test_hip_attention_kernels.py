"""Every bf16 attention kernel of csrc/attention.hip and csrc/attention_bwd.hip against the float64 references and per-row
budgets of tests/attn_refs.py: the 8-wave forward, the two generated 64-query forwards (attn_fwd64 through mgx_attn_fwd,
attn_fwd64q through mgx_attn_fwd_log2), the prep kernel (delta, dOt) and the 8-wave and generated 64-wide dkv / dq kernels.

One case = one shape, one input family, one output layout.  It runs the forward through both entries (scale 1 / sqrt(128) on q,
and the prescaled q2 with exponents of two) and the backward on each forward's own O and lse (scale 1 / sqrt(128) and ln 2), as
the model does, and checks
  * the kernels the dispatch takes (mgx_attn_fwd_path / mgx_attn_bwd_path) against the case's stated expectation AND against a
    restatement of the dispatch rule in this file;
  * EVERY row of O, dQ, dK, dV with rows_close at attn_refs.C, lse and delta at their bars, dOt bit for bit, the last-bit test
    rounded_once on every bf16 output;
  * what a kernel must not touch, bit for bit: O is written into a buffer of NaN sentinels -- the columns outside the head
    block (ldo = 5 H 128 at a column offset: the single blocks' `cat` buffer) and the gap between batches when
    o_bstride > S ldo must come back unchanged -- and lse, delta, dOt, dQ, dK, dV each carry a guard tail behind their last
    element.  dO sits in the same sentinel-filled layout (NaN wherever the kernels have no business reading), lse, delta, dOt,
    dQ, dK, dV start as NaN and must be finite everywhere afterwards;
  * the padding columns s >= S of V^T, Q^T and K^T hold the largest finite bf16 value in both signs (include/mixgrpo_hip.h:
    any finite value).

The references never come from a kernel."""
import math
import os

import pytest
import torch

import attn_refs as A

pytestmark = pytest.mark.gpu

HD = 128
GUARD = 4096
NAN16 = 0x7FC1                       # a quiet bf16 NaN with a payload bit: the sentinel


def _expected_paths(B, H, S, Sp, ldo, obs):
    """The dispatch rule of csrc/attention.hip / attention_bwd.hip restated (MGX_ATTN_W64 unset)."""
    wide = S % 256 == 0 and Sp == S
    assert S * ldo * 2 < 2 ** 31 and obs * 2 < 2 ** 31 and ldo * 2 < 2 ** 24        # the offset-width limits: not what is probed
    fwd = 0
    if wide:
        nq = S // 256
        grid = min(256, nq * H * B)
        stride = grid // 8 if grid % 8 == 0 else grid
        fwd = int(stride // nq < H)
    return fwd, int(wide)


def _guarded(shape, dtype):
    """A NaN-filled tensor of `shape` with GUARD more NaN elements right behind it: (tensor, guard)."""
    n = math.prod(shape)
    full = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=dtype)
    return full[:n].view(shape), full[n:]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pad_t(x, Sp):
    """[B, H, S, 128] -> the transposed operand [B, H, 128, Sp]; padding columns = +-(largest finite bf16), alternating."""
    B, H, S, _ = x.shape
    t = torch.full((B, H, HD, Sp), A.BF16_MAX, device=x.device, dtype=torch.bfloat16)
    t[..., 1::2] = -A.BF16_MAX
    t[..., :S] = x.transpose(-1, -2)
    return t


class _Layout:
    """O / dO as the kernels address them: [B, S, ldo] rows inside a flat sentinel buffer, the head block at column col0."""

    def __init__(self, B, H, S, ldo_mult, col0, gap):
        self.B, self.H, self.S = B, H, S
        self.ldo = H * HD * ldo_mult
        self.col0 = col0
        self.obs = S * self.ldo + gap
        assert col0 % 8 == 0 and col0 + H * HD <= self.ldo and gap % 8 == 0

    def new(self):
        full = torch.empty(self.B * self.obs + GUARD, device="cuda", dtype=torch.bfloat16)
        _bits(full).fill_(NAN16)
        return full

    def rows(self, full):
        return torch.as_strided(full, (self.B, self.S, self.ldo), (self.obs, self.ldo, 1))

    def block(self, full):
        return self.rows(full)[:, :, self.col0:self.col0 + self.H * HD]

    def heads(self, full):
        """The head block as [B, H, S, 128]."""
        return self.block(full).reshape(self.B, self.S, self.H, HD).permute(0, 2, 1, 3).contiguous()

    def put(self, full, x):
        self.block(full).copy_(x.permute(0, 2, 1, 3).reshape(self.B, self.S, self.H * HD))

    def arg(self, full):
        return full[self.col0:]

    def untouched_outside_block(self, full):
        chk = full.clone()
        _bits(self.block(chk)).fill_(NAN16)
        return bool((_bits(chk) == NAN16).all())


def _run(B, H, S, Sp, family, lay, seed, fails, keep=None):
    """Both forwards and both backwards of one case; appends a line to `fails` for every missed check, prints every figure."""
    from mixgrpo_amd import ops
    q, k, v, do = A.make_inputs(family, B, H, S, seed, device="cuda")
    vt, kt = _pad_t(v, Sp), _pad_t(k, Sp)
    dO = lay.new()
    lay.put(dO, do)
    for kind in ("scale", "log2"):
        qk, sc = (q, A.SCALE) if kind == "scale" else (A.to_log2(q), A.LN2)
        ref, bud = A.reference(qk, k, v, do, sc)

        def check(name, res):
            ok, msg = res
            print(f"  {kind:5s} {name:10s} {'ok  ' if ok else 'FAIL'} {msg}")
            if not ok:
                fails.append(f"{kind} {name}: {msg}")

        # ---- forward
        Ofull = lay.new()
        lse, lse_g = _guarded((B, H, S), torch.float32)
        if kind == "scale":
            ops.attn_fwd(qk, k, vt, lay.arg(Ofull), lse, B, H, S, Sp, lay.ldo, lay.obs, sc)
        else:
            ops.attn_fwd_log2(qk, k, vt, lay.arg(Ofull), lse, B, H, S, Sp, lay.ldo, lay.obs)
        torch.cuda.synchronize()
        O = lay.heads(Ofull)
        check("O", A.rows_close(O, ref["O"], bud["O"], A.C["O"]))
        check("O bits", A.rounded_once(O))
        check("lse", A.lse_close(lse, ref["lse"]))
        check("O outside", (lay.untouched_outside_block(Ofull), "columns outside the head block / batch gap / tail of O changed"))
        check("lse guard", (bool(torch.isnan(lse_g).all()), "the forward wrote behind lse"))

        # ---- backward on this forward's O and lse
        qt = _pad_t(qk, Sp)
        outs = {n: _guarded((B, H, S, HD), torch.bfloat16) for n in ("dQ", "dK", "dV")}
        delta, delta_g = _guarded((B, H, S), torch.float32)
        dOt, dOt_g = _guarded((B, H, HD, Sp), torch.bfloat16)
        ops.attn_bwd(qk, k, v, qt, kt, lay.arg(Ofull), lay.arg(dO), lse, delta, dOt, outs["dQ"][0], outs["dK"][0], outs["dV"][0],
                     B, H, S, Sp, lay.ldo, lay.obs, sc)
        torch.cuda.synchronize()
        check("delta", A.delta_close(delta, do, O))
        check("dOt", A.dot_exact(dOt, do, S))
        for n in ("dQ", "dK", "dV"):
            check(n, A.rows_close(outs[n][0], ref[n], bud[n], A.C[n]))
            check(n + " bits", A.rounded_once(outs[n][0]))
        guards_ok = all(bool(torch.isnan(g_.float()).all()) for g_ in (delta_g, dOt_g, outs["dQ"][1], outs["dK"][1], outs["dV"][1]))
        check("guards", (guards_ok, "the backward wrote behind delta / dOt / dQ / dK / dV"))
        check("inputs", (lay.untouched_outside_block(Ofull) and torch.equal(lay.heads(Ofull), O) and
                         torch.equal(_bits(qt), _bits(_pad_t(qk, Sp))), "the backward changed O or Q^T"))
        if keep is not None:
            keep.append([t.clone() for t in (Ofull, lse, delta, dOt, outs["dQ"][0], outs["dK"][0], outs["dV"][0])])
    return q


def _case(B, H, S, family, layout, fwd_path, bwd_path, Sp=None, seed=None, keep=None):
    from mixgrpo_amd import ops
    Sp = (S + 63) // 64 * 64 if Sp is None else Sp
    lay = {"plain": lambda: _Layout(B, H, S, 1, 0, 0),
           "cat": lambda: _Layout(B, H, S, 5, 2 * H * HD, 0),           # the head block in the middle of a 5 d wide row
           "gap": lambda: _Layout(B, H, S, 5, H * HD + 64, 3 * 5 * H * HD + 8)}[layout]()   # o_bstride > S ldo
    got = (ops.attn_fwd_path(B, H, S, Sp, lay.ldo, lay.obs), ops.attn_bwd_path(B, H, S, Sp, lay.ldo, lay.obs))
    print(f"case B {B} H {H} S {S} Sp {Sp} {family} {layout}: paths fwd {got[0]} bwd {got[1]}")
    assert got == (fwd_path, bwd_path), f"dispatch (fwd, bwd) = {got}, the case is about {(fwd_path, bwd_path)}"
    if os.environ.get("MGX_ATTN_W64", "1") != "0":
        assert got == _expected_paths(B, H, S, Sp, lay.ldo, lay.obs)
    fails = []
    _run(B, H, S, Sp, family, lay, 1000 * B + 10 * H + S if seed is None else seed, fails, keep)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------- the generated 64-wide kernels
# forward shapes of the persistent walk (blocks = B H S / 256, workgroups = min(256, blocks), stride = workgroups / 8 when that
# divides, else workgroups):
#   (2, 4, 512)   16 blocks, stride 2                 (3, 8, 512)   48 blocks, stride 6, nq 2: the head moves by 3 per step
#   (2, 24, 1536) 288 blocks on 256 workgroups: a second block per workgroup for 32 of them, across the batch boundary
#   (7, 24, 768)  504 blocks, ~2 per workgroup        (1, 24, 4608) the full tensor
# backward-only 64-wide shapes (their forward is the 8-wave kernel: the walk cannot take them):
#   (2, 3, 768)   18 workgroups                       (3, 5, 512)   30 workgroups, not a multiple of 8 (xcd_remap's remainder)
FWD64 = [(2, 4, 512), (3, 8, 512), (2, 24, 1536), (7, 24, 768), (1, 24, 4608)]
BWD64_ONLY = [(2, 3, 768), (3, 5, 512)]


@pytest.mark.parametrize("layout", ["plain", "cat"])
@pytest.mark.parametrize("family", ["uniform", "peaked"])
@pytest.mark.parametrize("B,H,S", FWD64)
def test_wide_forward_and_backward(B, H, S, family, layout):
    """attn_fwd64 / attn_fwd64q and the 64-wide dkv / dq pair (paths asserted 1, 1), B > 1, walks that carry into the next
    batch, O inside a 5 d wide row."""
    _case(B, H, S, family, layout, 1, 1)


@pytest.mark.parametrize("layout", ["plain", "cat"])
@pytest.mark.parametrize("family", ["uniform", "peaked"])
@pytest.mark.parametrize("B,H,S", BWD64_ONLY)
def test_wide_backward_behind_the_8_wave_forward(B, H, S, family, layout):
    """Shapes with S % 256 == 0 that the forward's walk cannot take (stride / nq >= H): 8-wave forward, 64-wide backward.
    (2, 3, 768) is one of the two shapes the older "64-query forward" tests ran without reaching that kernel."""
    _case(B, H, S, family, layout, 0, 1)


@pytest.mark.parametrize("B,H,S,family", [(2, 24, 1536, "peaked"), (2, 4, 512, "uniform"), (3, 8, 512, "spike")])
def test_wide_kernels_with_a_gap_between_batches(B, H, S, family):
    """o_bstride > S ldo: the batch offset of O / dO is o_bstride, not S ldo, in the persistent walk's carry and in the backward;
    the gap must come back bit for bit.  Spikes (rows with a one-hot P, the forward's overflow fix-up) at B > 1."""
    _case(B, H, S, family, "gap", 1, 1)


def test_wide_backward_gap_behind_the_8_wave_forward():
    _case(2, 3, 768, "peaked", "gap", 0, 1)


# ------------------------------------------------------------------------------------------------------------- the 8-wave kernels
RAGGED = [1, 31, 33, 63, 64, 65, 257, 320, 1100, 4112, 4672]


@pytest.mark.parametrize("layout", ["plain", "cat"])
@pytest.mark.parametrize("family", ["uniform", "peaked"])
@pytest.mark.parametrize("B,H", [(1, 2), (3, 5)])
@pytest.mark.parametrize("S", RAGGED)
def test_8_wave_kernels_at_ragged_lengths(S, B, H, family, layout):
    """S % 256 != 0 (paths asserted 0, 0): a single key / query tile (S < 32, S < 64: no prefetch), S % 32 in {1, 31} (the per-key
    mask of the dkv kernel), S % 64 == 0 with a partial 256-row block (320, 4672), one row beyond a full block (257), and
    720 x 1280's 4112 = 16 * 256 + 16; 6 and up to 285 workgroups (xcd_remap's remainder)."""
    _case(B, H, S, family, layout, 0, 0)


def test_8_wave_kernels_take_the_single_block_shape():
    """(1, 1, 256): one block, stride 1, 1 / 1 < 1 fails: the 8-wave forward (the other shape the older tests mis-filed); the
    backward has no walk and is 64-wide."""
    _case(1, 1, 256, "peaked", "plain", 0, 1)
    _case(1, 1, 256, "uniform", "cat", 0, 1)


@pytest.mark.parametrize("family", ["uniform", "peaked"])
def test_more_padding_than_needed_leaves_the_wide_kernels(family):
    """S % 256 == 0 with Sp = S + 64: accepted, and every kernel is the 8-wave one (the header says so); 64 padding columns."""
    _case(2, 4, 512, family, "cat", 0, 0, Sp=576)


@pytest.mark.parametrize("S,family", [(1100, "ramp"), (1100, "peaked"), (65, "uniform"), (4112, "peaked")])
def test_8_wave_kernels_with_a_gap_between_batches(S, family):
    """o_bstride > S ldo at ragged lengths, B = 3; the ramp family (keys drifting upwards: the deferred-rescale forward path and
    a backward whose P is recomputed from a large lse)."""
    _case(3, 5, S, family, "gap", 0, 0)


def test_8_wave_kernels_when_the_wide_ones_are_switched_off(monkeypatch):
    """MGX_ATTN_W64=0 is honoured by the queries and the launchers alike: a FLUX-like shape on the 8-wave kernels."""
    monkeypatch.setenv("MGX_ATTN_W64", "0")
    _case(2, 24, 1536, "peaked", "cat", 0, 0)


# ------------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("B,H,S,layout,paths", [(2, 24, 1536, "cat", (1, 1)), (3, 5, 1100, "gap", (0, 0))])
def test_two_launches_give_the_same_bits(B, H, S, layout, paths):
    """attention_bwd.hip: "no atomics, bitwise reproducible" -- O, lse, delta, dOt, dQ, dK, dV of two runs on the same operands,
    on one 64-wide shape and one ragged shape, both scales."""
    runs = []
    for _ in range(2):
        keep = []
        _case(B, H, S, "peaked", layout, *paths, keep=keep)
        runs.append(keep)
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))
