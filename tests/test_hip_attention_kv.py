"""mgx_attn_fwd_log2_kv on the GPU: the 64-query attention forward with a masked key tail (attn_fwd64qk, csrc/gen/attn_fwd64.py
`kv_tail`), which serves the rollout's F.scaled_dot_product_attention (fastvideo/utils/sampling_utils.py:68-82) when the
sequence is padded to a multiple of 256.  Everything is allocated at Sa; the rows < kv_len of O and lse are held to the
float64 reference of tests/attn_refs.py taken on the first kv_len rows of Q2, K and V, per row, at the budgets and constants
the unmasked kernels are held to (attn_refs.C["O"], lse_close).  Shapes: the smallest of the existing FWD64_PATH table on which
the 64-query walk applies."""
import functools

import pytest
import torch

import attn_refs as A
from test_hip_attention_kernels import NAN16, _bits, _guarded, _Layout
from test_hip_attention_log2 import FWD64_PATH

pytestmark = pytest.mark.gpu

# two shapes the walk takes (path 1) at S = 512 / 768; the table has none at 768, so both are its S = 512 entries
SHAPES = sorted((s for s, path in FWD64_PATH.items() if path == 1 and s[2] in (512, 768)), key=lambda s: (s[2], s[0] * s[1]))[:2]
if not SHAPES:
    SHAPES = sorted((s for s, path in FWD64_PATH.items() if path == 1), key=lambda s: (s[2], s[0] * s[1]))[:1]
# kv_len = Sa - d: no mask | last tile partial (720 x 720) | mask ends on a tile boundary | penultimate tile partial, last tile
# fully masked | a tile pair dropped, then a partial tile | the extreme of the allowed range
TAILS = (0, 23, 64, 100, 200, 255)


@functools.lru_cache(maxsize=None)
def _inputs(shape, family):
    B, H, Sa = shape
    q, k, v, _ = A.make_inputs(family, B, H, Sa, 1000 + Sa + H, device="cuda")
    return A.to_log2(q), k, v


@functools.lru_cache(maxsize=None)
def _reference(shape, family, kv_len):
    """float64 attention over the first kv_len keys, for the first kv_len queries; computed once, never written to."""
    q2, k, v = _inputs(shape, family)
    return A.reference(q2[:, :, :kv_len], k[:, :, :kv_len], v[:, :, :kv_len], None, A.LN2)


def _garbage(shape, seed):
    """Finite padding: unit noise, every fourth element around +-1e4."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, generator=g, device="cuda")
    big = torch.rand(shape, generator=g, device="cuda") < 0.25
    return torch.where(big, x.sign() * 1e4 * (1 + x.abs()), x).bfloat16()


def _operands(shape, family, kv_len, pad_seed):
    """(Q2, K, Vt) allocated at Sa with the rows / columns >= kv_len replaced by zeros (pad_seed None) or garbage."""
    q2, k, v = (t.clone() for t in _inputs(shape, family))
    B, H, Sa = shape
    for i, t in enumerate((q2, k, v)):
        t[:, :, kv_len:] = 0 if pad_seed is None else _garbage((B, H, Sa - kv_len, A.HD), 10 * pad_seed + i)
    return q2, k, v.transpose(-1, -2).contiguous()


def _run(shape, kv_len, q2, k, vt, lay=None):
    """-> (O [B, H, Sa, 128], lse [B, H, Sa]); asserts the path first, and that nothing outside O's head block or behind lse
    was written."""
    from mixgrpo_amd import ops
    B, H, Sa = shape
    lay = lay or _Layout(B, H, Sa, 1, 0, 0)
    assert ops.attn_fwd_kv_path(B, H, Sa, kv_len, lay.ldo, lay.obs) == 1
    Ofull = lay.new()
    lse, lse_g = _guarded((B, H, Sa), torch.float32)
    assert ops.attn_fwd_log2_kv(q2, k, vt, lay.arg(Ofull), lse, B, H, Sa, kv_len, lay.ldo, lay.obs)
    torch.cuda.synchronize()
    assert lay.untouched_outside_block(Ofull), "columns outside the head block / batch gap / rows behind Sa of O changed"
    assert bool(torch.isnan(lse_g).all()), "the forward wrote behind lse"
    return lay.heads(Ofull), lse


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_below_kv_len_against_fp64(shape, tail, family):
    kv_len = shape[2] - tail
    O, lse = _run(shape, kv_len, *_operands(shape, family, kv_len, pad_seed=1))
    ref, bud = _reference(shape, family, kv_len)
    ok_o, msg_o = A.rows_close(O[:, :, :kv_len], ref["O"], bud["O"], A.C["O"])
    ok_l, msg_l = A.lse_close(lse[:, :, :kv_len], ref["lse"])
    print(f"{shape} kv_len {kv_len} {family}: O {msg_o}; lse {'ok' if ok_l else msg_l}")
    assert ok_o, msg_o
    assert ok_l, msg_l
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all(), "rows >= kv_len must be written with finite values"
    if tail:                                 # (they are copies of the last valid row: the padding rows of Q are never read)
        assert torch.equal(_bits(O[:, :, kv_len:]), _bits(O[:, :, kv_len - 1:kv_len].expand(-1, -1, tail, -1)))


def test_workgroups_that_walk_several_blocks():
    """More blocks than the 256 workgroups of a launch (6 x 24 heads x 2 q-tiles = 288): some workgroups go on to a second block,
    whose Q fragments -- with the padding queries of ITS q-tile redirected -- are fetched during the first block's last tile."""
    shape = (6, 24, 512)
    kv_len = 512 - 23
    O, lse = _run(shape, kv_len, *_operands(shape, "uniform", kv_len, pad_seed=5))
    ref, bud = _reference(shape, "uniform", kv_len)
    A.assert_ok(A.rows_close(O[:, :, :kv_len], ref["O"], bud["O"], A.C["O"]))
    A.assert_ok(A.lse_close(lse[:, :, :kv_len], ref["lse"]))
    assert torch.equal(_bits(O[:, :, kv_len:]), _bits(O[:, :, kv_len - 1:kv_len].expand(-1, -1, 23, -1)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_tail_gives_the_bits_of_attn_fwd_log2(shape):
    from mixgrpo_amd import ops
    B, H, Sa = shape
    q2, k, vt = _operands(shape, "spike", Sa, None)
    O, lse = _run(shape, Sa, q2, k, vt)
    lay = _Layout(B, H, Sa, 1, 0, 0)
    assert ops.attn_fwd_path(B, H, Sa, Sa, lay.ldo, lay.obs) == 1
    O0 = lay.new()
    lse0 = torch.empty_like(lse)
    ops.attn_fwd_log2(q2, k, vt, lay.arg(O0), lse0, B, H, Sa, Sa, lay.ldo, lay.obs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(O), _bits(lay.heads(O0))) and torch.equal(_bits(lse), _bits(lse0))


@pytest.mark.parametrize("family", ["uniform", "spike"])
@pytest.mark.parametrize("tail", [23, 100, 255])
def test_result_does_not_depend_on_the_padding(tail, family):
    """Zero padding and two kinds of garbage (K pad rows, V^T pad columns, Q pad rows; magnitudes to 1e4 and beyond): the same
    bits in every row < kv_len of O and lse."""
    shape = SHAPES[0]
    kv_len = shape[2] - tail
    runs = [_run(shape, kv_len, *_operands(shape, family, kv_len, ps)) for ps in (None, 2, 3)]
    for O, lse in runs[1:]:
        assert torch.equal(_bits(O[:, :, :kv_len]), _bits(runs[0][0][:, :, :kv_len]))
        assert torch.equal(_bits(lse[:, :, :kv_len].contiguous()), _bits(runs[0][1][:, :, :kv_len].contiguous()))


@pytest.mark.parametrize("layout", ["cat", "gap"])
def test_stores_stay_inside_the_head_block(layout):
    """O inside a NaN-sentinel buffer, the head block in the middle of a 5 d wide row (the single blocks' operand) and with a gap
    between batches (o_bstride > Sa ldo): the columns outside the head block, the gap behind row Sa of every batch and the
    tail come back bit for bit (checked by `_run`), and the block itself is right."""
    B, H, Sa = shape = SHAPES[-1]
    kv_len = Sa - 23
    lay = {"cat": _Layout(B, H, Sa, 5, 2 * H * A.HD, 0), "gap": _Layout(B, H, Sa, 5, H * A.HD + 64, 3 * 5 * H * A.HD + 8)}[layout]
    O, lse = _run(shape, kv_len, *_operands(shape, "peaked", kv_len, 4), lay=lay)
    ref, bud = _reference(shape, "peaked", kv_len)
    A.assert_ok(A.rows_close(O[:, :, :kv_len], ref["O"], bud["O"], A.C["O"]))
    A.assert_ok(A.lse_close(lse[:, :, :kv_len], ref["lse"]))


@pytest.mark.parametrize("why", ["Sa % 256", "kv_len <= Sa - 256", "kv_len > Sa", "MGX_ATTN_W64=0"])
def test_refusals_return_1_and_launch_nothing(why, monkeypatch):
    """The caller keeps its unpadded path: the entry point says 1 (ops: False), the path query 0, O and lse are untouched.
    (The operands are allocated at the accepted size 512 or larger than what is passed, whatever the refused call claims.)"""
    from mixgrpo_amd import _lib, ops
    B, H, Sa = SHAPES[0]
    q2, k, vt = _operands((B, H, Sa), "uniform", Sa, None)
    Sa_arg, kv_len = {"Sa % 256": (Sa - 64, Sa - 100), "kv_len <= Sa - 256": (Sa, Sa - 256), "kv_len > Sa": (Sa, Sa + 1),
                      "MGX_ATTN_W64=0": (Sa, Sa - 23)}[why]
    if why == "MGX_ATTN_W64=0":
        assert ops.attn_fwd_kv_path(B, H, Sa_arg, kv_len, H * A.HD, Sa * H * A.HD) == 1
        monkeypatch.setenv("MGX_ATTN_W64", "0")
    lay = _Layout(B, H, Sa, 1, 0, 0)
    Ofull = lay.new()
    lse, lse_g = _guarded((B, H, Sa), torch.float32)
    assert ops.attn_fwd_kv_path(B, H, Sa_arg, kv_len, lay.ldo, lay.obs) == 0
    rc = _lib.lib().mgx_attn_fwd_log2_kv(q2.data_ptr(), k.data_ptr(), vt.data_ptr(), lay.arg(Ofull).data_ptr(), lse.data_ptr(), B, H,
                                         Sa_arg, kv_len, lay.ldo, lay.obs, ops.stream())
    assert rc == 1
    assert ops.attn_fwd_log2_kv(q2, k, vt, lay.arg(Ofull), lse, B, H, Sa_arg, kv_len, lay.ldo, lay.obs) is False
    torch.cuda.synchronize()
    assert bool((_bits(Ofull) == NAN16).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(lse_g).all())
