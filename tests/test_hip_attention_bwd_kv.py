"""mgx_attn_bwd_kv on the GPU: the generated 64-wide attention backward with a masked tail (attn_bwd_dq64kv / attn_bwd_dkv64kv,
`kv` of csrc/gen/attn_bwd_dq64.py and attn_bwd_dkv64.py, and the kv_len form of the prep kernel), which serves the autograd of
F.scaled_dot_product_attention (fastvideo/train_grpo_flux.py:134-144) when the sequence is padded to a multiple of 256.
Everything is allocated at Sa; the rows < kv_len of dQ, dK, dV are held to the float64 reference of tests/attn_refs.py taken
on the first kv_len rows of Q2, K, V and dO, per row, at the budgets and constants the unmasked kernels are held to
(attn_refs.C), the rows >= kv_len must be zero, and nothing may depend on what the padding holds.  O and lse come from
mgx_attn_fwd_log2_kv on the same padded operands where its walk takes the shape, else from the float64 reference (bf16 O,
fp32 lse); the backward runs at scale = ln 2 on q2 = to_log2(q), as the model runs it."""
import functools

import pytest
import torch

import attn_refs as A
from test_hip_attention_kernels import NAN16, _bits, _guarded, _Layout
from test_hip_attention_kv import TAILS, _garbage

pytestmark = pytest.mark.gpu

# 16 and 48 workgroups, and 30: not a multiple of 8 (xcd_remap's remainder; the forward's walk cannot take that one)
SHAPES = [(2, 4, 512), (3, 8, 512), (3, 5, 512)]
_ids = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _inputs(shape, family):
    B, H, Sa = shape
    q, k, v, do = A.make_inputs(family, B, H, Sa, 2000 + Sa + H, device="cuda")
    return A.to_log2(q), k, v, do


@functools.lru_cache(maxsize=None)
def _reference(shape, family, kv_len):
    """float64 attention forward and backward over the first kv_len keys and queries; computed once, never written to."""
    q2, k, v, do = (t[:, :, :kv_len] for t in _inputs(shape, family))
    return A.reference(q2, k, v, do, A.LN2)


def _fill(t, kv_len, pad_seed, i, dim=2):
    """The rows (dim 2) or columns (dim 3) >= kv_len of t become zeros (pad_seed None) or garbage of magnitudes to 1e4 and beyond."""
    idx = [slice(None)] * t.dim()
    idx[dim] = slice(kv_len, None)
    n = t[tuple(idx)].shape
    if 0 in n:
        return t
    t[tuple(idx)] = 0 if pad_seed is None else _garbage(n, 20 * pad_seed + i).to(t.dtype)
    return t


def _operands(shape, family, kv_len, pad_seed):
    """(q2, k, v, qt, kt, do) allocated at Sa, every padding row / column filled independently."""
    q2, k, v, do = (t.clone() for t in _inputs(shape, family))
    qt, kt = q2.transpose(-1, -2).contiguous(), k.transpose(-1, -2).contiguous()
    for i, t in enumerate((q2, k, v, do)):
        _fill(t, kv_len, pad_seed, i)
    for i, t in enumerate((qt, kt)):
        _fill(t, kv_len, pad_seed, 4 + i, dim=3)
    return q2, k, v, qt, kt, do


def _forward(shape, family, kv_len, q2, k, v, lay, pad_seed):
    """O (in the layout's sentinel buffer) and lse of the rows < kv_len, the rows >= kv_len filled like every other padding."""
    from mixgrpo_amd import ops
    B, H, Sa = shape
    Ofull = lay.new()
    if ops.attn_fwd_kv_path(B, H, Sa, kv_len, lay.ldo, lay.obs) == 1:
        lse = torch.empty((B, H, Sa), device="cuda", dtype=torch.float32)
        assert ops.attn_fwd_log2_kv(q2, k, v.transpose(-1, -2).contiguous(), lay.arg(Ofull), lse, B, H, Sa, kv_len, lay.ldo, lay.obs)
        O = lay.heads(Ofull)
    else:                                    # the forward's walk cannot take the shape: the reference's O and lse, rounded
        ref, _ = _reference(shape, family, kv_len)
        O = torch.zeros((B, H, Sa, A.HD), device="cuda", dtype=torch.bfloat16)
        lse = torch.zeros((B, H, Sa), device="cuda", dtype=torch.float32)
        O[:, :, :kv_len] = ref["O"].to(torch.bfloat16)
        lse[:, :, :kv_len] = ref["lse"].to(torch.float32)
    lay.put(Ofull, _fill(O, kv_len, pad_seed, 6))
    return Ofull, _fill(lse, kv_len, pad_seed, 7)


def _run(shape, family, kv_len, pad_seed, lay=None, entry="kv"):
    """One backward.  -> dict(dQ, dK, dV, delta, dOt, O [B, H, Sa, 128], do); asserts the path first, then that the guard tails,
    the inputs and everything of O / dO's buffers came back bit for bit and that everything written is finite."""
    from mixgrpo_amd import ops
    B, H, Sa = shape
    lay = lay or _Layout(B, H, Sa, 1, 0, 0)
    q2, k, v, qt, kt, do = _operands(shape, family, kv_len, pad_seed)
    Ofull, lse = _forward(shape, family, kv_len, q2, k, v, lay, pad_seed)
    dOfull = lay.new()
    lay.put(dOfull, do)
    ins = (q2, k, v, qt, kt, Ofull, dOfull, lse)
    before = [t.clone() for t in ins]
    outs = {n: _guarded((B, H, Sa, A.HD), torch.bfloat16) for n in ("dQ", "dK", "dV")}
    outs["delta"] = _guarded((B, H, Sa), torch.float32)
    outs["dOt"] = _guarded((B, H, A.HD, Sa), torch.bfloat16)
    args = (q2, k, v, qt, kt, lay.arg(Ofull), lay.arg(dOfull), lse, outs["delta"][0], outs["dOt"][0], outs["dQ"][0], outs["dK"][0],
            outs["dV"][0], B, H, Sa)
    if entry == "kv":
        assert ops.attn_bwd_kv_path(B, H, Sa, kv_len, lay.ldo, lay.obs) == 1
        assert ops.attn_bwd_kv(*args, kv_len, lay.ldo, lay.obs, A.LN2)
    else:
        assert kv_len == Sa and ops.attn_bwd_path(B, H, Sa, Sa, lay.ldo, lay.obs) == 1
        ops.attn_bwd(*args, Sa, lay.ldo, lay.obs, A.LN2)
    torch.cuda.synchronize()
    for n, (t, guard) in outs.items():
        assert bool(torch.isnan(guard.float()).all()), f"the backward wrote behind {n}"
        assert bool(torch.isfinite(t.float()).all()), f"{n}: not everything was written with finite values"
    for t, t0 in zip(ins, before):
        assert torch.equal(_bits(t), _bits(t0)), "the backward changed one of its inputs (Q, K, V, Q^T, K^T, O, dO, lse)"
    res = {n: t for n, (t, _) in outs.items()}
    res.update(O=lay.heads(Ofull), do=do)
    return res


def _check(res, shape, family, kv_len):
    ref, bud = _reference(shape, family, kv_len)
    fails = []
    for n in ("dQ", "dK", "dV"):
        ok, msg = A.rows_close(res[n][:, :, :kv_len], ref[n], bud[n], A.C[n])
        print(f"  {shape} kv_len {kv_len} {family} {n}: {msg}")
        if not ok:
            fails.append(f"{n}: {msg}")
        ok, msg = A.rounded_once(res[n])
        if not ok:
            fails.append(f"{n} bits: {msg}")
        if not bool((_bits(res[n][:, :, kv_len:]) & 0x7FFF == 0).all()):
            fails.append(f"{n}: rows >= kv_len are not zero")
    for ok, msg in (A.delta_close(res["delta"][:, :, :kv_len], res["do"][:, :, :kv_len], res["O"][:, :, :kv_len]),
                    A.dot_exact(res["dOt"], res["do"][:, :, :kv_len], kv_len)):
        if not ok:
            fails.append(msg)
    if not bool((res["delta"][:, :, kv_len:] == 0).all()):
        fails.append("delta: rows >= kv_len are not zero")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rows_below_kv_len_against_fp64(shape, tail, family):
    """Every row < kv_len of dQ, dK, dV (garbage in every padding row and column, of dO, O and lse too), delta, dOt, the last-bit
    test, zero rows behind kv_len."""
    kv_len = shape[2] - tail
    _check(_run(shape, family, kv_len, pad_seed=1), shape, family, kv_len)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_no_tail_gives_the_bits_of_attn_bwd(shape):
    a = _run(shape, "spike", shape[2], None)
    b = _run(shape, "spike", shape[2], None, entry="plain")
    for n in ("dQ", "dK", "dV", "delta", "dOt"):
        assert torch.equal(_bits(a[n]), _bits(b[n])), n


@pytest.mark.parametrize("family", ["uniform", "spike"])
@pytest.mark.parametrize("tail", [23, 100, 255])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_ids)
def test_result_does_not_depend_on_the_padding(shape, tail, family):
    """Zero padding and two kinds of garbage in the padding rows of Q, K, V, dO, O, lse and the padding columns of Q^T, K^T: the
    same bits in every row < kv_len of dQ, dK, dV, delta and every column < kv_len of dOt."""
    kv_len = shape[2] - tail
    runs = [_run(shape, family, kv_len, ps) for ps in (None, 2, 3)]
    for r in runs[1:]:
        for n in ("dQ", "dK", "dV", "delta"):
            assert torch.equal(_bits(r[n][:, :, :kv_len].contiguous()), _bits(runs[0][n][:, :, :kv_len].contiguous())), n
        assert torch.equal(_bits(r["dOt"]), _bits(runs[0]["dOt"]))


@pytest.mark.parametrize("layout", ["cat", "gap"])
def test_strided_o_and_do(layout):
    """O and dO inside NaN-sentinel buffers, the head block in the middle of a 5 d wide row (the single blocks' operand) and with
    a gap between batches (o_bstride > Sa ldo): nothing outside the head block is read (a NaN would show) or written (`_run`)."""
    B, H, Sa = shape = SHAPES[1]
    kv_len = Sa - 23
    lay = {"cat": _Layout(B, H, Sa, 5, 2 * H * A.HD, 0), "gap": _Layout(B, H, Sa, 5, H * A.HD + 64, 3 * 5 * H * A.HD + 8)}[layout]
    _check(_run(shape, "peaked", kv_len, 4, lay=lay), shape, "peaked", kv_len)


@pytest.mark.parametrize("why", ["Sa % 256", "kv_len <= Sa - 256", "kv_len > Sa", "MGX_ATTN_W64=0"])
def test_refusals_return_1_and_launch_nothing(why, monkeypatch):
    """There is no other kernel behind the entry point: it says 1 (ops: False), the path query 0, every output is untouched.
    (The operands are allocated at the accepted size 512, whatever the refused call claims.)"""
    from mixgrpo_amd import _lib, ops
    B, H, Sa = shape = SHAPES[0]
    q2, k, v, qt, kt, do = _operands(shape, "uniform", Sa, None)
    Sa_arg, kv_len = {"Sa % 256": (Sa - 64, Sa - 100), "kv_len <= Sa - 256": (Sa, Sa - 256), "kv_len > Sa": (Sa, Sa + 1),
                      "MGX_ATTN_W64=0": (Sa, Sa - 23)}[why]
    ldo, obs = H * A.HD, Sa * H * A.HD
    if why == "MGX_ATTN_W64=0":
        assert ops.attn_bwd_kv_path(B, H, Sa_arg, kv_len, ldo, obs) == 1
        monkeypatch.setenv("MGX_ATTN_W64", "0")
    O = do.permute(0, 2, 1, 3).reshape(B, Sa, ldo).contiguous()
    lse = torch.zeros((B, H, Sa), device="cuda", dtype=torch.float32)
    outs = [_guarded(s, dt)[0] for s, dt in (((B, H, Sa), torch.float32), ((B, H, A.HD, Sa), torch.bfloat16)) +
            (((B, H, Sa, A.HD), torch.bfloat16),) * 3]
    assert ops.attn_bwd_kv_path(B, H, Sa_arg, kv_len, ldo, obs) == 0
    rc = _lib.lib().mgx_attn_bwd_kv(*(t.data_ptr() for t in (q2, k, v, qt, kt, O, O, lse, *outs)), B, H, Sa_arg, kv_len, ldo, obs,
                                    A.LN2, ops.stream())
    assert rc == 1
    assert ops.attn_bwd_kv(q2, k, v, qt, kt, O, O, lse, *outs, B, H, Sa_arg, kv_len, ldo, obs, A.LN2) is False
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t.float()).all()) for t in outs)
