"""The masked-tail variants of the generated attention BACKWARD streams (attn_bwd_dq64kv_body.inc, attn_bwd_dkv64kv_body.inc,
`kv` of mixgrpo_amd/csrc/gen/attn_bwd_dq64.py and attn_bwd_dkv64.py; entry point mgx_attn_bwd_kv), checked WITHOUT a GPU:
interpreted by tests/asm_emu.py against the fp64 reference of test_attn_bwd64_emulated.py::_problem taken on kv_len rows, plus
the static hazard pass.  Everything is allocated at Sa (% 256 == 0); keys and queries >= kv_len are padding that must
contribute exactly nothing whatever finite values it holds, and rows >= kv_len of dQ / dK / dV are stored as zero.  The
kernels serve the autograd of F.scaled_dot_product_attention (fastvideo/train_grpo_flux.py:134-144) at sequence lengths off
256.  Tolerance: the one of test_attn_bwd64_emulated.py (relative L2 < 4e-3 over the valid rows)."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "mixgrpo_amd", "csrc", "gen"))
import asm_emu  # noqa: E402
import attn_bwd_dkv64 as GK  # noqa: E402
import attn_bwd_dq64 as GQ  # noqa: E402
import attn_fwd64 as GF  # noqa: E402
import test_attn_bwd64_emulated as E  # noqa: E402

# (Sa, block, kv_len): Sa = 256 -- four key tiles / eight query blocks, everything outside the loops --: no mask | last tile /
# block partial | mask on a tile boundary | two tiles masked | only the first tile has valid rows | one valid row;
# Sa = 512, second block: a 256-row block that is partly padding behind a full one, with and without a dropped tile pair
CASES = [(256, 0, kv) for kv in (256, 233, 192, 156, 56, 1)] + [(512, 1, 489), (512, 1, 300)]
# the two interpreter settings of test_attn_bwd64_emulated.py, alternating over the cases (both run on every stream)
MODES = (("late", [0, 1, 2, 3]), ("early", [3, 2, 1, 0]))
PADS = (None, 1, 2)              # zero padding, two seeds of garbage


def _garbage(shape, seed, dtype):
    """Finite padding: unit noise with every fourth element around +-1e4 (bf16 bits or fp32)."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal(shape).astype(np.float32)
    big = rng.random(shape) < 0.25
    x = np.where(big, np.sign(x) * 1e4 * (1 + np.abs(x)), x).astype(np.float32)
    return E._bf16(x) if dtype == np.uint16 else x


@functools.lru_cache(maxsize=None)
def _valid(kv_len, seed):
    """_problem at kv_len rows.  With ONE row the softmax is the constant 1 and the reference's dQ and dK are exactly zero
    (dS = P (dP - delta) = 0), so no relative error exists; the error of such a result is held to the same 4e-3 of the term
    that cancels, scale (P o dP) K resp. scale (P o dP)^T Q, which is what the kernels' roundings are relative to."""
    pr, ref = E._problem(kv_len, seed)
    if kv_len == 1:
        q, k, v_, do = (E._f32(x).astype(np.float64) for x in (pr["Q"], pr["K"], pr["V"], pr["DO"][:, pr["col0"]:pr["col0"] + 128]))
        assert not ref["dQ"].any() and not ref["dK"].any()
        ref = dict(ref, dQ_den=np.linalg.norm((do @ v_.T) @ k * pr["scale"]), dK_den=np.linalg.norm((do @ v_.T).T @ q * pr["scale"]))
    return pr, ref


def _padded(Sa, kv_len, seed, pad):
    """The operands of _problem(kv_len) allocated at Sa rows / columns: the padding is zero (pad None) or garbage, a different
    one in every operand (the transposed operands' padding columns are not the transposes of the padding rows)."""
    pr, ref = _valid(kv_len, seed)
    out = dict(scale=pr["scale"], ldo=pr["ldo"], col0=pr["col0"])
    for i, (nm, axis) in enumerate((("Q", 0), ("K", 0), ("V", 0), ("DO", 0), ("LSE", 0), ("DL", 0), ("KT", 1), ("QT", 1), ("DOT", 1))):
        src = np.ascontiguousarray(pr["DO"][:, pr["col0"]:pr["col0"] + 128].T) if nm == "DOT" else pr[nm]
        shape = list(src.shape)
        shape[axis] = Sa - kv_len
        fill = np.zeros(shape, src.dtype) if pad is None else _garbage(tuple(shape), 16 * pad + i, src.dtype)
        out[nm] = np.ascontiguousarray(np.concatenate([src, fill], axis=axis))
    # what attn_bwd_prep's kv_len form leaves: delta and dO^T of the padding are zero
    out["DL"][kv_len:] = 0
    out["DOT"][:, kv_len:] = 0
    return out, ref


def _scalars(pr):
    return dict(cs=float(np.float32(pr["scale"] * 1.4426950408889634)), scale=float(np.float32(pr["scale"])))


def _emulate_dq(Sa, qt, kv_len, mode, order, pad, seed=0, masked=True):
    """-> (dQ bits of the workgroup's 256 rows, reference rows, machine)."""
    pr, ref = _padded(Sa, kv_len, seed, pad)
    dQ = np.full((Sa, 128), 0x7FC0, np.uint16)                      # NaN sentinel: every row of the block must be written
    ldo = pr["ldo"]
    inputs = dict(tid=np.arange(256).reshape(4, 64), q=("ptr", "Q", qt * 65536), k=("ptr", "K", 0), v=("ptr", "V", 0),
                  kt=("ptr", "KT", 0), do=("ptr", "DO", qt * 256 * ldo * 2 + 2 * pr["col0"]), lse=("ptr", "LSE", qt * 1024),
                  dl=("ptr", "DL", qt * 1024), dq=("ptr", "DQ", qt * 65536), sp2=Sa * 2, ldo2=ldo * 2, **_scalars(pr))
    if masked:
        inputs.update(GQ.kv_operands(kv_len, qt))
    else:
        inputs.update(nloop=(Sa // 64 - 2) // 2, seq=Sa)
    bufs = {k_: pr[k_] for k_ in ("Q", "K", "V", "KT", "DO", "LSE", "DL")}
    bufs["DQ"] = dQ
    m = asm_emu.Machine(GQ.generate(kv=masked), inputs, bufs, lds_bytes=98304, mode=mode, order=order).run()
    sl = slice(qt * 256, qt * 256 + 256)
    assert (np.delete(dQ, np.s_[sl], axis=0) == 0x7FC0).all(), "stores outside this workgroup's dQ block"
    return dQ[sl], (ref["dQ"][sl], ref.get("dQ_den")), m


def _emulate_dkv(Sa, kt, kv_len, mode, order, pad, seed=0, masked=True):
    """-> ((dK bits, dV bits) of the workgroup's 256 rows, (reference rows), machine)."""
    pr, ref = _padded(Sa, kv_len, seed, pad)
    dK, dV = np.full((Sa, 128), 0x7FC0, np.uint16), np.full((Sa, 128), 0x7FC0, np.uint16)
    ldo = pr["ldo"]
    inputs = dict(tid=np.arange(256).reshape(4, 64), q=("ptr", "Q", 0), do=("ptr", "DO", 2 * pr["col0"]), qt=("ptr", "QT", 0),
                  dot=("ptr", "DOT", 0), k=("ptr", "K", kt * 65536), v=("ptr", "V", kt * 65536), lse=("ptr", "LSE", 0),
                  dl=("ptr", "DL", 0), dk=("ptr", "DK", kt * 65536), dv=("ptr", "DV", kt * 65536), sp2=Sa * 2, ldo2=ldo * 2,
                  nis=float(np.float32(-1.0 / pr["scale"])), ldo32=64 * ldo, **_scalars(pr))
    if masked:
        inputs.update(GK.kv_operands(kv_len, kt))
    else:
        NQ = Sa // 32
        inputs.update(nloop=(NQ - 2) // 2, qmax=(NQ - 1) * 8192, cmax=(NQ - 1) * 128)
    bufs = {k_: pr[k_] for k_ in ("Q", "K", "V", "QT", "DO", "LSE", "DL", "DOT")}
    bufs.update(DK=dK, DV=dV)
    m = asm_emu.Machine(GK.generate(kv=masked), inputs, bufs, lds_bytes=GK.LDS_BYTES, mode=mode, order=order).run()
    sl = slice(kt * 256, kt * 256 + 256)
    for arr in (dK, dV):
        assert (np.delete(arr, np.s_[sl], axis=0) == 0x7FC0).all(), "stores outside this workgroup's key block"
    return (dK[sl], dV[sl]), ((ref["dK"][sl], ref.get("dK_den")), (ref["dV"][sl], None)), m


def _check(got, want, n):
    """Rows < n: relative L2 against the fp64 reference (want = (rows, the denominator where theirs is zero: _valid));
    rows >= n: zero bits, sign ignored."""
    want, den = want
    rel = np.linalg.norm(E._f32(got[:n]).astype(np.float64) - want[:n]) / (den or np.linalg.norm(want[:n]))
    assert rel < 4e-3, rel
    assert not (got[n:] & 0x7FFF).any(), "rows >= kv_len must be stored as zero"
    return rel


def _loop(text):
    lines = text.split("\n")
    lo = next(i for i, ln in enumerate(lines) if ln.startswith(".Lloop_"))
    hi = next(i for i, ln in enumerate(lines) if ln.startswith(".Lloopdone_"))
    return lines[lo:hi + 1]


# ------------------------------------------------------------------------------------------------ the text of the streams
def _macro(src, name):
    """The replacement text of `#define name` in src, continuation lines joined."""
    import re
    m = re.search(r"^#define %s[ \t]+((?:.*\\\n)*.*)$" % name, src, flags=re.M)
    assert m, f"#define {name} not found"
    return m.group(1).replace("\\\n", " ")


def test_new_bodies_fit_what_the_kernels_include():
    """The two new bodies are build products (written by build._generate() through the registered generators, not committed):
    attention_bwd.hip includes them by the names the generators write them under and expands the macros they define, and
    every `%[name]` operand of a stream is bound by the operand macro of its kernel's asm statement (the masked streams': the
    unmasked one's operands and the `_KV` extension)."""
    import re
    from mixgrpo_amd.csrc import gen
    assert {"attn_bwd_dq64", "attn_bwd_dkv64"} <= set(gen.GENERATORS)
    src = open(os.path.join(HERE, "..", "mixgrpo_amd", "csrc", "attention_bwd.hip")).read()
    for G, macro, ops in ((GQ, "ATTN_BWD_DQ64KV", "ATTN_BWD_DQ64"), (GK, "ATTN_BWD_DKV64KV", "ATTN_BWD_DKV64")):
        assert f'#include "{os.path.basename(G.OUT_BODY_KV)}"' in src
        text = G.render(kv=True)
        assert f"#define {macro}_BODY" in text and f"#define {macro}_CLOBBERS" in text
        # the statement that expands the masked body takes the _KV operand macro, which extends the unmasked one
        assert re.search(r"asm volatile\(%s_BODY\s*:\s*:\s*%s_KV_OPERANDS\s*:\s*%s_CLOBBERS\)" % (macro, ops, macro), src)
        kv_ops = _macro(src, f"{ops}_KV_OPERANDS")
        assert re.match(r"%s_OPERANDS\s*," % ops, kv_ops)
        bound = set(re.findall(r"\[(\w+)\]", kv_ops)) | set(re.findall(r"\[(\w+)\]", _macro(src, f"{ops}_OPERANDS")))
        assert set(re.findall(r"%\[(\w+)\]", text)) <= bound, set(re.findall(r"%\[(\w+)\]", text)) - bound
        # ... and the unmasked statement binds the unmasked stream's
        assert re.search(r"asm volatile\(%s_BODY\s*:\s*:\s*%s_OPERANDS\s*:\s*%s_CLOBBERS\)" % (ops, ops, ops), src)
        plain = set(re.findall(r"\[(\w+)\]", _macro(src, f"{ops}_OPERANDS")))
        assert set(re.findall(r"%\[(\w+)\]", G.render())) <= plain


def test_existing_bodies_do_not_change_with_the_variants():
    """The five bodies from before the masked backward regenerate byte for byte with the new variants importable."""
    for path, text in ((GQ.OUT_BODY, GQ.render()), (GK.OUT_BODY, GK.render()), (GF.OUT_BODY, GF.render()),
                       (GF.OUT_BODY_Q, GF.render(acc=True)), (GF.OUT_BODY_QK, GF.render(acc=True, kv_tail=True))):
        with open(path) as f:
            assert f.read() == text, path


@pytest.mark.parametrize("G", [GQ, GK], ids=["dq", "dkv"])
def test_static_hazards_clean(G):
    text = G.generate(kv=True)
    assert asm_emu.check_hazards(text) == []
    body = _loop(text)[1:-1]
    assert asm_emu.check_hazards("\n".join(body + body)) == []


@pytest.mark.parametrize("G", [GQ, GK], ids=["dq", "dkv"])
def test_loop_body_is_the_unmasked_streams(G):
    """The steady state pays nothing: between the loop labels the stream is the unmasked one's line for line, no mask
    instruction is in it, and the unmasked stream has none at all."""
    loop = _loop(G.generate(kv=True))
    assert loop == _loop(G.generate())
    assert not any("v_cndmask" in ln or "v_cmp_lt_u32" in ln for ln in loop)
    assert "v_cndmask" in "\n".join(G.generate(kv=True).split("\n")[-2000:])


def test_masks_sit_outside_the_loops():
    """dQ: one compare + one select per dS element, two chains x 16 elements x eight 32-key blocks (first tile + last three).
    dK / dV: two selects per element (S' and dP'), 32 elements x four 32-query blocks (first + last three)."""
    q, k = GQ.generate(kv=True), GK.generate(kv=True)
    assert sum("v_cndmask_b32" in ln and ", 0, " in ln for ln in q.split("\n")) == 2 * 16 * 8
    assert k.count("v_cndmask_b32") == GK.generate().count("v_cndmask_b32") + 2 * 32 * 4 + 4     # + the epilogue's multipliers
    assert q.count("v_mfma_f32_32x32x16_bf16") == GQ.generate().count("v_mfma_f32_32x32x16_bf16") + 2 * 96
    assert k.count("v_mfma_f32_32x32x16_bf16") == GK.generate().count("v_mfma_f32_32x32x16_bf16") + 2 * 64


def test_operands_of_the_launcher():
    """kv_operands of both generators: key tiles / query blocks without a valid row are dropped in pairs, never below four."""
    nt = lambda kv: GQ.kv_operands(kv)["seq"] // 64
    assert [nt(2560 - d) for d in (0, 23, 64, 100, 200, 255)] == [40, 40, 40, 40, 38, 38]
    assert [nt(kv) for kv in (1, 64, 129, 256, 257, 384, 385)] == [4, 4, 4, 4, 6, 6, 8]
    o = GQ.kv_operands(2537, 9)
    assert (o["nloop"], o["qlast"], list(o["kt0"].to_bytes(4, "little")), list(o["kt1"].to_bytes(4, "little"))) == \
        (18, 232, [40, 40, 40, 40], [40, 40, 40, 8 + 9])
    assert GQ.kv_operands(2537, 3)["qlast"] == 255
    nq = lambda kv: GK.kv_operands(kv)["qmax"] // 8192 + 1
    assert [nq(2560 - d) for d in (0, 23, 64, 100, 200, 255)] == [80, 80, 78, 78, 74, 74]
    assert [nq(kv) for kv in (1, 32, 97, 128, 129, 256)] == [4, 4, 4, 4, 6, 8]
    o = GK.kv_operands(2537, 9)
    assert (o["nloop"], o["klast"], o["cmax"], list(o["qk"].to_bytes(4, "little"))) == (38, 232, 79 * 128, [40, 40, 40, 8 + 9])
    o = GK.kv_operands(56, 0)
    assert (o["nloop"], o["klast"], list(o["qk"].to_bytes(4, "little"))) == (0, 55, [40, 8 + 24, 8, 8])


def test_the_kernels_derive_the_same_operands():
    """What attn_bwd_dq64_kernel<true> and attn_bwd_dkv64_kernel<true> are launched with -- dq64 and dkv64 of
    csrc/attn_operands.h, the functions the kernels call, returned by the host query mgx_attn_kv_operands (no GPU needed) --
    is kv_operands for every kv_len up to 1024 and every 256-row block that holds a valid row."""
    import ctypes
    from mixgrpo_amd import _lib
    h = _lib.lib()
    out = (ctypes.c_int * 5)()
    for stream, G, names in ((1, GQ, ("nloop", "seq", "kt0", "kt1", "qlast")), (2, GK, ("nloop", "qmax", "cmax", "qk", "klast"))):
        for kv_len in range(1, 1025):
            for block in range((kv_len + 255) // 256):
                assert h.mgx_attn_kv_operands(stream, kv_len, block, out, 5) == 5
                assert dict(zip(names, out)) == G.kv_operands(kv_len, block), (stream, kv_len, block)


# ------------------------------------------------------------------------------------------------ interpreted
@functools.lru_cache(maxsize=None)
def _runs(kind, case):
    """The stream `kind` on CASES[case] with zero padding and with two seeds of garbage, the interpreter setting alternating
    with the case.  -> [(outputs, references)] per padding."""
    Sa, blk, kv_len = CASES[case]
    emu = _emulate_dq if kind == "dq" else _emulate_dkv
    out = []
    for i, pad in enumerate(PADS):
        mode, order = MODES[(case + i) & 1]
        got, want, m = emu(Sa, blk, kv_len, mode, order, pad, seed=case)
        out.append((got, want, m.mfma_count))
    return out


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"Sa{a}-blk{b}-kv{k}" for a, b, k in CASES])
def test_dq64kv_emulated(case):
    """dQ of the valid rows against fp64 (garbage in every padded row and column), zero rows behind them, and the same bits
    whatever the padding holds."""
    Sa, qt, kv_len = CASES[case]
    n = min(256, kv_len - 256 * qt)
    runs = _runs("dq", case)
    for got, want, mfmas in runs:
        rel = _check(got, want, n)
        assert mfmas == 4 * 48 * GQ.kv_operands(kv_len)["seq"] // 32
    print(f"dq Sa {Sa} kv_len {kv_len}: rel {rel:.3g}")
    for got, _, _ in runs[1:]:
        assert np.array_equal(got[:n], runs[0][0][:n]), "valid rows depend on the padding"


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"Sa{a}-blk{b}-kv{k}" for a, b, k in CASES])
def test_dkv64kv_emulated(case):
    Sa, kt, kv_len = CASES[case]
    n = min(256, kv_len - 256 * kt)
    runs = _runs("dkv", case)
    for got, want, mfmas in runs:
        rels = [_check(g, w, n) for g, w in zip(got, want)]
        assert mfmas == 4 * 64 * (GK.kv_operands(kv_len)["qmax"] // 8192 + 1)
    print(f"dkv Sa {Sa} kv_len {kv_len}: rel dK {rels[0]:.3g} dV {rels[1]:.3g}")
    for got, _, _ in runs[1:]:
        for g, g0 in zip(got, runs[0][0]):
            assert np.array_equal(g[:n], g0[:n]), "valid rows depend on the padding"


@pytest.mark.parametrize("Sa,blk,mode,order", [(256, 0, "late", [0, 1, 2, 3]), (512, 1, "early", [3, 2, 1, 0])])
def test_no_mask_gives_the_unmasked_streams_bits(Sa, blk, mode, order):
    """kv_len = Sa: both masked streams store the bits of the unmasked ones on the same buffers."""
    a, _, _ = _emulate_dq(Sa, blk, Sa, mode, order, None, seed=7)
    b, _, _ = _emulate_dq(Sa, blk, Sa, mode, order, None, seed=7, masked=False)
    assert np.array_equal(a, b)
    a, _, _ = _emulate_dkv(Sa, blk, Sa, mode, order, None, seed=7)
    b, _, _ = _emulate_dkv(Sa, blk, Sa, mode, order, None, seed=7, masked=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
