"""The key-masked variant of the generated attention forward (attn_fwd64qk_body.inc, `kv_tail` of
mixgrpo_amd/csrc/gen/attn_fwd64.py; entry point mgx_attn_fwd_log2_kv), checked WITHOUT a GPU: interpreted by tests/asm_emu.py
against the fp64 reference of tests/attn_refs.py taken on the first kv_len rows of Q2, K and V, plus the static hazard pass.
Everything is allocated at Sa (% 256 == 0); keys >= kv_len must contribute exactly nothing, whatever finite values the padding
holds.  The kernel serves the rollout's F.scaled_dot_product_attention (fastvideo/utils/sampling_utils.py:68-82) at sequence
lengths off 256.  Tolerances: those of test_attn_fwd64_emulated.py (relative L2 of O < 4e-3, lse within 1e-5; 1e-4 where the
rescale fix-up runs)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "mixgrpo_amd", "csrc", "gen"))
import asm_emu  # noqa: E402
import attn_fwd64 as G  # noqa: E402
import attn_refs as R  # noqa: E402

# kv_len as Sa - d: no mask | last tile partial (720 x 720: 2560 - 23) | mask ends on a tile boundary | penultimate tile
# partial, last tile fully masked | a tile pair dropped, then a partial tile | the extreme of the allowed range
TAILS = (0, 23, 64, 100, 200, 255)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(family, Sa, seed):
    """(q2, k, v) bf16 [Sa, 128] of one head, from the seeded families of attn_refs."""
    q, k, v, _ = R.make_inputs(family, 1, 1, Sa, seed)
    return R.to_log2(q)[0, 0], k[0, 0], v[0, 0]


def _garbage(shape, seed):
    """Finite padding: unit noise with every fourth element around +-1e4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    big = torch.rand(shape, generator=g) < 0.25
    return torch.where(big, x.sign() * 1e4 * (1 + x.abs()), x).bfloat16()


def _padded(q2, k, v, kv_len, pad_seed):
    """The operands with their rows >= kv_len replaced: zeros (pad_seed None) or garbage."""
    q2, k, v = q2.clone(), k.clone(), v.clone()
    n = q2.shape[0] - kv_len
    for i, t in enumerate((q2, k, v)):
        t[kv_len:] = 0 if pad_seed is None else _garbage((n, 128), 100 * pad_seed + i)
    return q2, k, v


def _emulate(q2, k, v, kv_len, qt, mode="late", order=(0, 1, 2, 3), masked=True):
    """One workgroup = q-tile `qt` (256 queries) of one head allocated at Sa = len(q2).  -> (O bits [256, 128], lse [256], machine).
    masked=False: the attn_fwd64q stream on the same buffers (kv_len must be Sa)."""
    Sa = q2.shape[0]
    nt = Sa // 64
    Q, K = _bits(q2), _bits(k)
    Vt = np.ascontiguousarray(_bits(v).T)
    O = np.zeros((Sa, 128), np.uint16)
    lse = np.full(Sa, -7.0, np.float32)
    inputs = dict(tid=np.arange(256).reshape(4, 64), q=("ptr", "Q", qt * 256 * 256), k=("ptr", "K", 0), v=("ptr", "V", 0),
                  o=("ptr", "O", qt * 256 * 256), l=("ptr", "L", qt * 1024), sp2=Sa * 2, ldo2=256, cs=float("nan"),
                  nloop=(nt - 2) // 2, kmax=(nt - 1) * 16384, vmax=(nt - 1) * 128, nblk=1, qt0=qt, hh0=0, b0=0, nq=Sa // 256, nh=1,
                  kstep=Sa * 256, ostep=128 * 512, obs=Sa * 256, ob=("ptr", "O", 0), sq=1 % (Sa // 256), dbh=1 // (Sa // 256),
                  qstride=65536, lstride=1024)
    if masked:
        inputs.update(G.kv_operands(kv_len))
    else:
        assert kv_len == Sa
    text = G.generate(acc=True, kv_tail=masked)
    m = asm_emu.Machine(text, inputs, dict(Q=Q, K=K, V=Vt, O=O, L=lse), mode=mode, order=list(order)).run()
    rows = slice(qt * 256, qt * 256 + 256)
    untouched = np.ones(Sa, bool)
    untouched[rows] = False
    assert not O[untouched].any() and (lse[untouched] == -7.0).all(), "stores outside the workgroup's block"
    return O[rows], lse[rows], m


def _errors(O, lse, q2, k, v, kv_len, qt):
    """(relative L2 of O, max |lse - ref|) over the tile's rows < kv_len, against fp64 attention over the first kv_len keys."""
    ref_o, ref_l, _ = R.attention_ref(q2[None, None, :kv_len], k[None, None, :kv_len], v[None, None, :kv_len], R.LN2)
    n = min(256, kv_len - qt * 256)
    assert n > 0
    ro, rl = ref_o[0, 0, qt * 256:qt * 256 + n].numpy(), ref_l[0, 0, qt * 256:qt * 256 + n].numpy()
    got = _f32(O[:n]).astype(np.float64)
    assert np.isfinite(_f32(O)).all() and np.isfinite(lse).all(), "rows >= kv_len must be written with finite values too"
    return np.linalg.norm(got - ro) / np.linalg.norm(ro), np.abs(lse[:n] - rl).max()


def _loop(text):
    lines = text.split("\n")
    lo = next(i for i, ln in enumerate(lines) if ln.startswith(".Lloop_"))
    hi = next(i for i, ln in enumerate(lines) if ln.startswith(".Lloopdone_"))
    return lines[lo:hi + 1]


# ------------------------------------------------------------------------------------------------ the text of the stream
def test_generated_file_is_current():
    with open(G.OUT_BODY_QK) as f:
        assert f.read() == G.render(acc=True, kv_tail=True), "run `python mixgrpo_amd/csrc/gen/attn_fwd64.py` (or mixgrpo_amd.build)"


def test_other_streams_do_not_change_with_the_variant():
    for acc, path in ((False, G.OUT_BODY), (True, G.OUT_BODY_Q)):
        with open(path) as f:
            assert f.read() == G.render(acc=acc)


def test_static_hazards_clean():
    text = G.generate(acc=True, kv_tail=True)
    assert asm_emu.check_hazards(text) == []
    body = _loop(text)[1:-1]
    assert asm_emu.check_hazards("\n".join(body + body)) == []
    assert text.count("v_mfma_f32_32x32x16_bf16") == 256 + 128          # first, loop pair, peeled pair, last


def test_loop_body_is_the_unmasked_streams():
    """The steady state pays nothing: between the loop labels the stream is attn_fwd64q's line for line, and no mask
    instruction (nor the vcc compare it needs) is in it."""
    loop = _loop(G.generate(acc=True, kv_tail=True))
    assert loop == _loop(G.generate(acc=True))
    assert not any("v_cndmask" in ln or "v_cmp_lt_u32" in ln for ln in loop)


def test_masks_sit_in_the_peeled_iterations_only():
    """Two iterations behind the loop carry one compare + one select per score and chain in their MFMA gaps; the first tile and
    the third from the end carry a branched-around block each (partial only at Sa = 256)."""
    text = G.generate(acc=True, kv_tail=True)
    assert text.count("v_cndmask_b32") == 4 * 64 and "v_cndmask" not in G.generate(acc=True)
    after = text.split("\n")
    after = after[next(i for i, ln in enumerate(after) if ln.startswith(".Lloopdone_")):]
    assert sum("v_cndmask_b32" in ln for ln in after) == 3 * 64


def test_operands_of_the_launcher():
    """kv_operands: tiles without a valid key are dropped in pairs, never below four."""
    nt = lambda kv: G.kv_operands(kv)["kmax"] // 16384 + 1
    assert [nt(2560 - d) for d in TAILS] == [40, 40, 40, 40, 38, 38]
    assert [nt(kv) for kv in (1, 64, 129, 256, 257, 384, 385)] == [4, 4, 4, 4, 6, 6, 8]
    o = G.kv_operands(2537)
    assert (o["nloop"], list(o["kt"].to_bytes(4, "little"))) == (18, [72, 72, 72, 8 + 41])
    o = G.kv_operands(100)
    assert (o["nloop"], list(o["kt"].to_bytes(4, "little"))) == (0, [72, 8 + 36, 8, 8])


def test_the_kernel_derives_the_same_operands():
    """What attn_fwd64_kernel<true, true> is launched with -- fwd64 of csrc/attn_operands.h, the function the kernel calls,
    returned by the host query mgx_attn_kv_operands (no GPU needed) -- is kv_operands for every kv_len up to 1024."""
    import ctypes
    from mixgrpo_amd import _lib
    h = _lib.lib()
    names = ("nloop", "kmax", "vmax", "kt", "kvm1")
    out = (ctypes.c_int * 5)()
    for kv_len in range(1, 1025):
        assert h.mgx_attn_kv_operands(0, kv_len, 0, out, 5) == 5
        assert dict(zip(names, out)) == G.kv_operands(kv_len), kv_len
    for bad in ((3, 100, 0, out, 5), (-1, 100, 0, out, 5), (0, 0, 0, out, 5), (0, 100, 0, out, 4), (0, 100, 0, None, 5)):
        assert h.mgx_attn_kv_operands(*bad) == -1, bad


# ------------------------------------------------------------------------------------------------ interpreted
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("Sa,qt,mode,order", [(512, 1, "late", (0, 1, 2, 3)), (768, 2, "early", (3, 1, 2, 0))])
def test_emulated_vs_reference(Sa, qt, mode, order, tail):
    """The q-tile that holds the boundary between valid and padded queries, garbage in every padded row and column."""
    kv_len = Sa - tail
    q2, k, v = _padded(*_inputs("uniform", Sa, 11), kv_len, pad_seed=1)
    O, lse, m = _emulate(q2, k, v, kv_len, qt, mode, order)
    rel, lerr = _errors(O, lse, q2, k, v, kv_len, qt)
    print(f"Sa {Sa} kv_len {kv_len}: rel {rel:.3g} lse {lerr:.3g}")
    assert rel < 4e-3 and lerr < 1e-5
    assert m.mfma_count == 4 * 64 * (G.kv_operands(kv_len)["kmax"] // 16384 + 1)
    assert not any(k_.startswith(".Lfix") for k_ in m.branches_taken)   # the garbage query rows are never read ...
    n = kv_len - qt * 256
    if n < 256:                              # ... their O and lse are those of the last valid row
        assert (O[n:] == O[n - 1]).all() and (lse[n:].view(np.uint32) == lse[n - 1:n].view(np.uint32)).all()
    if tail == 0:                            # no mask: the bits of the emulated attn_fwd64q
        O0, lse0, _ = _emulate(q2, k, v, kv_len, qt, mode, order, masked=False)
        assert np.array_equal(O, O0) and np.array_equal(lse.view(np.uint32), lse0.view(np.uint32))


@pytest.mark.parametrize("tail", [23, 200])
def test_emulated_first_query_tile(tail):
    """A q-tile of valid queries only (every row is checked)."""
    Sa, kv_len = 512, 512 - tail
    q2, k, v = _padded(*_inputs("peaked", Sa, 12), kv_len, pad_seed=2)
    O, lse, _ = _emulate(q2, k, v, kv_len, 0, "early", (2, 0, 3, 1))
    rel, lerr = _errors(O, lse, q2, k, v, kv_len, 0)
    assert rel < 4e-3 and lerr < 1e-5


@pytest.mark.parametrize("tail", [23, 100, 255])
def test_emulated_result_does_not_depend_on_the_padding(tail):
    """Different finite garbage (magnitudes to 1e4 and beyond) in the K pad rows, the V^T pad columns and the Q pad rows: O and
    lse of the rows < kv_len are the same bits."""
    Sa, kv_len, qt = 512, 512 - tail, 1
    runs = [_emulate(*_padded(*_inputs("uniform", Sa, 13), kv_len, pad_seed=ps), kv_len, qt)[:2] for ps in (None, 3, 4)]
    n = kv_len - qt * 256
    for O, lse in runs[1:]:
        assert np.array_equal(O[:n], runs[0][0][:n])
        assert np.array_equal(lse[:n].view(np.uint32), runs[0][1][:n].view(np.uint32))


@pytest.mark.parametrize("tail", [23, 100])
def test_emulated_rescale_fixup_in_a_masked_tile(tail):
    """The spike family with one more spike in the LAST VALID key, which lies in a partially masked tile: that tile's row sum
    overflows 2^40, its out-of-line fix-up takes the new maximum from score registers that already hold -inf for the masked
    keys, and the result is still right."""
    Sa, kv_len, qt = 512, 512 - tail, 0
    q2, k, v = (t.clone() for t in _inputs("spike", Sa, 14))
    k[kv_len - 1] = (8.0 * q2[40].float() / (R.LOG2E * R.SCALE)).bfloat16()
    q2, k, v = _padded(q2, k, v, kv_len, pad_seed=5)
    O, lse, m = _emulate(q2, k, v, kv_len, qt)
    text = G.generate(acc=True, kv_tail=True).split("\n")
    # the fix-ups branched to from the two iterations whose softmax carries the masks in its gaps (the last two of the walk)
    gap_masked = [i for i, ln in enumerate(text) if "MASKED" in ln][-2]
    assert gap_masked > next(i for i, ln in enumerate(text) if ln.startswith(".Lloopdone_"))
    labels = {ln.split()[-1].replace("%=", "0") for ln in text[gap_masked:] if "s_cbranch_vccnz" in ln}
    assert len(labels) == 4
    assert labels & set(m.branches_taken), "the spike in the last valid key did not force the fix-up of a masked tile"
    rel, lerr = _errors(O, lse, q2, k, v, kv_len, qt)
    assert rel < 4e-3 and lerr < 1e-4


@pytest.mark.parametrize("kv_len", [1, 30, 64, 100, 129, 200, 256])
def test_emulated_shortest_allocation(kv_len):
    """Sa = 256: four tiles, nothing dropped, the loop does not run; below 64 / 128 valid keys the first tile / the third tile
    from the end are partial too and take their branched-around mask blocks."""
    Sa = 256
    q2, k, v = _padded(*_inputs("uniform", Sa, 15), kv_len, pad_seed=6)
    O, lse, m = _emulate(q2, k, v, kv_len, 0)
    rel, lerr = _errors(O, lse, q2, k, v, kv_len, 0)
    assert rel < 4e-3 and lerr < 1e-5
    assert m.mfma_count == 4 * 4 * 64


def test_emulated_walk_over_blocks_redirects_the_padding_queries_per_block():
    """One workgroup walking four blocks of a [H = 2, Sa = 512] problem, (head 0, q-tile 0) (0, 1) (1, 0) (1, 1): the Q fragments
    of the next block are fetched during the current block's last iteration, with the offsets of ITS q-tile -- rows >= kv_len
    (q-tile 1 only) read row kv_len - 1, q-tile 0 reads its own rows again afterwards."""
    Sa, H, kv_len = 512, 2, 512 - 100
    heads = [_padded(*_inputs("uniform", Sa, 20 + h), kv_len, pad_seed=7 + h) for h in range(H)]
    Q, K = (np.stack([_bits(t[i]) for t in heads]) for i in (0, 1))
    Vt = np.stack([np.ascontiguousarray(_bits(t[2]).T) for t in heads])
    ldo = H * 128
    O = np.zeros((Sa, ldo), np.uint16)
    lse = np.full((H, Sa), -7.0, np.float32)
    nt = Sa // 64
    inputs = dict(tid=np.arange(256).reshape(4, 64), q=("ptr", "Q", 0), k=("ptr", "K", 0), v=("ptr", "V", 0), o=("ptr", "O", 0),
                  l=("ptr", "L", 0), sp2=Sa * 2, ldo2=ldo * 2, cs=float("nan"), nblk=4, qt0=0, hh0=0, b0=0, nq=2, nh=H,
                  kstep=Sa * 256, ostep=ldo * 512, obs=Sa * ldo * 2, ob=("ptr", "O", 0), sq=1, dbh=0, qstride=65536, lstride=1024,
                  **G.kv_operands(kv_len))
    asm_emu.Machine(G.generate(acc=True, kv_tail=True), inputs, dict(Q=Q, K=K, V=Vt, O=O, L=lse), mode="late",
                    order=[1, 0, 3, 2]).run()
    for h, (q2, k, v) in enumerate(heads):
        for qt in range(2):
            rows = slice(qt * 256, qt * 256 + 256)
            rel, lerr = _errors(O[rows, h * 128:h * 128 + 128], lse[h, rows], q2, k, v, kv_len, qt)
            assert rel < 4e-3 and lerr < 1e-5, (h, qt, rel, lerr)
        assert (O[kv_len:, h * 128:h * 128 + 128] == O[kv_len - 1, h * 128:h * 128 + 128]).all()
