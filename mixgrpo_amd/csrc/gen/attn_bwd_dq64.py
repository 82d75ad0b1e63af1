#!/usr/bin/env python3
"""Generator of the hand-placed gfx950 instruction stream of `attn_bwd_dq64_kernel` (mixgrpo_amd/csrc/attention_bwd.hip).

dQ of the joint attention backward (autograd of F.scaled_dot_product_attention at the reference's call site
fastvideo/train_grpo_flux.py:134-144), for S % 256 == 0; the 8-wave kernel of round 1 / 2 stays for other shapes.

Same construction as the forward (the docstring of csrc/gen/attn_fwd64.py: read that first; what the two files emit alike --
the K and V^T tile images, `segment`, the store block -- is in csrc/gen/emit.py): one wave per SIMD, a wave owns 64 queries =
chains a and b of 32, and every K / V / K^T fragment read from LDS feeds both chains.  Per 32-key block j and chain c:
    QK(c, j):  S^T = K Q_c^T (8 MFMAs)  and  dP^T = V dO_c^T (8 MFMAs)         [key on the row, query on the lane]
    SM(c, j):  p = exp2(s c - lse_q log2 e),  ds = p (dp - delta_q)            [4.5 VALU per element, no maximum: lse is known]
    DQ(c, j):  dQ_c^T += K^T dS_c^T (8 MFMAs), dS^T taken from the accumulator registers in place (bf16 pairs)
Block-iteration j = two segments of 24 MFMA gaps:
    segment 1:  MFMA QK(b, j), DQ(b, j-1)      VALU SM(a, j)      LDS K, V (j+1) fragments, each after its last use
    segment 2:  MFMA QK(a, j+1), DQ(a, j)      VALU SM(b, j)      LDS K^T (j) fragments
Registers: dQ_a a[0:63], dQ_b a[64:127], Q_a a[128:159], Q_b a[160:191], dO_a a[192:223], dO_b a[224:255];
           S_a v[4:19], dP_a v[20:35], S_b v[36:51], dP_b v[52:67], dS_a v[68:75], dS_b v[76:83], the block's 8 K fragments
           v[84:115], 8 V fragments v[116:147], 8 K^T fragments v[148:179].
LDS (96 KiB): two slots each of a K window, a V window (64 keys x 128, rows XOR-swizzled like the forward's K tile) and a K^T
tile ([128 d][64 keys], the forward's V^T image), by LDS-DMA.  Barrier interval t = block-iterations 2t, 2t+1: it reads K^T
tile t (keys 64 t ..) and the K / V WINDOW of keys 64 t + 32 .. 64 t + 95 (QK runs one block ahead of DQ); the window's
second half does not exist in the last interval: waves 2, 3, whose DMA pieces it is, skip them.
dQ is scaled by `scale` in the epilogue (dS carries no scale).  Checked on the CPU by tests/test_attn_bwd64_emulated.py.

Masked tail (`kv`, attn_bwd_dq64kv_body.inc, entry point mgx_attn_bwd_kv): the same stream for a sequence that was padded to a
multiple of 256.  Everything is allocated at Sa; keys and queries >= kv_len (Sa - 256 < kv_len <= Sa) are padding that may hold
any finite values.  The loop pays nothing -- its text is the unmasked stream's line for line:
  * trailing key tiles without a valid key are dropped in pairs by the launcher (`kv_operands`: nloop, seq), never below four;
  * the loop runs one trip less and its last pair of intervals is emitted once more behind it.  Every interval OUTSIDE the loop
    (the first, the peeled pair, the last: eight 32-key blocks) carries the mask in its softmax stream: dS of a key >= kv_len
    is replaced by 0 behind `ds = p (dp - delta)`, one v_cmp + one v_cndmask per element (`mask_key`; S register e of a block is
    key 16 (e >> 3) + 8 h + (e & 7), so the threshold is per lane half, v[248:255]).  A SELECT, not a product: whatever the
    padding rows of K and V made of p and dp -- inf, NaN -- is discarded, and 0 x (a finite K^T padding column) adds nothing to
    dQ.  With four tiles walked (Sa = 256, or kv_len within the first 256 keys) these eight blocks are all there is, so no
    further mask block is needed; otherwise the masked keys lie in the last two tiles that remain;
  * a padding QUERY row (the query is on the lane: nothing it holds can reach another row) reads row kv_len - 1 of Q, dO, lse
    and delta instead of its own, so that its accumulators stay finite, and its dQ is multiplied by 0 instead of `scale` in
    the epilogue (v245, v246): rows >= kv_len of dQ are stored as zero.
kv_len = Sa masks nothing and gives the unmasked stream's bits.  Checked on the CPU by tests/test_attn_bwd64kv_emulated.py.
"""
import os
import sys
from collections import namedtuple

import emit
from emit import MFMA, Asm, a, ar, s, sr, spread, v, vr

# ------------------------------------------------------------------------------------------------ register map
DQ_A, DQ_B = 0, 64
QF_A, QF_B = 128, 160
DOF_A, DOF_B = 192, 224
S_A, DP_A, S_B, DP_B = 4, 20, 36, 52
DS_A, DS_B = 68, 76
KFR, VFR, KTF = 84, 116, 148
KA = 180            # 8 K / V fragment read addresses (per k-step)
KTA = 188           # 4 K^T fragment read addresses (key step s = 2 kb + s2 of the tile)
KSRC = 192          # 4 K / V DMA source offsets
KTSRC = 196         # 4 K^T DMA source offsets
T = 200             # 8 temporaries
LSE_A, LSE_B, DL_A, DL_B = 208, 209, 210, 211
X = 212             # v[212:243] scratch (prologue / epilogue)
ROWOFF = 244        # (w * 64 + r) * 256 + h * 16: Q / dQ byte offset of this lane
V_LAST = 247
SCL_A, SCL_B = 245, 246   # kv: `scale`, or 0 in the lanes of a padding query row (the epilogue's multiplier)
TH = 248            # kv: v[248:255] lane thresholds of the eight 32-key blocks outside the loop (mask_key)
V_LAST_KV = 255

sW, sWOFF = 64, 65
sKP, sVP, sKTP = 66, 68, 70      # pairs: DMA base pointers
sLOOP, sROW, sKTT, sTMP = 72, 73, 74, 75
sQ, sK, sV, sKT, sDO, sLSE, sDL, sDQ = 76, 78, 80, 82, 84, 86, 88, 90
sSP2, sLDO2, sCS, sSCALE, sNLOOP, sS = 92, 93, 94, 95, 96, 97
sTP = 98                         # pair: prologue scratch pointer
sKPU, sVPU = 76, 84              # pairs (the Q / dO pointers' registers, free after the prologue): per-wave K / V DMA bases
S_FIRST, S_LAST = 64, 99

K_BASE, V_BASE, KT_BASE = 0, 32768, 65536
SLOT = 16384


Chain = namedtuple("Chain", "name DQ QF DOF S DP DS LSE DL")

CA = Chain("a", DQ_A, QF_A, DOF_A, S_A, DP_A, DS_A, LSE_A, DL_A)
CB = Chain("b", DQ_B, QF_B, DOF_B, S_B, DP_B, DS_B, LSE_B, DL_B)


# ------------------------------------------------------------------------------------------------ building blocks
def mfma_qk(ch, g):
    """gap g of QK: k-step ks = g >> 1; even: S^T (+)= K[ks] Q[ks]; odd: dP^T (+)= V[ks] dO[ks]."""
    ks = g >> 1
    if g & 1:
        d = vr(ch.DP, 16)
        return f"{MFMA} {d}, {vr(VFR + 4 * ks, 4)}, {ar(ch.DOF + 4 * ks, 4)}, {'0' if ks == 0 else d}"
    d = vr(ch.S, 16)
    return f"{MFMA} {d}, {vr(KFR + 4 * ks, 4)}, {ar(ch.QF + 4 * ks, 4)}, {'0' if ks == 0 else d}"


def mfma_dq(ch, n):
    """n = 4 s2 + dt: dQ^T[dt] += K^T fragment (s2, dt) x dS^T[s2]."""
    s2, dt = n >> 2, n & 3
    o = ar(ch.DQ + 16 * dt, 16)
    return f"{MFMA} {o}, {vr(KTF + 4 * n, 4)}, {vr(ch.DS + 4 * s2, 4)}, {o}"


def read_kv(g, slot, hb):
    """Reload, behind gap g of QK (its last use), the fragment that gap g of the NEXT block's QK uses: K or V rows of
    window half hb (0: rows 0..31 of the window, 1: rows 32..63)."""
    ks = g >> 1
    base = V_BASE if (g & 1) else K_BASE
    dst = VFR if (g & 1) else KFR
    return f"ds_read_b128 {vr(dst + 4 * ks, 4)}, {v(KA + ks)} offset:{base + slot * SLOT + hb * 8192}"


def read_kt(n, slot, kb):
    s2, dt = n >> 2, n & 3
    return f"ds_read_b128 {vr(KTF + 4 * n, 4)}, {v(KTA + 2 * kb + s2)} offset:{slot * SLOT + dt * 4096}"   # KT_BASE in the address


def mask_key(ch, e, thr):
    """kv: S / dP register e of a chain is key 16 (e >> 3) + 8 h + (e & 7) of the 32-key block (h = lane half); `thr` (a VGPR)
    holds 8 + (valid keys of the block, 0 .. 32) - 8 h, so the key's dS -- in its dP register -- becomes 0 unless
    8 + 16 (e >> 3) + (e & 7) < thr.  Unsigned on both sides by construction (the 8)."""
    return [f"v_cmp_lt_u32 vcc, {8 + 16 * (e >> 3) + (e & 7)}, {thr}",
            f"v_cndmask_b32 {v(ch.DP + e)}, 0, {v(ch.DP + e)}, vcc"]


def softmax_stream(ch, thr=None):
    """SM(c, j) as a flat, software-pipelined instruction list (72 instructions, 16 of them v_exp_f32).
    kv, outside the loop: thr = the VGPR of the block's lane threshold, dS of the masked keys is replaced by 0 (+ 32)."""
    def t(e):
        return v(T + (e & 7))
    out = []
    for st in range(16 + 3):
        e = st
        if e - 1 >= 0 and e - 1 < 16:
            out.append(f"v_exp_f32 {t(e - 1)}, {t(e - 1)}")
        if e < 16:
            out.append(f"v_fma_f32 {t(e)}, {v(ch.S + e)}, {s(sCS)}, -{v(ch.LSE)}")
            out.append(f"v_sub_f32 {v(ch.DP + e)}, {v(ch.DP + e)}, {v(ch.DL)}")
        if 0 <= e - 2 < 16:
            out.append(f"v_mul_f32 {v(ch.DP + e - 2)}, {t(e - 2)}, {v(ch.DP + e - 2)}")
            if thr is not None:
                out += mask_key(ch, e - 2, thr)
        if 0 <= e - 3 < 16 and ((e - 3) & 1):
            k = (e - 3) >> 1
            out.append(f"v_cvt_pk_bf16_f32 {v(ch.DS + k)}, {v(ch.DP + 2 * k)}, {v(ch.DP + 2 * k + 1)}")
    return out


def dma_piece(kind, p, slot, ptrs=None):
    base = {"k": K_BASE, "v": V_BASE, "kt": KT_BASE}[kind] + slot * SLOT + p * 1024
    src = (KTSRC if kind == "kt" else KSRC) + p
    ptr = {"k": sKPU, "v": sVPU, "kt": sKTP}[kind] if ptrs is None else ptrs[kind]
    return (f"s_add_i32 m0, {s(sWOFF)}, {base}", f"global_load_lds_dwordx4 {v(src)}, {sr(ptr, 2)}")


def block_iteration(A, par, kb, first=False, last=False, dma1=None, dma2=None, thr=None):
    """Block-iteration j = 2 t + kb, t & 1 == par.  K, V (j+1) live in window half kb of slot par; K^T (j) in tile half kb.
    dma1 / dma2: DMA pieces issued inside segment 1 / segment 2.  thr (kv, outside the loop): the block's mask threshold."""
    A.c(f"================ block-iteration parity {par} kb {kb}{' FIRST' if first else ''}{' LAST' if last else ''}"
        f"{' MASKED' if thr else ''}")
    # ---------------- segment 1: QK(b, j), DQ(b, j-1); SM(a, j); K, V (j+1) reloads
    mf = [mfma_qk(CB, g) for g in range(16)] + ([] if first else [mfma_dq(CB, n) for n in range(8)])
    vg = spread(softmax_stream(CA, thr), len(mf))
    lds = {} if last else {g: read_kv(g, par, kb) for g in range(16)}
    dma = {1 + 3 * i: pc for i, pc in enumerate(dma1 or [])}
    A.c("---- segment 1")
    emit.segment(A, mf, vg, lds=lds, dma=dma)
    if first:
        A.e("s_nop 3")                                      # no DQ gaps behind QK(b, 0): its dP is read by the next VALU
    # ---------------- segment 2: QK(a, j+1), DQ(a, j); SM(b, j); K^T (j) reloads
    mf = ([] if last else [mfma_qk(CA, g) for g in range(16)]) + [mfma_dq(CA, n) for n in range(8)]
    vg = spread(softmax_stream(CB, thr), len(mf))
    lds = {n: read_kt(n, par, kb) for n in range(8)}
    waits = {0: "s_waitcnt lgkmcnt(0)", 16: "s_waitcnt lgkmcnt(0)"}
    if last:                                                 # K^T reads, then DQ at once: read first, wait, then the MFMAs
        for n in range(8):
            A.e(read_kt(n, par, kb))
        lds, waits = {}, {0: "s_waitcnt lgkmcnt(0)"}
    dma = {9 + 3 * i: pc for i, pc in enumerate(dma2 or [])}
    A.c("---- segment 2")
    emit.segment(A, mf, vg, lds=lds, dma=dma, waits=waits)


def interval(A, par, first=False, last=False, th=(None, None)):
    """Barrier interval t (t & 1 == par): block-iterations (2t, 2t+1) + the DMA of interval t+1's tiles.
    th (kv, outside the loop): the mask thresholds of its two blocks."""
    nxt = 1 - par
    if last:
        block_iteration(A, par, 0, first=first, thr=th[0])
        block_iteration(A, par, 1, last=True, thr=th[1])
        return
    kt = [dma_piece("kt", p, nxt) for p in range(4)]
    kp = [dma_piece("k", p, nxt) for p in range(4)]
    vp = [dma_piece("v", p, nxt) for p in range(4)]
    A.e(f"s_add_u32 {s(sKTP)}, {s(sKT)}, {s(sKTT)}")
    A.e(f"s_addc_u32 {s(sKTP + 1)}, {s(sKT + 1)}, 0")
    # rows of the next window that lie beyond the sequence (second half of the last window: waves 2, 3) are fetched from 32 rows
    # earlier instead: valid memory, and that half of the window is never read
    A.e(f"s_cmp_ge_u32 {s(sROW)}, {s(sS)}")
    A.e(f"s_cselect_b32 {s(sTMP)}, 8192, 0")
    for dst, src in ((sKPU, sKP), (sVPU, sVP)):
        A.e(f"s_sub_u32 {s(dst)}, {s(src)}, {s(sTMP)}")
        A.e(f"s_subb_u32 {s(dst + 1)}, {s(src + 1)}, 0")
    block_iteration(A, par, 0, first=first, dma1=kp, dma2=kt[:2], thr=th[0])
    block_iteration(A, par, 1, dma1=vp, dma2=kt[2:], thr=th[1])
    A.e(f"s_add_u32 {s(sKTT)}, {s(sKTT)}, 128")                             # next K^T tile: + 64 keys
    A.e(f"s_add_u32 {s(sROW)}, {s(sROW)}, 64")
    A.e(f"s_add_u32 {s(sKP)}, {s(sKP)}, {SLOT}")                            # next window: + 64 rows of 256 bytes
    A.e(f"s_addc_u32 {s(sKP + 1)}, {s(sKP + 1)}, 0")
    A.e(f"s_add_u32 {s(sVP)}, {s(sVP)}, {SLOT}")
    A.e(f"s_addc_u32 {s(sVP + 1)}, {s(sVP + 1)}, 0")
    A.e("s_waitcnt vmcnt(0)")
    A.e("s_barrier")


# ------------------------------------------------------------------------------------------------ prologue / epilogue
def prologue(A, kv=False):
    names = (("q", sQ), ("k", sK), ("v", sV), ("kt", sKT), ("do", sDO), ("lse", sLSE), ("dl", sDL), ("dq", sDQ))
    for nm, reg in names:
        A.e(f"s_mov_b32 {s(reg)}, %[{nm}_lo]")
        A.e(f"s_mov_b32 {s(reg + 1)}, %[{nm}_hi]")
    for dst, nm in ((sSP2, "sp2"), (sLDO2, "ldo2"), (sCS, "cs"), (sSCALE, "scale"), (sNLOOP, "nloop"), (sS, "seq")):
        A.e(f"s_mov_b32 {s(dst)}, %[{nm}]")
    L = emit.lane_decode(A, X, s_wave=sW, s_woff=sWOFF, woff_shift=12)         # v[X : X + 6]: lane, w, r, h, t0, t1, t2
    w, r, h, t1 = L.w, L.r, L.h, L.t1
    x3 = (v(X + 7), v(X + 8), v(X + 9))
    A.c("K / V fragment read addresses (the forward's K image: MFMA row r reads window row pi(r), chunk (2 ks + h) ^ (row & 15))")
    emit.k_image_read_addrs(A, L, KA, x3)
    A.c("K^T fragment read addresses (the forward's V^T image): row d = 32 dt + r, chunk (2 s + h) ^ ((r >> 1) & 7)")
    emit.vt_image_read_addrs(A, L, KTA, x3, KT_BASE)
    A.c("K / V DMA source offsets: piece p of wave w = window rows 16 w + 4 p + (lane >> 4)")
    emit.k_image_dma_offsets(A, L, KSRC, x3)
    A.c("K^T DMA source offsets: piece p of wave w = rows d = 32 w + 8 p + (lane >> 3)")
    emit.vt_image_dma_offsets(A, L, KTSRC, x3, sSP2)
    A.c("this lane's query row w * 64 + r (chain b: + 32): Q / dQ offset, dO offset, lse / delta")
    row = v(X + 10)
    A.e(f"v_lshl_add_u32 {row}, {w}, 6, {r}")
    A.e(f"v_lshlrev_b32 {t1}, 8, {row}")
    A.e(f"v_lshl_add_u32 {v(ROWOFF)}, {h}, 4, {t1}")
    A.e(f"v_add_u32 {v(X + 11)}, 8192, {v(ROWOFF)}")                       # chain b Q offset
    A.e(f"v_mul_lo_u32 {t1}, {row}, {s(sLDO2)}")
    A.e(f"v_lshl_add_u32 {v(X + 12)}, {h}, 4, {t1}")                       # dO offset chain a
    A.e(f"s_lshl_b32 {s(sTMP)}, {s(sLDO2)}, 5")
    A.e(f"v_add_u32 {v(X + 13)}, {s(sTMP)}, {v(X + 12)}")                  # dO offset chain b
    A.e(f"v_lshlrev_b32 {v(X + 14)}, 2, {row}")                            # lse / delta offset
    qa, qb, doa, dob, la, lb = ROWOFF, X + 11, X + 12, X + 13, X + 14, None
    if kv:
        A.c("masked tail: a padding query row reads row %[qlast] (the block's last valid row) of Q / dO / lse / delta instead of")
        A.c("its own and multiplies its dQ by 0; ROWOFF stays the lane's own row (the dQ store)")
        ra, rb, vs, vz = v(X + 15), v(X + 16), v(X + 17), v(X + 18)
        qa, lb = X + 19, X + 20
        A.e(f"v_add_u32 {rb}, 32, {row}")
        A.e(f"v_mov_b32 {vs}, {s(sSCALE)}")
        A.e(f"v_mov_b32 {vz}, 0")
        A.e(f"v_cmp_lt_u32 vcc, %[qlast], {row}")
        A.e(f"v_cndmask_b32 {v(SCL_A)}, {vs}, {vz}, vcc")
        A.e(f"v_cmp_lt_u32 vcc, %[qlast], {rb}")
        A.e(f"v_cndmask_b32 {v(SCL_B)}, {vs}, {vz}, vcc")
        A.e(f"v_min_u32 {ra}, %[qlast], {row}")
        A.e(f"v_min_u32 {rb}, %[qlast], {rb}")
        for rr, qo, do_, lo in ((ra, qa, doa, la), (rb, qb, dob, lb)):
            A.e(f"v_lshlrev_b32 {t1}, 8, {rr}")
            A.e(f"v_lshl_add_u32 {v(qo)}, {h}, 4, {t1}")
            A.e(f"v_mul_lo_u32 {t1}, {rr}, {s(sLDO2)}")
            A.e(f"v_lshl_add_u32 {v(do_)}, {h}, 4, {t1}")
            A.e(f"v_lshlrev_b32 {v(lo)}, 2, {rr}")
        A.c("lane thresholds of the eight 32-key blocks outside the loop: %[kt0], %[kt1] = four bytes each, 8 + the valid keys")
        A.c("(0 .. 32) of the blocks of the first tile and of the last three (mask_key)")
        A.e(f"v_lshlrev_b32 {t1}, 3, {h}")
        for i in range(8):
            A.e(f"s_lshr_b32 {s(sTMP)}, %[kt{i >> 2}], {8 * (i & 3)}")
            A.e(f"s_and_b32 {s(sTMP)}, {s(sTMP)}, 0xff")
            A.e(f"v_sub_u32 {v(TH + i)}, {s(sTMP)}, {t1}")
    A.c("first tiles: K^T tile 0 and the K / V window of keys 32..95 -> slot 0; keys 0..31 (the second half of 'window -1',")
    A.c("the pieces of waves 2 and 3, whose source rows are 32..63 of it) -> slot 1")
    A.e(f"s_mov_b32 {s(sKTT)}, 0")
    A.e(f"s_add_u32 {s(sKTP)}, {s(sKT)}, 0")
    A.e(f"s_addc_u32 {s(sKTP + 1)}, {s(sKT + 1)}, 0")
    for p in range(4):
        emit.lds_dma(A, dma_piece("kt", p, 0))
    A.e(f"s_mov_b32 {s(sKTT)}, 128")
    for ptr, src in ((sKP, sK), (sVP, sV)):
        A.e(f"s_add_u32 {s(ptr)}, {s(src)}, 8192")                          # window 0 starts at key 32
        A.e(f"s_addc_u32 {s(ptr + 1)}, {s(src + 1)}, 0")
    for kind in ("k", "v"):
        for p in range(4):
            emit.lds_dma(A, dma_piece(kind, p, 0, ptrs={"k": sKP, "v": sVP}))
    skip = A.new_label("w01")
    A.e(f"s_cmp_lt_u32 {s(sW)}, 2")
    A.e(f"s_cbranch_scc1 {skip}")
    for ptr, src in ((sKTP, sK), (sTP, sV)):
        A.e(f"s_sub_u32 {s(ptr)}, {s(src)}, 8192")                          # window -1: rows -32..31; only its rows 32..63 are read
        A.e(f"s_subb_u32 {s(ptr + 1)}, {s(src + 1)}, 0")
    for kind in ("k", "v"):
        for p in range(4):
            emit.lds_dma(A, dma_piece(kind, p, 1, ptrs={"k": sKTP, "v": sTP}))
    A.label(skip)
    # this wave's row base of the NEXT window to fetch (window 1 = keys 96..159): rows 16 w .. 16 w + 15 of it
    A.e(f"s_lshl_b32 {s(sROW)}, {s(sW)}, 4")
    A.e(f"s_add_u32 {s(sROW)}, {s(sROW)}, 96")
    A.e(f"s_add_u32 {s(sKP)}, {s(sKP)}, {SLOT}")
    A.e(f"s_addc_u32 {s(sKP + 1)}, {s(sKP + 1)}, 0")
    A.e(f"s_add_u32 {s(sVP)}, {s(sVP)}, {SLOT}")
    A.e(f"s_addc_u32 {s(sVP + 1)}, {s(sVP + 1)}, 0")
    A.c("Q and dO fragments (B operands), lse * log2(e) and delta of this lane's two rows")
    for ch, qoff, dooff in ((CA, qa, doa), (CB, qb, dob)):
        for ks in range(8):
            A.e(f"global_load_dwordx4 {ar(ch.QF + 4 * ks, 4)}, {v(qoff)}, {sr(sQ, 2)} offset:{32 * ks}")
        for ks in range(8):
            A.e(f"global_load_dwordx4 {ar(ch.DOF + 4 * ks, 4)}, {v(dooff)}, {sr(sDO, 2)} offset:{32 * ks}")
    offb = " offset:128" if lb is None else ""
    lb = la if lb is None else lb
    A.e(f"global_load_dword {v(LSE_A)}, {v(la)}, {sr(sLSE, 2)}")
    A.e(f"global_load_dword {v(LSE_B)}, {v(lb)}, {sr(sLSE, 2)}{offb}")
    A.e(f"global_load_dword {v(DL_A)}, {v(la)}, {sr(sDL, 2)}")
    A.e(f"global_load_dword {v(DL_B)}, {v(lb)}, {sr(sDL, 2)}{offb}")
    A.c("dQ = 0")
    for i in range(128):
        A.e(f"v_accvgpr_write_b32 {a(i)}, 0")
    A.e("s_waitcnt vmcnt(0)")
    A.e(f"v_mul_f32 {v(LSE_A)}, 0x3fb8aa3b, {v(LSE_A)}")                   # log2(e)
    A.e(f"v_mul_f32 {v(LSE_B)}, 0x3fb8aa3b, {v(LSE_B)}")
    A.e("s_barrier")
    for g in range(16):                                                     # K, V (block 0): window half 1 of slot 1
        ks = g >> 1
        base = V_BASE if (g & 1) else K_BASE
        dst = VFR if (g & 1) else KFR
        A.e(f"ds_read_b128 {vr(dst + 4 * ks, 4)}, {v(KA + ks)} offset:{base + SLOT + 8192}")
    A.e("s_waitcnt lgkmcnt(0)")
    A.e("s_barrier")                                     # every wave holds K, V (block 0): slot 1 may be refilled
    for g in range(16):
        A.e(mfma_qk(CA, g))
    A.e("s_nop 7")
    A.e("s_nop 7")


def epilogue(A, kv=False):
    A.c("================ tail: DQ(b) of the last block")
    for n in range(8):
        A.e(mfma_dq(CB, n))
    A.e("s_nop 7")
    A.e("s_nop 7")
    A.c("================ epilogue: dQ * scale -> bf16, 16-byte stores (lane halves exchanged pairwise)")
    for ch, addr in ((CA, ROWOFF), (CB, X + 7)):          # X + 7: chain b's rows, 32 further (generate())
        mul = s(sSCALE) if not kv else v(SCL_A if ch is CA else SCL_B)      # kv: 0 in the lanes of a padding query row
        emit.store_acc_bf16(A, ch.DQ, mul, X + 8, X + 24, v(addr), sDQ)


def generate(kv=False):
    A = Asm()
    th = (lambda i: (v(TH + i), v(TH + i + 1))) if kv else (lambda i: (None, None))
    prologue(A, kv)
    A.e(f"v_add_u32 {v(X + 7)}, 8192, {v(ROWOFF)}")     # chain b dQ offset for the epilogue (X + 7 is free from here on)
    interval(A, 0, first=True, th=th(0))
    emit.counted_loop(A, sLOOP, sNLOOP, lambda: interval(A, 1), lambda: interval(A, 0))
    if kv:                                               # the loop runs one trip less: its last pair is peeled
        interval(A, 1, th=th(2))
        interval(A, 0, th=th(4))
    interval(A, 1, last=True, th=th(6))
    epilogue(A, kv)
    return A.text()


def kv_operands(kv_len, qt=0):
    """kv: what the launcher derives from kv_len for the workgroup of q-tile `qt` (in C++: dq64 of csrc/attn_operands.h, which
    the kernel calls and mgx_attn_kv_operands returns -- the tests hold it equal to this; the CPU tests feed the interpreter
    from here): the 64-key tiles walked -- those with a valid key, rounded up to a pair, at least four --, the loop's trips
    (its last pair is peeled), the length the window fetch is clamped at, kt0 / kt1 = four bytes each, lowest first: 8 + the
    valid keys (0 .. 32) of the 32-key blocks of the first tile and of the last three, and the block's last valid query
    row."""
    nt = max(4, ((kv_len + 63) // 64 + 1) & ~1)
    c = lambda j: 8 + min(32, max(0, kv_len - 32 * j))
    pack = lambda js: sum(c(j) << (8 * i) for i, j in enumerate(js))
    return dict(nloop=(nt - 4) // 2, seq=64 * nt, kt0=pack((0, 1, 2 * nt - 6, 2 * nt - 5)),
                kt1=pack((2 * nt - 4, 2 * nt - 3, 2 * nt - 2, 2 * nt - 1)), qlast=min(255, kv_len - 1 - 256 * qt))


HERE = os.path.dirname(os.path.abspath(__file__))
OUT_BODY = os.path.join(HERE, "..", "attn_bwd_dq64_body.inc")
OUT_BODY_KV = os.path.join(HERE, "..", "attn_bwd_dq64kv_body.inc")


def render(kv=False):
    return emit.render("ATTN_BWD_DQ64KV" if kv else "ATTN_BWD_DQ64", __file__, generate(kv),
                       emit.clobbers(V_LAST_KV if kv else V_LAST, S_FIRST, S_LAST))


def write():
    return tuple(emit.write_if_changed(path, render(kv)) for path, kv in ((OUT_BODY, False), (OUT_BODY_KV, True)))


if __name__ == "__main__":
    emit.main(lambda: generate("--kv" in sys.argv), write)
