"""What the generators of the 64-wide attention instruction streams share (attn_fwd64.py, attn_bwd_dq64.py, attn_bwd_dkv64.py).

A generator holds what is specific to its kernel -- design, register map, MFMA / VALU streams, schedule -- and builds its text
from the emitters here, each of which exists once: register names and the line buffer `Asm`; the counted loop; the lane
decode and the tile images' address set-ups; the LDS-DMA idiom and the MFMA-gap `segment`; the accumulator -> bf16 store
block; `render` (stream -> the C macros of a *_body.inc) and the command line.  Nothing here knows a register map: every
register and operand is an argument, so an emitter reproduces each of its users' streams exactly (the unmasked and the
forward's .inc files are committed, the backward's two masked-tail bodies are written by the build only; CPU tests interpret
the generators' text).  Plain module, no imports from the package: the generators run as scripts.
"""
import os
import sys
from collections import namedtuple

MFMA = "v_mfma_f32_32x32x16_bf16"


# ------------------------------------------------------------------------------------------------ names, line buffer
def v(i):
    return f"v{i}"


def vr(i, n):
    return f"v[{i}:{i + n - 1}]"


def a(i):
    return f"a{i}"


def ar(i, n):
    return f"a[{i}:{i + n - 1}]"


def s(i):
    return f"s{i}"


def sr(i, n):
    return f"s[{i}:{i + n - 1}]"


class Asm:
    def __init__(self):
        self.lines = []
        self.nlabel = 0

    def e(self, text):
        self.lines.append("  " + text)

    def c(self, text):
        self.lines.append("  ; " + text)

    def label(self, name):
        self.lines.append(f"{name}:")

    def new_label(self, stem):
        """Labels carry a running number: the order in which they are asked for is part of the output."""
        self.nlabel += 1
        return f".L{stem}_{self.nlabel}_%="

    def text(self):
        return "\n".join(self.lines) + "\n"


def spread(items, ngaps):
    """Distribute a flat list over ngaps gaps as evenly as possible, keeping the order."""
    out, n = [], len(items)
    for g in range(ngaps):
        out.append(items[g * n // ngaps:(g + 1) * n // ngaps])
    return out


# ------------------------------------------------------------------------------------------------ control flow
def counted_loop(A, counter, count, body_a, body_b):
    """`count` (an SGPR, may be 0) trips of body_a() body_b(): the loops are unrolled by two (slot parity)."""
    A.e(f"s_mov_b32 {s(counter)}, {s(count)}")
    loop, done = A.new_label("loop"), A.new_label("loopdone")
    A.e(f"s_cmp_eq_u32 {s(counter)}, 0")
    A.e(f"s_cbranch_scc1 {done}")
    A.label(loop)
    body_a()
    body_b()
    A.e(f"s_sub_u32 {s(counter)}, {s(counter)}, 1")
    A.e(f"s_cmp_lg_u32 {s(counter)}, 0")
    A.e(f"s_cbranch_scc1 {loop}")
    A.label(done)


# ------------------------------------------------------------------------------------------------ lane decode, tile images
# lane, wave, MFMA row r = lane & 31, lane half h = lane >> 5, and three temporaries: VGPR names
Lane = namedtuple("Lane", "lane w r h t0 t1 t2")


def lane_decode(A, x, s_wave=None, s_woff=None, woff_shift=None):
    """v[x : x + 6] become a `Lane`; with s_wave: the wave id and its LDS-DMA offset (wave << woff_shift) in SGPRs."""
    L = Lane(*(v(x + i) for i in range(7)))
    A.e(f"v_and_b32 {L.lane}, 63, %[tid]")
    A.e(f"v_lshrrev_b32 {L.w}, 6, %[tid]")
    A.e(f"v_and_b32 {L.r}, 31, {L.lane}")
    A.e(f"v_lshrrev_b32 {L.h}, 5, {L.lane}")
    if s_wave is not None:
        A.e(f"v_readfirstlane_b32 {s(s_wave)}, {L.w}")
        A.e(f"s_lshl_b32 {s(s_woff)}, {s(s_wave)}, {woff_shift}")
    return L


def row_permutation(A, L, pi, xk, pi8):
    """MFMA row r reads row pi(r) = r with bits 2 and 3 exchanged of a tile of 256-byte rows whose 16-byte chunks are
    XOR-swizzled by row & 15: pi, xk = h ^ (pi & 15) (bit 0 of the lane's chunk index, swizzled), pi8 = the row's byte offset."""
    A.e(f"v_and_b32 {L.t0}, 0x13, {L.r}")
    A.e(f"v_and_b32 {L.t1}, 4, {L.r}")
    A.e(f"v_lshlrev_b32 {L.t1}, 1, {L.t1}")
    A.e(f"v_and_b32 {L.t2}, 8, {L.r}")
    A.e(f"v_lshrrev_b32 {L.t2}, 1, {L.t2}")
    A.e(f"v_or3_b32 {pi}, {L.t0}, {L.t1}, {L.t2}")
    A.e(f"v_and_b32 {L.t0}, 15, {pi}")
    A.e(f"v_xor_b32 {xk}, {L.h}, {L.t0}")
    A.e(f"v_lshlrev_b32 {pi8}, 8, {pi}")


def k_image_read_addrs(A, L, dst, scratch):
    """K image ([64 rows][128] bf16, the forward's K tile and dQ's K / V windows): v[dst + ks] = fragment read address of
    k-step ks = row pi(r), chunk (2 ks + h) ^ (row & 15).  The LDS base goes into the ds_read's offset."""
    pi, xk, pi8 = scratch
    row_permutation(A, L, pi, xk, pi8)
    for ks in range(8):
        A.e(f"v_xor_b32 {L.t0}, {2 * ks}, {xk}")
        A.e(f"v_lshl_add_u32 {v(dst + ks)}, {L.t0}, 4, {pi8}")


def vt_image_read_addrs(A, L, dst, scratch, lds_base):
    """V^T image ([128 d][64 keys] bf16, the forward's V^T tile and dQ's K^T tile): v[dst + s] = fragment read address of key
    step s = row d = 32 dt + r (dt in the ds_read's offset), chunk (2 s + h) ^ ((r >> 1) & 7)."""
    yv, r7 = scratch[:2]
    A.e(f"v_bfe_u32 {L.t0}, {L.r}, 1, 3")
    A.e(f"v_xor_b32 {yv}, {L.h}, {L.t0}")
    A.e(f"v_lshlrev_b32 {r7}, 7, {L.r}")
    A.e(f"v_add_u32 {r7}, {lds_base}, {r7}")
    for si in range(4):
        A.e(f"v_xor_b32 {L.t0}, {2 * si}, {yv}")
        A.e(f"v_lshl_add_u32 {v(dst + si)}, {L.t0}, 4, {r7}")


def k_image_dma_offsets(A, L, dst, scratch):
    """K image: v[dst + p] = global byte offset that piece p of wave w fetches = rows 16 w + 4 p + (lane >> 4) of 256 bytes,
    LDS position lane & 15 holding chunk (lane & 15) ^ (row & 15)."""
    l4, l15, key0 = scratch
    A.e(f"v_lshrrev_b32 {l4}, 4, {L.lane}")
    A.e(f"v_and_b32 {l15}, 15, {L.lane}")
    A.e(f"v_lshl_add_u32 {key0}, {L.w}, 4, {l4}")
    for p in range(4):
        A.e(f"v_add_u32 {L.t0}, {4 * p}, {key0}")
        A.e(f"v_add_u32 {L.t1}, {4 * p}, {l4}")
        A.e(f"v_xor_b32 {L.t1}, {l15}, {L.t1}")
        A.e(f"v_lshlrev_b32 {L.t1}, 4, {L.t1}")
        A.e(f"v_lshl_add_u32 {v(dst + p)}, {L.t0}, 8, {L.t1}")


def vt_image_dma_offsets(A, L, dst, scratch, row_stride):
    """V^T image: v[dst + p] = global byte offset that piece p of wave w fetches = rows d = 32 w + 8 p + (lane >> 3) of
    `row_stride` bytes (an SGPR), position lane & 7 holding chunk (lane & 7) ^ ((d >> 1) & 7)."""
    l3, l7, d0 = scratch
    A.e(f"v_lshrrev_b32 {l3}, 3, {L.lane}")
    A.e(f"v_and_b32 {l7}, 7, {L.lane}")
    A.e(f"v_lshl_add_u32 {d0}, {L.w}, 5, {l3}")
    for p in range(4):
        A.e(f"v_add_u32 {L.t0}, {8 * p}, {d0}")
        A.e(f"v_bfe_u32 {L.t1}, {L.t0}, 1, 3")
        A.e(f"v_xor_b32 {L.t1}, {l7}, {L.t1}")
        A.e(f"v_lshlrev_b32 {L.t1}, 4, {L.t1}")
        A.e(f"v_mad_u32_u24 {v(dst + p)}, {L.t0}, {s(row_stride)}, {L.t1}")


# ------------------------------------------------------------------------------------------------ LDS-DMA, MFMA gaps
def lds_dma(A, piece, fill=None):
    """piece = (m0 write, global_load_lds_*).  The wait state the load needs behind the m0 write is taken by the first
    instruction of `fill` (a list, consumed) or by an s_nop."""
    m0w, ld = piece
    A.e(m0w)
    A.e(fill.pop(0) if fill else "s_nop 0")
    A.e(ld)


def segment(A, mfmas, valu_gaps, valu_tail=(), lds=None, dma=None, pre=None, waits=None, extra=None, timing_only=()):
    """Emit one segment: per gap [wait] MFMA, the gap's VALU slice, at most one LDS read, at most one DMA piece.

    lds: {gap: instr}; dma: {gap: (m0 write, load)}; waits: {gap: 's_waitcnt ...'} placed in front of the gap's MFMA;
    extra: {gap: [instr]} behind everything else of the gap; pre / valu_tail: in front of / behind the segment.
    timing_only: diagnostic variants (wrong results) that leave out the "nodma", "nolds" or "novalu" share."""
    lds, dma, waits, extra = lds or {}, dma or {}, waits or {}, extra or {}
    if "nodma" in timing_only:
        dma = {}
    if "nolds" in timing_only:
        lds = {}
    if "novalu" in timing_only:
        valu_gaps = [[] for _ in valu_gaps]
    for x in pre or []:
        A.e(x)
    for g, m in enumerate(mfmas):
        if g in waits:
            A.e(waits[g])
        A.e(m)
        fill = list(valu_gaps[g]) if g < len(valu_gaps) else []
        if g in dma:
            lds_dma(A, dma[g], fill)
        for x in fill:
            A.e(x)
        if g in lds:
            A.e(lds[g])
        for x in extra.get(g, []):
            A.e(x)
    for x in valu_tail:
        A.e(x)


# ------------------------------------------------------------------------------------------------ epilogue stores
def store_acc_bf16(A, acc, mul, staging, rd, addr, ptr, offset=0):
    """a[acc : acc + 63] (a 32 x 128 fp32 tile: 4 d-tiles x 16) [* mul] -> bf16 -> memory at `addr` (a VGPR name) + the SGPR pair
    `ptr` + offset, as eight 16-byte stores: the lane halves exchange register pairs (v_permlane32_swap) so that each lane
    holds 8 consecutive columns.  v[rd : rd + 7] take the accumulators, the four quads v[staging : staging + 15] rotate."""
    for dt in range(4):
        for g in (0, 2):
            E = staging + 4 * ((dt * 2 + (g >> 1)) & 3)
            regs = [v(rd + j) for j in range(8)]
            for j in range(8):
                A.e(f"v_accvgpr_read_b32 {regs[j]}, {a(acc + 16 * dt + 4 * g + j)}")
            if mul is not None:
                for j in range(8):
                    A.e(f"v_mul_f32 {regs[j]}, {regs[j]}, {mul}")
            for j in range(4):
                A.e(f"v_cvt_pk_bf16_f32 {v(E + j)}, {regs[2 * j]}, {regs[2 * j + 1]}")
            A.e("s_nop 1")
            A.e(f"v_permlane32_swap_b32 {v(E)}, {v(E + 2)}")
            A.e(f"v_permlane32_swap_b32 {v(E + 1)}, {v(E + 3)}")
            A.e(f"global_store_dwordx4 {addr}, {vr(E, 4)}, {sr(ptr, 2)} offset:{offset + 64 * dt + 16 * g}")


# ------------------------------------------------------------------------------------------------ output
def clobbers(v_last, s_first, s_last):
    """The asm block's clobber list: v4 .. v_last, every AGPR, s_first .. s_last."""
    regs = [f"v{i}" for i in range(4, v_last + 1)] + [f"a{i}" for i in range(256)] + \
           [f"s{i}" for i in range(s_first, s_last + 1)] + ["vcc", "scc", "memory"]
    return ", ".join(f'"{x}"' for x in regs)


def render(macro_prefix, generator_path, body, clobber_list):
    """The text of a *_body.inc: <macro_prefix>_CLOBBERS and <macro_prefix>_BODY (the stream as one C string literal)."""
    lines = [f"// GENERATED by mixgrpo_amd/csrc/gen/{os.path.basename(generator_path)} -- do not edit; see that file for the design.",
             f"#define {macro_prefix}_CLOBBERS " + clobber_list,
             f"#define {macro_prefix}_BODY \\"]
    for ln in body.rstrip("\n").split("\n"):
        lines.append('  "' + ln.replace("\\", "\\\\").replace('"', '\\"') + '\\n" \\')
    lines.append('  ""')
    return "\n".join(lines) + "\n"


def write_if_changed(path, text):
    old = open(path).read() if os.path.exists(path) else None
    if old != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def main(generate, write, argv=None):
    """A generator's command line: `--print` writes the bare stream to stdout, the default rewrites its *_body.inc."""
    argv = sys.argv[1:] if argv is None else argv
    if "--print" in argv:
        sys.stdout.write(generate())
    else:
        print(write())
