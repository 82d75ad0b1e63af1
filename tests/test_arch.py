"""The model description (mixgrpo_amd/arch.py) on the host: the flat layout it derives is the one the commit before it built by
hand (names, shapes, order: checkpoints, optimizer state and the DP buckets depend on it), every descriptor's offsets are
`ParamStore`'s, fused projections split on member boundaries only, and the LoRA members computed from a descriptor are what
the scan of the layout order gave."""
import hashlib
import json

import pytest

from mixgrpo_amd import lora as LR
from mixgrpo_amd.arch import describe
from mixgrpo_amd.flux import FluxConfig, param_layout

# (entries, sha256[:16] of the json of [[name, shape]]) of `param_layout` at the commit before the description existed
PARENT_LAYOUT = [
    (FluxConfig(), 1160, "0ab99ad7b706c82b"),
    (FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2), 112, "7772ae304a79b13a"),
    (FluxConfig(num_layers=1, num_single_layers=1, num_attention_heads=2, guidance_embeds=False), 62, "b56bf0eb6f44d171"),
]
CFG = PARENT_LAYOUT[1][0]
D = CFG.dim


def wgrad_linears(arch):
    """Every Linear `flux_backward._wgrad` is called with."""
    out = [arch.x_embedder, arch.context_embedder, arch.proj_out]
    for b in arch.double:
        for s in b.streams:
            out += [s.qkv, s.out, s.ff0, s.ff2]
    for b in arch.single:
        out += [b.qkv_mlp, b.proj_out]
    return out


def all_linears(arch):
    out = wgrad_linears(arch) + [arch.norm_out] + [l for _, l1, l2 in arch.embedders for l in (l1, l2)]
    out += [s.norm for b in arch.double for s in b.streams]
    for b in arch.single:
        out += [b.norm, b.qkv, b.proj_mlp]
    return out


@pytest.mark.parametrize("cfg,count,digest", PARENT_LAYOUT, ids=["flux1dev", "2+2", "1+1_noguidance"])
def test_layout_is_the_parents(cfg, count, digest):
    layout = param_layout(cfg)
    assert len(layout) == count
    assert hashlib.sha256(json.dumps([[n, list(s)] for n, s in layout]).encode()).hexdigest()[:16] == digest


@pytest.mark.parametrize("cfg", [c for c, _, _ in PARENT_LAYOUT], ids=["flux1dev", "2+2", "1+1_noguidance"])
def test_descriptor_offsets_are_the_stores(cfg):
    """Offsets recomputed from the layout the way `ParamStore` always laid it out: every tensor at the next multiple of 64."""
    arch, layout = describe(cfg), param_layout(cfg)
    off, want = 0, {}
    for name, shape in layout:
        n = 1
        for s in shape:
            n *= s
        want[name] = (off, tuple(shape))
        off += (n + 63) // 64 * 64
    assert arch.index == want and arch.numel == off and list(arch.index) == [n for n, _ in layout]
    lins = all_linears(arch)
    assert len(lins) == 4 + 2 * len(arch.embedders) + 10 * cfg.num_layers + 5 * cfg.num_single_layers
    for lin in lins:
        assert (lin.w_off, lin.b_off) == (want[f"{lin.module}.weight"][0], want[f"{lin.module}.bias"][0]), lin.module
        assert lin.members[0][:2] == (lin.module, 0) and sum(n for _, _, n in lin.members) == lin.N
        for module, r0, n in lin.members:                     # each member sits where a fused view expects it
            assert want[f"{module}.weight"] == (lin.w_off + r0 * lin.K, (n, lin.K)), module
            assert want[f"{module}.bias"] == (lin.b_off + r0, (n,)), module
    for vec in [v for b in arch.double for s in b.streams for v in (s.norm_q, s.norm_k)] + \
               [v for b in arch.single for v in (b.norm_q, b.norm_k)]:
        assert want[vec.name] == (vec.off, (vec.n,))
    # every parameter belongs to exactly one descriptor
    covered = [f"{m}.{part}" for lin in lins if lin not in [x for b in arch.single for x in (b.qkv, b.proj_mlp)]
               for m, _, _ in lin.members for part in ("weight", "bias")]
    covered += [s_.name for b in arch.double for s in b.streams for s_ in (s.norm_q, s.norm_k)]
    covered += [v.name for b in arch.single for v in (b.norm_q, b.norm_k)]
    assert sorted(covered) == sorted(want)


def test_rows_split_fused_linears_on_member_boundaries_only():
    arch = describe(CFG)
    fused = [lin for lin in all_linears(arch) if len(lin.members) > 1]
    assert len(fused) == 2 * CFG.num_layers + 2 * CFG.num_single_layers      # (qkv per stream; qkv_mlp and its qkv rows)
    for lin in fused:
        assert sum(n for _, _, n in lin.members) == lin.N
        for i, (module, r0, n) in enumerate(lin.members):
            for j in range(i, len(lin.members)):                             # every run of members i..j
                hi = lin.members[j][1] + lin.members[j][2]
                sub = lin.rows(r0, hi)
                assert (sub.module, sub.N, sub.K) == (module, hi - r0, lin.K)
                assert (sub.w_off, sub.b_off) == arch.index[f"{module}.weight"][0:1] + arch.index[f"{module}.bias"][0:1]
                assert sub.members == tuple((m, a - r0, k) for m, a, k in lin.members[i:j + 1])
        for lo, hi in ((1, lin.N), (0, lin.N - 1), (0, D // 2), (D // 2, D), (0, lin.N + D), (D, D), (lin.N, lin.N + D)):
            with pytest.raises(ValueError):
                lin.rows(lo, hi)
    sb = arch.single[1]
    assert sb.qkv == sb.qkv_mlp.rows(0, 3 * D) and sb.proj_mlp == sb.qkv_mlp.rows(3 * D, 7 * D)
    assert sb.proj_mlp.members == ((f"{sb.prefix}.proj_mlp", 0, 4 * D),)


def layout_scan_members(layout, by_module, wname, total):
    """The LoRA members as the commit before the description found them: a cumulative scan of the layout order from the
    first member's weight name over `total` output rows."""
    order, shape = [n for n, _ in layout], dict(layout)
    hit, i, col = [], order.index(wname), 0
    while col < total:
        name = order[i]
        module = name[:-len(".weight")]
        if module in by_module:
            hit.append((module, col, shape[name][0]))
        col += shape[name][0]
        i += 1
    assert col == total
    return hit


@pytest.mark.parametrize("targets", [None, LR.SUPPORTED_TARGETS], ids=["default", "all_supported"])
def test_lora_members_are_the_layout_scans(targets):
    arch = describe(CFG)
    lo = LR.LoraStore(CFG, "cpu", 16, 16, targets, allocate=False)
    found = 0
    for lin in wgrad_linears(arch):
        got = lo.members(lin)
        assert got == layout_scan_members(param_layout(CFG), lo.by_module, f"{lin.module}.weight", lin.N), lin.module
        found += len(got)
    assert found == len(lo.targets)                            # every adapter is reached by exactly one weight-gradient call


def test_block_ranges_are_the_layout_scans():
    """`ParamStore.block_ranges` reads the block starts off the description; the commit before it scanned the names."""
    from mixgrpo_amd.flux import ParamStore
    for cfg in (CFG, PARENT_LAYOUT[2][0], FluxConfig(num_layers=0, num_single_layers=2, num_attention_heads=2)):
        st = ParamStore(cfg, "cpu")
        block = lambda n: ".".join(n.split(".")[:2]) if "transformer_blocks." in n else \
            ("head" if st.index[n][0] < st.index["norm_out.linear.weight"][0] else "tail")
        want = {}
        for n, (off, _) in st.index.items():
            want.setdefault(block(n), off)
        ends = list(want.values())[1:] + [st.numel]
        assert list(st.block_ranges().items()) == [(k, (lo, hi)) for (k, lo), hi in zip(want.items(), ends)]
