"""The buffer plan of one block and one pass (flux_backward._BlockPlan) against the table of what each pass reads, writes and
skips, written out here per pass: no-grad, training forward into keep buffers, full recompute, replay of what was kept.
Everything is compared by data_ptr() and shape on CPU tensors: 2 double + 2 single blocks, H = 4, head_dim 128, capacity
B = 2 with a view at B = 1, L = 24, N = 60."""
import pytest
import torch

from mixgrpo_amd import flux_backward as FB
from mixgrpo_amd.flux import FluxConfig, _Work, _WorkView

CFG = FluxConfig(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4, joint_attention_dim=64,
                 pooled_projection_dim=32)
B, L, N = 2, 24, 60
D = CFG.dim
ROLES = ("restore", "x_in", "nrm1", "nrm2", "qkv", "V", "Qt", "Kt", "O", "lse", "y_attn", "hid_pre")
FLAGS = ("fused_qkv", "run_qkv", "run_attn", "run_out", "run_ff", "lean")
# (KEEP_ACTS, KEEP_FF, KEEP_QKV) -> per block (keeps hid_pre, keeps qkv)
SETTINGS = {(False, "0", "0"): None,
            (True, "0", "0"): [(False, False)] * 4,
            (True, "1", "2"): [(True, True), (False, True), (False, False), (False, False)],
            (True, "99", "99"): [(True, True)] * 4}


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype


def buffers(monkeypatch, setting):
    for name, v in zip(("KEEP_ACTS", "KEEP_FF", "KEEP_QKV"), setting):
        monkeypatch.setattr(FB, name, v)
    w = _Work(CFG, B, L, N, torch.device("cpu"))
    return w, FB._Train(CFG, w, torch.device("cpu"))


def expected(w, tr, blk, kind, keeps):
    """(roles, flags) of the issue's table; `keeps`: (hid_pre kept, qkv kept) of this block, or None without keep buffers."""
    double = blk < CFG.num_layers
    k = tr.keep[blk] if keeps is not None else None
    s = tr.save
    ff, qkv = keeps if keeps is not None else (False, False)
    flags = dict(fused_qkv=False, run_qkv=True, run_attn=True, run_out=True, run_ff=True, lean=False)
    if kind == "nograd" or (kind == "forward" and k is None):
        flags["fused_qkv"] = True
        r = dict(restore=None, x_in=w.X, nrm1=w.nrm, nrm2=w.nrm, qkv=w.qkv, V=None, Qt=None, Kt=None, O=w.O, lse=None, y_attn=None,
                 hid_pre=None, y_ff=None, x_mid=None, O_keep=None)
    elif kind == "forward":
        r = dict(restore=None, x_in=w.X, nrm1=w.nrm, nrm2=w.nrm, qkv=k["qkv"] if qkv else w.qkv, V=None, Qt=None, Kt=None, O=k["O"],
                 lse=k["lse"], y_attn=k["y_attn"], hid_pre=k["hid_pre"] if ff else None, y_ff=k.get("y_ff"), x_mid=k.get("x_mid"),
                 O_keep=k["O"])
    elif k is None:                                       # recompute, nothing kept
        r = dict(restore=tr.block_in[blk], x_in=w.X, nrm1=s["nrm1"], nrm2=s["nrm2"], qkv=w.qkv, V=s["V"], Qt=s["Qt"], Kt=s["Kt"],
                 O=w.O, lse=w.lse, y_attn=s["y_attn"], hid_pre=s["hid_pre"], y_ff=s["y_ff"], x_mid=s["x_mid"], O_keep=None)
    else:                                                 # recompute, replaying what the block kept
        flags.update(run_qkv=not qkv, run_attn=False, run_out=False, run_ff=not ff, lean=ff and not double)
        r = dict(restore=None, x_in=tr.block_in[blk], nrm1=s["nrm1"], nrm2=s["nrm2"], qkv=k["qkv"] if qkv else w.qkv, V=s["V"],
                 Qt=s["Qt"], Kt=s["Kt"], O=k["O"], lse=k["lse"], y_attn=k["y_attn"], hid_pre=k["hid_pre"] if ff else s["hid_pre"],
                 y_ff=k.get("y_ff"), x_mid=k.get("x_mid"), O_keep=k["O"])
    if double:
        r["ldo"] = D
        del r["O_keep"]
    else:                                                 # [O | mlp] in w.cat at row stride 5d, unless lean
        del r["y_ff"], r["x_mid"]
        r["O"], r["ldo"] = (k["O"], D) if flags["lean"] else (w.cat, 5 * D)
    return r, flags


def plan(w, tr, blk, kind):
    double = blk < CFG.num_layers
    if kind == "nograd":
        return FB._BlockPlan(w, double)
    return FB._BlockPlan(w, double, tr, blk, recompute=kind == "recompute")


@pytest.mark.parametrize("setting", list(SETTINGS), ids=lambda s: "-".join(map(str, s)))
def test_every_role_and_step_of_every_pass(monkeypatch, setting):
    w, tr = buffers(monkeypatch, setting)
    keeps = SETTINGS[setting]
    assert (tr.keep is not None) == setting[0]
    if keeps is not None:
        assert [("hid_pre" in k, "qkv" in k) for k in tr.keep] == keeps
    for wv, trv in ((w, tr), (w.view(1), tr.view(1))):
        for blk in range(4):
            for kind in ("nograd", "forward", "recompute"):
                pl = plan(wv, trv, blk, kind)
                roles, flags = expected(wv, trv, blk, kind, None if keeps is None else keeps[blk])
                where = (setting, wv.B, blk, kind)
                for name, t in roles.items():
                    got = getattr(pl, name)
                    assert (got == t) if name == "ldo" else same(got, t), (where, name)
                for name, v in flags.items():
                    assert getattr(pl, name) is v, (where, name)
                assert hasattr(pl, "y_ff") == hasattr(pl, "x_mid") == (blk < 2) and hasattr(pl, "O_keep") == (blk >= 2), where


def test_lean_exactly_for_single_blocks_that_keep_hid_pre(monkeypatch):
    for setting, keeps in SETTINGS.items():
        w, tr = buffers(monkeypatch, setting)
        for blk in range(4):
            want = keeps is not None and keeps[blk][0] and blk >= CFG.num_layers
            assert plan(w, tr, blk, "recompute").lean is want, (setting, blk)
            assert plan(w, tr, blk, "forward").lean is False and plan(w, tr, blk, "nograd").lean is False
    assert sum(keeps is not None and keeps[blk][0] and blk >= 2 for keeps in SETTINGS.values() for blk in range(4)) == 2


def test_views_resolve_to_leading_slices_of_the_same_storage(monkeypatch):
    w, tr = buffers(monkeypatch, (True, "1", "2"))
    w1, tr1 = w.view(1), tr.view(1)
    assert isinstance(w1, _WorkView) and isinstance(tr1, FB._TrainView)
    for blk in range(4):
        for kind in ("nograd", "forward", "recompute"):
            full, part = plan(w, tr, blk, kind), plan(w1, tr1, blk, kind)
            for name in ROLES + (("y_ff", "x_mid") if blk < 2 else ("O_keep",)):
                a, b = getattr(full, name), getattr(part, name)
                assert (a is None) == (b is None), (blk, kind, name)
                if a is not None:
                    assert b.data_ptr() == a.data_ptr() and b.is_contiguous(), (blk, kind, name)
                    assert b.shape[0] * 2 == a.shape[0] and b.shape[1:] == a.shape[1:], (blk, kind, name)
            assert all(getattr(full, f) == getattr(part, f) for f in FLAGS + ("ldo",))


def test_kv_len_lives_on_the_view(monkeypatch):
    w, _ = buffers(monkeypatch, (False, "0", "0"))
    assert w.view(B) is w and w.kv_len is None
    for b in (1, B):                                      # a padded call gets a view of its own even at full capacity
        v = w.view(b, kv_len=L + N - 5)
        assert isinstance(v, _WorkView) and v.kv_len == L + N - 5 and v.B == b and v.base is w
        assert same(v.X, w.X[:b]) and same(v.cat, w.cat[:b]) and same(v.lse, w.lse[:b])
    assert w.view(1).kv_len is None and w.kv_len is None
