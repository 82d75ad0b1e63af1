"""The padded no-grad forward of the FLUX MMDiT (ops.ATTN_PAD_KV / MGX_ATTN_PAD_KV=1): a sequence off 256 runs at the next
multiple of 256 with the added keys masked in the attention forward (mgx_attn_fwd_log2_kv), against the CPU oracle
(oracle/mmdit.py) on the unpadded problem.  Smallest configuration of the existing MMDiT tests (tests/test_hip_mmdit.py:
small_cfg, 1 + 1 blocks), L = 256 text + N = 225 image tokens (a 15 x 15 packed latent): S = 481 -> Sa = 512."""
import pytest
import torch

from oracle import mmdit as OM
from test_hip_mmdit import build_pair, make_inputs, rel_err, small_cfg

pytestmark = pytest.mark.gpu

B, HG, WG, L = 1, 15, 15, 256
FWD_REL_L2 = 1e-2            # the bound of the no-grad forward against the oracle, tests/test_hip_mmdit.py:62 (and :406)


@pytest.fixture(scope="module")
def problem():
    ocfg, P, m = build_pair(small_cfg(1, 1))
    m.eval()
    x, ehs, pooled, ids, tids, t, gd = make_inputs(B, HG, WG, L)
    with torch.no_grad():
        ref = OM.forward(P, ocfg, x, ehs.float(), t, gd.float(), tids, pooled.float(), ids)
    args = (x.cuda(), ehs.cuda(), t.cuda(), gd.cuda(), tids.cuda(), pooled.cuda(), ids.cuda())
    return m, args, ref


def test_padded_forward_vs_oracle(problem, monkeypatch):
    from mixgrpo_amd import ops
    m, args, ref = problem
    N, H, d = HG * WG, m.cfg.num_attention_heads, m.cfg.dim
    assert (L + N) % 256 != 0 and ops.attn_fwd_kv_path(B, H, 512, L + N, d, 512 * d) == 1
    monkeypatch.setattr(ops, "ATTN_PAD_KV", True)
    calls = m.padded_kv_calls
    with torch.no_grad():
        out = m._forward_nograd(*args)
    torch.cuda.synchronize()
    assert m.last_route == "padded_kv" and m.padded_kv_calls == calls + 1, "the padded route was not taken"
    assert out.dtype == torch.bfloat16 and out.shape == (B, N, 64) and out.is_contiguous()
    e = rel_err(out, ref)
    print(f"padded forward against the oracle: rel L2 {e:.3g}")
    assert e < FWD_REL_L2
    # through the public call as well, and the workspace's mask does not outlive the call
    out2 = m(*args)[0]
    assert torch.equal(out2, out) and m.last_route == "padded_kv"
    assert all(w.kv_len is None for w in m._work.values())


def test_switch_off_is_the_unpadded_path(problem, monkeypatch):
    """With the switch off (the default) the route is not taken, and the forward is what it was: the same bits from a second
    call, also after a padded call in between (its workspace is another one), and within the same bound of the oracle."""
    from mixgrpo_amd import ops
    m, args, ref = problem
    monkeypatch.setattr(ops, "ATTN_PAD_KV", False)
    calls = m.padded_kv_calls
    with torch.no_grad():
        a = m._forward_nograd(*args)
        assert m.last_route == "plain"
        monkeypatch.setattr(ops, "ATTN_PAD_KV", True)
        m._forward_nograd(*args)
        assert m.last_route == "padded_kv"
        monkeypatch.setattr(ops, "ATTN_PAD_KV", False)
        b = m._forward_nograd(*args)
    assert m.last_route == "plain" and m.padded_kv_calls == calls + 1
    assert torch.equal(a, b)
    assert rel_err(a, ref) < FWD_REL_L2


def test_switch_is_off_by_default_and_skips_what_it_cannot_take(problem, monkeypatch):
    import os
    from mixgrpo_amd import ops
    m, args, _ = problem
    if "MGX_ATTN_PAD_KV" not in os.environ:
        assert ops.ATTN_PAD_KV is False
    monkeypatch.setattr(ops, "ATTN_PAD_KV", True)
    monkeypatch.setenv("MGX_ATTN_W64", "0")           # the 64-query kernels are switched off: the path query says 0
    with torch.no_grad():
        m._forward_nograd(*args)
    assert m.last_route == "plain"
