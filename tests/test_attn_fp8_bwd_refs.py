"""CPU checks of the references of the e4m3 attention backward (tests/attn_fp8_bwd_refs.py) and of the host side of
`mgx_attn_bwd_fp8`: (a) is torch autograd of the dequantised forward; (b) -- the kernel's quantisation points -- lies within
5e-2 relative L2 of (a) per tensor (the e4m3 mantissa: 3 bits, rms relative error 3.6 % per value, the size of the forward's
4e-2; a CPU emulation of the recipe measured 3.6-3.8e-2 at S = 320 and 1024, gaussian inputs at amplitude 1 and 2); the
transposed images use the forward's key order; the workspace query and the switch's default."""
import math
import os

import pytest
import torch

import attn_fp8_bwd_refs as R
from oracle import attention_fp8 as OA

SCALE = 1.0 / math.sqrt(128)


def _inputs(B, H, S, amp, seed):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randn(B, H, S, 128, generator=g) * amp).bfloat16()
    K = (torch.randn(B, H, S, 128, generator=g) * amp).bfloat16()
    V = torch.randn(B, H, S, 128, generator=g).bfloat16()
    dO = (torch.randn(B, H, S, 128, generator=g) * 1e-3).bfloat16()
    return Q, K, V, dO


def test_exact_reference_is_autograd_of_the_dequantised_forward():
    Q, K, V, dO = _inputs(1, 2, 150, 1.0, 0)
    am = R.amax_table(Q, K, V, dO)
    q, k, v = (R.dequantize(OA.quantize(x, am[i]), am[i]).requires_grad_(True) for i, x in enumerate((Q, K, V)))
    O = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * SCALE, -1) @ v
    (O * dO.double()).sum().backward()
    ref = R.backward(Q, K, V, O.detach(), dO, SCALE, faithful=False)
    for mine, auto in zip(ref, (q.grad, k.grad, v.grad)):
        assert R.rel_l2(mine, auto) < 1e-12
    assert torch.allclose(O.detach(), OA.attention(Q, K, V, SCALE)[0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("S,amp", [(320, 1.0), (320, 2.0), (200, 2.0)])
def test_quantiser_faithful_reference_is_within_the_e4m3_mantissa(S, amp):
    Q, K, V, dO = _inputs(1, 2, S, amp, S)
    O = OA.attention(Q, K, V, SCALE)[0].bfloat16()
    a = R.backward(Q, K, V, O, dO, SCALE, faithful=False)
    b = R.backward(Q, K, V, O, dO, SCALE, faithful=True)
    for name, xa, xb in zip(("dQ", "dK", "dV"), a, b):
        rel = R.rel_l2(xb, xa)
        print(f"S {S} amp {amp} {name}: (b) vs (a) rel L2 {rel:.3e}")
        assert 1e-3 < rel < 5e-2, (name, rel)


def test_mx_blocks_are_exact_on_representable_data():
    """Values that are e4m3 numbers times one power of two per block come back unchanged, whatever the block's magnitude."""
    g = torch.Generator().manual_seed(1)
    base = torch.randint(-15, 16, (3, 100, 70), generator=g).double() / 8           # e4m3-exact
    x = base * torch.exp2(torch.randint(-30, 10, (3, 1, 70), generator=g).double())
    assert torch.equal(R.mx_quantize(x, -2), x)
    y = base.clone()
    y[:, 32:64] *= 2.0 ** -20                                                       # one block far below its neighbours
    assert torch.equal(R.mx_quantize(y, -2), y)
    assert torch.equal(R.mx_quantize(torch.zeros(2, 5, 9, dtype=torch.float64), -1), torch.zeros(2, 5, 9, dtype=torch.float64))


def test_transposed_image_permutation_is_the_forwards_key_order():
    assert R.accumulator_order() == OA.key_order()
    assert sorted(R.accumulator_order()) == list(range(64))
    x8 = torch.arange(2 * 70 * 128).view(1, 2, 70, 128).to(torch.uint8).view(torch.float8_e4m3fn)
    assert torch.equal(R.transposed_image(x8, 128), OA.v8t_layout(x8, 128))


def test_workspace_query_needs_no_gpu():
    from mixgrpo_amd import ops
    sizes = [ops.attn_bwd_fp8_workspace(2, 3, S, (S + 63) // 64 * 64) for S in (1, 63, 64, 65, 300, 4608)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    for S in (1, 300):
        Sp = (S + 63) // 64 * 64
        lay = ops.attn_bwd_fp8_layout(2, 3, S, Sp)
        end = max(off + math.prod(shape) for off, shape in lay.values())
        assert end <= ops.attn_bwd_fp8_workspace(2, 3, S, Sp) and all(off % 256 == 0 for off, _ in lay.values())
    with pytest.raises(ValueError):
        ops.attn_bwd_fp8_workspace(1, 1, 65, 64)


def test_switch_is_off_by_default():
    from mixgrpo_amd import ops
    assert ops.ATTN_FP8_BWD is (os.environ.get("MGX_ATTN_FP8_BWD", "0") != "0")
    assert "MGX_ATTN_FP8_BWD" in os.environ or ops.ATTN_FP8_BWD is False
