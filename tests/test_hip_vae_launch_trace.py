"""The VAE host code's launch sequence, call for call, against a recording of the commit before the halves' layer description
existed: every C-ABI call a decode / encode makes -- entry point, return code, every scalar, and every pointer as
`<buffer>+<byte offset>` (helpers.Recorder) -- has to be the recorded one.  A wrong key, channel count, resolution or buffer
at one of the description's users shows here as the first differing call.

The registered buffers are the weights `P.<key>`, the model's activation buffers `buf.<key tuple>` -- their keys decide
which layers share memory and keep `pad_z` / `pad_x` apart from the shared 64-channel pads, so they are part of the record --
`ones`, `ops._scratch` and `ops._sk_ws`.  Everything else (the per-image inputs, images, moments, the Gaussian's tensors) is a
temporary; which temporaries share an address is the caching allocator's doing, so each pass runs on a private memory pool
with the scratch caches emptied.

`python tests/test_hip_vae_launch_trace.py --write` records tests/golden/vae_launch_trace.json (on an MI355X)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GOLDEN, Recorder, assert_trace, record_traces, scratch_buffers, tensor_extents  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "vae_launch_trace.json")
SMALL = dict(block_out_channels=(64, 128, 128), layers_per_block=1, sample_size=64)        # 4x; tile 64 px / 16 latent
# name -> config, `z` (decode) or `x` (encode) shape, tiling; sample: draw from the posterior with a seeded device generator;
# full False: the fixture holds the number of calls and a sha256 of their canonical text instead of every call
PASSES = {
    # a batch of two, image by image; a 128 -> 64 shortcut resnet; upsamplers; attention at H W % 64 == 0
    "dec_whole": dict(cfg=SMALL, z=(2, 16, 16, 16)),
    # 2 x 3 ragged tiles: buffers re-keyed per tile size
    "dec_tiled": dict(cfg=SMALL, z=(1, 16, 20, 28), tiling=True, full=False),
    # H W = 35: the spare k rows, the zero-padded P and v^T of `_attention`
    "dec_odd_attn": dict(cfg=SMALL, z=(1, 16, 5, 7)),
    "dec_no_attn": dict(cfg=dict(block_out_channels=(64, 64), layers_per_block=1, sample_size=32, mid_block_add_attention=False),
                        z=(1, 16, 8, 8)),
    # down blocks, the stride-2 convolution, pad_x, the Gaussian's calls
    "enc_whole": dict(cfg=SMALL, x=(2, 3, 32, 48), sample=True),
    "enc_odd_attn": dict(cfg=SMALL, x=(1, 3, 20, 28)),
    # 2 x 3 image tiles, their moments blended, one Gaussian
    "enc_tiled": dict(cfg=SMALL, x=(1, 3, 80, 112), tiling=True, full=False),
    # the four-block channel walk of the real configuration (512, 512, 256, 128: two shortcuts)
    "dec_flux16": dict(cfg={}, z=(1, 16, 16, 16), full=False),
    "enc_flux32": dict(cfg={}, x=(1, 3, 32, 32), full=False),
}


def _buffers(m, ops):
    named = [(f"P.{k}", t) for k, t in m.P.items()]
    named += [("buf." + ".".join(str(p) for p in key), t) for key, t in m._buf.items()]
    return tensor_extents(named + [("ones", m._ones)] + scratch_buffers(ops))


def run_pass(spec, monkeypatch):
    """The calls of one pass, in order."""
    from mixgrpo_amd import _lib, ops
    from mixgrpo_amd.vae import AutoencoderKL, VaeConfig
    rec = Recorder(_lib.lib(), _lib.SIGNATURES)
    monkeypatch.setattr(ops, "lib", lambda: rec)
    ops._scratch.clear()
    ops._sk_ws.clear()
    torch.cuda.synchronize()
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        m = AutoencoderKL(VaeConfig(**spec["cfg"]), device="cuda").init_synthetic(seed=7)
        m.enable_tiling(spec.get("tiling", False))
        decode = "z" in spec
        inp = torch.randn(spec["z" if decode else "x"], generator=torch.Generator().manual_seed(3))
        inp = (inp if decode else inp.clamp(-1, 1)).cuda()
        rec.buffers = lambda: _buffers(m, ops)
        del rec.calls[:]
        rec.first_use.clear()
        if decode:
            out = m.decode(inp, return_dict=False)[0]
        else:
            out = m.encode(inp).latent_dist
            if spec.get("sample"):
                out = (out, out.sample(torch.Generator(device="cuda").manual_seed(5)))
        torch.cuda.synchronize()
        rec.buffers = None
        del m, inp, out
    monkeypatch.undo()
    ops._scratch.clear()
    ops._sk_ws.clear()
    del pool
    return rec.calls


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["passes"]


@pytest.mark.parametrize("name", list(PASSES))
def test_vae_launch_sequence_is_the_recorded_one(name, recorded, monkeypatch):
    assert_trace(name, run_pass(PASSES[name], monkeypatch), recorded[name])


if __name__ == "__main__":
    # record the fixture (twice, the second time in the reverse order: helpers.record_traces)
    assert sys.argv[1:2] == ["--write"], "usage: python tests/test_hip_vae_launch_trace.py --write [PATH]"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record_traces(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, PASSES, run_pass)
