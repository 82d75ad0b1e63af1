"""The MMDiT host code's launch sequence, call for call, against a recording of the commit before the model description
(mixgrpo_amd/arch.py) existed: every C-ABI call a forward / backward makes -- entry point, return code, every scalar, and
every pointer as `<buffer>+<byte offset>` -- has to be the recorded one.  A wrong N / K / row range / operand address at one
of the description's users shows here as the first differing call instead of as a tolerance failure of a whole model.

`ops.lib` is replaced by a recording proxy (helpers.Recorder) and nothing else is patched.  Pointers (the `c_void_p` arguments of
`_lib.SIGNATURES`) are named after the registered buffer they fall into -- the parameter stores, the `_Work` / `_Train` bases,
`tr.save`, `tr.keep`, `ops._scratch`, `ops._sk_ws` -- and any other address is a temporary, `tmp<k>` with k the index of the
first call that used that exact address (`tmp<k>.<j>` for the further new addresses of that call).  Which temporaries share
an address is the caching allocator's doing, so each pass runs on a private memory pool with the scratch caches emptied and
the backward on the calling thread: the record then does not depend on what ran before it in the process.

`python tests/test_hip_launch_trace.py --write` records tests/golden/launch_trace.json (on an MI355X).  The persistent-GEMM-
only entry points need >= 128 tiles of 256 x 256 to take a problem: here they are called and refuse (return code 1 in the
trace), the full-width tests run them."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import (GOLDEN, Recorder, assert_trace, make_inputs, record_traces, scratch_buffers, small_cfg,  # noqa: E402
                     tensor_extents)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "launch_trace.json")
LORA_TARGETS = ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out", "proj_mlp",
                "ff.net.0.proj")
S84 = dict(blocks=(1, 1), B=2, grid=(6, 10), L=24)          # S = 84: the 8-wave attention kernels
# name -> blocks, batch, latent grid, text tokens; keep = (KEEP_ACTS, KEEP_FF, KEEP_QKV) of a training forward + backward
# (absent: the no-grad forward); lora: with rank-16 adapters on LORA_TARGETS; full: the fixture holds every call (else the
# number of calls and a sha256 of their canonical text)
PASSES = {
    "nograd": dict(S84),
    "train_keep": dict(S84, keep=(True, "0", "0")),
    "train_recompute": dict(S84, keep=(False, "0", "0")),
    "train_lean": dict(S84, keep=(True, "99", "99")),
    "lora_keep": dict(S84, keep=(True, "0", "0"), lora=True),
    "lora_recompute": dict(S84, keep=(False, "0", "0"), lora=True),
    "lora_lean": dict(S84, keep=(True, "99", "99"), lora=True),
    # block-index arithmetic across the double / single boundary, kept and not-kept blocks mixed
    "train_2+2_mixed": dict(S84, blocks=(2, 2), keep=(True, "1", "2"), full=False),
    # S = 256: the 64-wide attention streams; no guidance embedder
    "train_s256_noguidance": dict(blocks=(1, 1), B=1, grid=(16, 12), L=64, keep=(True, "0", "0"), guidance_embeds=False),
}


def _buffers(model, ops):
    named = []
    for sname, st in (("store", model.store), ("lora", model.lora)):
        named += [(f"{sname}.{b}", getattr(st, b, None)) for b in ("w16", "w32", "g32")]
    for wi, base in enumerate(model._work.values()):
        named += [(f"work{wi}.{k}", v) for k, v in vars(base).items()]
        tr = base.train
        if tr is None:
            continue
        named += [(f"train{wi}.{k}", v) for k, v in vars(tr).items()]
        named += [(f"train{wi}.save.{k}", v) for k, v in tr.save.items()]
        for i, kb in enumerate(tr.keep or []):
            named += [(f"train{wi}.keep{i}.{k}", v) for k, v in kb.items()]
    return tensor_extents(named + scratch_buffers(ops))


def run_pass(spec, monkeypatch):
    """The calls of one pass, in order."""
    from mixgrpo_amd import _lib, ops
    from mixgrpo_amd import flux_backward as FB
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    keep = spec.get("keep")
    for name, v in zip(("KEEP_ACTS", "KEEP_FF", "KEEP_QKV"), keep or ()):
        monkeypatch.setattr(FB, name, v)
    rec = Recorder(_lib.lib(), _lib.SIGNATURES)
    monkeypatch.setattr(ops, "lib", lambda: rec)
    ops._scratch.clear()
    ops._sk_ws.clear()
    torch.cuda.synchronize()
    B, (hg, wg), L = spec["B"], spec["grid"], spec["L"]
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool), torch.autograd.set_multithreading_enabled(False):
        cfg = FluxConfig(**small_cfg(*spec["blocks"]), guidance_embeds=spec.get("guidance_embeds", True))
        m = FluxTransformer2DModel(cfg, device="cuda").init_synthetic(seed=1, std=0.05, bias_std=0.02)
        if spec.get("lora"):
            m.add_lora(rank=16, target_modules=LORA_TARGETS)
        inputs = [t.cuda() for t in make_inputs(B, hg, wg, L, seed=3)]
        x, ehs, pooled, ids, tids, t, gd = inputs
        R = torch.randn(B, hg * wg, 64, generator=torch.Generator().manual_seed(9)).cuda()
        rec.buffers = lambda: _buffers(m, ops)
        del rec.calls[:]                                   # (attaching adapters merges them: not part of the pass)
        rec.first_use.clear()
        if keep is None:
            with torch.no_grad():
                m.eval()
                m._forward_nograd(x, ehs, t, gd, tids, pooled, ids)
        else:
            m.train()
            out = m(x, ehs, t, gd, tids, pooled, ids)[0]
            (out.float() * R).sum().backward()
            del out
        torch.cuda.synchronize()
        rec.buffers = None
        del m, inputs, x, ehs, pooled, ids, tids, t, gd, R
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
def test_launch_sequence_is_the_recorded_one(name, recorded, monkeypatch):
    assert_trace(name, run_pass(PASSES[name], monkeypatch), recorded[name])


if __name__ == "__main__":
    # record the fixture (twice, the second time in the reverse order: helpers.record_traces)
    assert sys.argv[1:2] == ["--write"], "usage: python tests/test_hip_launch_trace.py --write [PATH]"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record_traces(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, PASSES, run_pass)
