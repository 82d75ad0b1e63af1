"""The MMDiT host code's launch sequence, call for call, against a recording of the commit before the model description
(mixgrpo_amd/arch.py) existed: every C-ABI call a forward / backward makes -- entry point, return code, every scalar, and
every pointer as `<buffer>+<byte offset>` -- has to be the recorded one.  A wrong N / K / row range / operand address at one
of the description's users shows here as the first differing call instead of as a tolerance failure of a whole model.

`ops.lib` is replaced by a recording proxy and nothing else is patched.  Pointers (the `c_void_p` arguments of
`_lib.SIGNATURES`) are named after the registered buffer they fall into -- the parameter stores, the `_Work` / `_Train` bases,
`tr.save`, `tr.keep`, `ops._scratch`, `ops._sk_ws` -- and any other address is a temporary, `tmp<k>` with k the index of the
first call that used that exact address (`tmp<k>.<j>` for the further new addresses of that call).  Which temporaries share
an address is the caching allocator's doing, so each pass runs on a private memory pool with the scratch caches emptied and
the backward on the calling thread: the record then does not depend on what ran before it in the process.

`python tests/test_hip_launch_trace.py --write` records tests/golden/launch_trace.json (on an MI355X).  The persistent-GEMM-
only entry points need >= 128 tiles of 256 x 256 to take a problem: here they are called and refuse (return code 1 in the
trace), the full-width tests run them."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GOLDEN, make_inputs, small_cfg  # noqa: E402

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
    out = []

    def add(name, t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.numel():
            out.append((name, t.data_ptr(), t.numel() * t.element_size()))

    for sname, st in (("store", model.store), ("lora", model.lora)):
        for b in ("w16", "w32", "g32"):
            add(f"{sname}.{b}", getattr(st, b, None))
    for wi, base in enumerate(model._work.values()):
        for k, v in vars(base).items():
            add(f"work{wi}.{k}", v)
        tr = base.train
        if tr is None:
            continue
        for k, v in vars(tr).items():
            add(f"train{wi}.{k}", v)
        for k, v in tr.save.items():
            add(f"train{wi}.save.{k}", v)
        for i, kb in enumerate(tr.keep or []):
            for k, v in kb.items():
                add(f"train{wi}.keep{i}.{k}", v)
    for key, t in ops._scratch.items():
        add(f"scratch.{key[0]}", t)
    for i, t in enumerate(ops._sk_ws.values()):
        add(f"sk_ws{i}", t)
    return out


class Recorder:
    """Stands in for the ctypes handle `ops.lib()` returns: forwards every call and appends [name, return value, arguments]."""

    def __init__(self, real, signatures, ops):
        self.real, self.signatures, self.ops = real, signatures, ops
        self.model, self.calls, self.first_use = None, [], {}

    def _pointer(self, v, bufs):
        v = getattr(v, "value", v)
        if not v:
            return "null"
        for name, lo, size in bufs:
            if lo <= v < lo + size:
                return f"{name}+{v - lo}"
        if v not in self.first_use:            # (the second, third new address of one call: tmp<k>.1, tmp<k>.2)
            self.first_use[v] = f"tmp{len(self.calls)}" + (f".{self.fresh}" if self.fresh else "")
            self.fresh += 1
        return self.first_use[v]

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        argtypes = self.signatures[name][1]

        def call(*args):
            bufs = _buffers(self.model, self.ops) if self.model is not None else []
            self.fresh = 0
            rec = [self._pointer(a, bufs) if t is ctypes.c_void_p else (a if isinstance(a, (int, float)) else "struct")
                   for a, t in zip(args, argtypes)]
            assert len(args) == len(argtypes), name
            ret = fn(*args)
            self.calls.append([name, ret, rec])
            return ret

        return call


def run_pass(spec, monkeypatch):
    """The calls of one pass, in order."""
    from mixgrpo_amd import _lib, ops
    from mixgrpo_amd import flux_backward as FB
    from mixgrpo_amd.flux import FluxConfig, FluxTransformer2DModel
    keep = spec.get("keep")
    for name, v in zip(("KEEP_ACTS", "KEEP_FF", "KEEP_QKV"), keep or ()):
        monkeypatch.setattr(FB, name, v)
    rec = Recorder(_lib.lib(), _lib.SIGNATURES, ops)
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
        rec.model = m
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
        rec.model = None
        del m, inputs, x, ehs, pooled, ids, tids, t, gd, R
    monkeypatch.undo()
    ops._scratch.clear()
    ops._sk_ws.clear()
    del pool
    return rec.calls


def canonical(calls):
    return "\n".join(json.dumps(c) for c in calls)


def digest(calls):
    return dict(count=len(calls), sha256=hashlib.sha256(canonical(calls).encode()).hexdigest())


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["passes"]


@pytest.mark.parametrize("name", list(PASSES))
def test_launch_sequence_is_the_recorded_one(name, recorded, monkeypatch):
    calls = json.loads(json.dumps(run_pass(PASSES[name], monkeypatch)))
    want = recorded[name]
    if "calls" in want:
        for i, (got, exp) in enumerate(zip(calls, want["calls"])):
            assert got == exp, f"{name}: call {i} differs\n recorded: {exp}\n this code: {got}"
        assert len(calls) == len(want["calls"]), \
            f"{name}: {len(calls)} calls, recorded {len(want['calls'])}; first extra: {(calls + want['calls'])[min(len(calls), len(want['calls']))]}"
    else:
        assert digest(calls) == want, f"{name}: {digest(calls)} != recorded {want}"


if __name__ == "__main__":
    # record the fixture; run twice, the second time in the reverse order on a used allocator, to show that the record does not
    # depend on what ran before
    assert sys.argv[1:2] == ["--write"], "usage: python tests/test_hip_launch_trace.py --write [PATH]"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    first = {n: run_pass(s, pytest.MonkeyPatch()) for n, s in PASSES.items()}
    junk = [torch.empty(n, device="cuda") for n in (100, 5000, 70000, 300, 1 << 20)]
    del junk[::2]
    again = {n: run_pass(PASSES[n], pytest.MonkeyPatch()) for n in reversed(list(PASSES))}
    for n in PASSES:
        assert canonical(first[n]) == canonical(again[n]), f"{n}: the record is not reproducible within one process"
    out = {n: dict(calls=c) if PASSES[n].get("full", True) else digest(c) for n, c in first.items()}
    with open(path, "w") as f:
        f.write('{"passes": {\n' + ",\n".join(
            f'{json.dumps(n)}: ' + ('{"calls": [\n' + ",\n".join(json.dumps(c) for c in v["calls"]) + "\n]}" if "calls" in v
                                    else json.dumps(v)) for n, v in out.items()) + "\n}}\n")
    print({n: digest(c) for n, c in first.items()}, os.path.getsize(path))
