"""Shared test helpers: fixture loading, exact-grid operands, process groups, the C-ABI call recorder of the launch traces."""
import ctypes
import hashlib
import json
import os

from safetensors.torch import load_file

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    tensors = load_file(os.path.join(GOLDEN, name + ".safetensors"))
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    return tensors, meta


def host_matches_fixture_host():
    """torch's CPU scalar math (sqrt/log of 0-dim tensors) is not bit-stable across hosts: the fixtures carry the
    generating host's last bits.  True when this host reproduces them (then comparisons are bit-exact)."""
    import torch
    t, _ = load_golden("solver_steps")
    sig = t["sigma/shift3.0_T25"]
    s, dt = sig[2], sig[3] - sig[2]
    std = torch.sqrt(s / (1 - s)) * 0.7
    return (1 + std ** 2 / (2 * s) * dt).item() == 0.8668485283851624 and \
        torch.log(std * torch.sqrt(-1 * dt)).item() == -0.6758469939231873


def assert_same(a, b, exact=True, rtol=2e-6, atol=2e-6):
    """Bit-exact comparison (NaNs equal), or a few-ulp tolerance when `exact` is False."""
    import torch
    a = a.detach().cpu()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    if exact:
        assert torch.equal(torch.nan_to_num(a, nan=777.0), torch.nan_to_num(b, nan=777.0)), (a - b).abs().max()
    else:
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin & ~torch.isnan(b)], b[~fin & ~torch.isnan(b)])
        assert torch.allclose(a[fin].float(), b[fin].float(), rtol=rtol, atol=atol), (a[fin].float() - b[fin].float()).abs().max()


def grid(shape, lo, hi, div, gen, dtype=None, device="cuda"):
    """randint(lo, hi) / div: operands of the exact-sum tests.  With small integers over a power of two every partial sum is
    exact in fp32, so a kernel must give the fp64 result bit for bit in whatever order it adds."""
    import torch
    x = torch.randint(lo, hi, shape, generator=gen, device=device).to(torch.float32) / div
    return x.to(torch.bfloat16 if dtype is None else dtype)


def sentinel(shape, device="cuda"):
    """A bf16 tensor whose bit patterns run 1 .. 251 (denormals): non-zero everywhere and no value of any `grid`, for
    pre-filling buffers whose untouched or zero-filled parts a test checks."""
    import math

    import torch
    return (torch.arange(math.prod(shape), device=device) % 251 + 1).to(torch.int16).view(torch.bfloat16).view(shape)


# ---- the exact GEMM tests (test_hip_gemm_handover.py, test_hip_gemm_small.py): operands on a grid whose sums are exact in fp32
GCOLS, GROWS = 8, 3  # guard columns right of every row, guard rows below every batch


def grid_ints(shape, lo, hi, div, gen):
    """randint(lo .. hi inclusive) / div as bf16, on the CPU"""
    import torch
    return (torch.randint(lo, hi + 1, shape, generator=gen).float() / div).bfloat16()


def exact_gemm_problem(Mr, Nr, K):
    """(A [Mr, K], W [Nr, K], bias [Nr], acc = A @ W^T in fp32 -- exact) on the CPU: A in multiples of 1/8 up to 1/2, W in
    multiples of 1/4 up to 1/2, so every product and partial sum is a multiple of 1/32 below 2^24 / 32 (asserted)."""
    import torch
    g = torch.Generator().manual_seed(Mr + 3 * Nr + K)
    A = grid_ints((Mr, K), -4, 4, 8, g)
    W = grid_ints((Nr, K), -2, 2, 4, g)
    bias = grid_ints((Nr,), -16, 16, 32, g)
    acc = A.float() @ W.float().t()
    assert float(acc.abs().max()) * 32 < 2 ** 24
    return A, W, bias, acc


class GuardedOut:
    """A row-batched (or plain: rpb None) output matrix with guard rows and columns, and the bookkeeping to check them."""

    def __init__(self, Mr, N, rpb, dtype, gen):
        import torch
        from mixgrpo_amd.ops import Rows
        self.M, self.N, self.rpb = Mr, N, rpb or Mr
        self.ld = N + GCOLS
        nb = (Mr + self.rpb - 1) // self.rpb
        cg = torch.Generator(device="cuda").manual_seed(int(torch.randint(0, 2 ** 31, (1,), generator=gen)))
        self.init = (torch.randint(-64, 65, (nb, self.rpb + GROWS, self.ld), generator=cg, device="cuda").float() / 32).to(dtype)
        self.store = self.init.clone()
        self.rows = Rows(self.store, Mr, self.ld, self.rpb if rpb else 1 << 40, (self.rpb + GROWS) * self.ld if rpb else 0)
        bi, ri = torch.arange(nb)[:, None], torch.arange(self.rpb + GROWS)[None, :]
        row_ok = (ri < self.rpb) & (bi * self.rpb + ri < Mr)                  # [batch, row]: a row of the matrix
        owned = row_ok[:, :, None] & (torch.arange(self.ld) < N)[None, None, :]
        self.guard = (~owned).cuda()

    def dense(self, t=None):
        t = self.store if t is None else t
        return t[:, :self.rpb, :self.N].reshape(-1, self.N)[:self.M]

    def reset(self):
        self.store.copy_(self.init)

    def guards_untouched(self):
        import torch
        return torch.equal(self.store[self.guard], self.init[self.guard])

    def batch_of_row(self):
        import torch
        return torch.arange(self.M) // self.rpb


def same_bits(got, want):
    """bit-for-bit on the CPU (bf16 / fp32 compared as integers: -0.0 != 0.0, and a NaN cannot hide)"""
    import torch
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape
    same = torch.equal(got.view(it), want.view(it))
    if not same:
        bad = (got.view(it) != want.view(it)).nonzero()
        raise AssertionError(f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} "
                             f"want {want[tuple(bad[0])].item()}")


def linear_ref(acc, bias, N, with_bias):
    """bf16(acc + bias): the Linear's output"""
    return (acc[:, :N] + bias[:N].float()).bfloat16() if with_bias else acc[:, :N].bfloat16()


def oracle_flux(cfg, P, device=None):
    """oracle/mmdit.forward behind the transformer call signature, parameters trainable (fp32 master weights; the
    restatement rounds to bf16 where autocast does).  Used by the end-to-end tests on both the CPU and the GPU side.
    `device`: run the MMDiT restatement's (device-agnostic, plain fp32 torch) arithmetic there -- parameters on that device,
    inputs moved over, the output moved back -- while the trainer oracle around it stays on the host: what makes the
    full-width, many-block cases affordable inside the suite's time limit (the host pass of a 2.5 B-parameter train step took
    100-340 s depending on the box).  None: everything on the host."""
    import torch
    from oracle import mmdit as OM

    class OracleFlux(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg, self.names = cfg, list(P)
            self.params = torch.nn.ParameterList([torch.nn.Parameter(P[k].clone() if device is None else P[k].to(device))
                                                  for k in self.names])
            self.config = {"oracle": True}

        def forward(self, hidden_states, encoder_hidden_states, timestep, guidance, txt_ids, pooled_projections, img_ids,
                    joint_attention_kwargs=None, return_dict=False):
            Pd = dict(zip(self.names, self.params))
            f = (lambda x: x.float()) if device is None else (lambda x: x.float().to(device))
            out = OM.forward(Pd, self.cfg, f(hidden_states), f(encoder_hidden_states), f(timestep), f(guidance), f(txt_ids),
                             f(pooled_projections), f(img_ids))
            out = out.to(torch.bfloat16)
            return (out if device is None else out.cpu(),)

        def clip_grad_norm_(self, max_norm):
            n = torch.nn.utils.clip_grad_norm_(self.parameters(), max_norm)
            return n if device is None else n.cpu()

    return OracleFlux()


def small_cfg(layers=1, singles=1):
    return dict(num_layers=layers, num_single_layers=singles, attention_head_dim=128, num_attention_heads=4,
                joint_attention_dim=64, pooled_projection_dim=32)


def make_inputs(B, hgrid, wgrid, L, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    N = hgrid * wgrid
    x = torch.randn(B, N, 64, generator=g)
    ehs = torch.randn(B, L, 64, generator=g).bfloat16()
    pooled = torch.randn(B, 32, generator=g).bfloat16()
    ids = torch.zeros(hgrid, wgrid, 3)
    ids[..., 1] += torch.arange(hgrid)[:, None]
    ids[..., 2] += torch.arange(wgrid)[None]
    ids = ids.reshape(N, 3)
    t = torch.tensor([0.954, 0.5, 0.123][:B] if B <= 3 else [0.954] * B)
    return x, ehs, pooled, ids, torch.zeros(L, 3), t, torch.tensor([3.5]).bfloat16()


def free_port():
    """A TCP port the kernel just handed out (bind to port 0): distinct per call, whatever the pytest pid is."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(worker, world, timeout=300, extra=()):
    """Start `worker(rank, world, port, queue, *extra)` as `world` daemon processes, collect one queue item per rank and
    ALWAYS reap the children: a rank that fails can neither hang the collection (bounded `get`) nor pytest's exit (daemon
    processes, terminate() + join() in `finally`).  Returns the items sorted by their first field (the rank)."""
    import queue as _queue

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + tuple(extra), daemon=True) for r in range(world)]
    try:
        for p in procs:
            p.start()
        out = []
        for _ in procs:
            try:
                out.append(q.get(timeout=timeout))
            except _queue.Empty:
                codes = [p.exitcode for p in procs]
                raise AssertionError(f"a rank produced no result within {timeout} s (exit codes so far: {codes})")
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, f"rank exited with {p.exitcode}"
        return sorted(out, key=lambda t: t[0])
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()


class Recorder:
    """Stands in for the ctypes handle `ops.lib()` returns: forwards every call and appends [name, return value, arguments].
    Pointers (the `c_void_p` arguments of `signatures`) are named `<buffer>+<byte offset>` after the buffer they fall into, of
    those that `buffers()` lists as (name, address, bytes) at the time of the call -- `buffers` is None while nothing is to
    be named -- and any other address is a temporary, `tmp<k>` with k the index of the first call that used that exact
    address (`tmp<k>.<j>` for the further new addresses of that call)."""

    def __init__(self, real, signatures):
        self.real, self.signatures = real, signatures
        self.buffers, self.calls, self.first_use = None, [], {}

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
            bufs = self.buffers() if self.buffers is not None else []
            self.fresh = 0
            rec = [self._pointer(a, bufs) if t is ctypes.c_void_p else (a if isinstance(a, (int, float)) else "struct")
                   for a, t in zip(args, argtypes)]
            assert len(args) == len(argtypes), name
            ret = fn(*args)
            self.calls.append([name, ret, rec])
            return ret

        return call


def tensor_extents(named):
    """(name, address, bytes) of those of the (name, value) pairs that are non-empty device tensors: a Recorder's buffers."""
    import torch
    return [(name, t.data_ptr(), t.numel() * t.element_size()) for name, t in named
            if isinstance(t, torch.Tensor) and t.is_cuda and t.numel()]


def scratch_buffers(ops):
    """ops' own caches, as the launch traces name them"""
    return [(f"scratch.{key[0]}", t) for key, t in ops._scratch.items()] + \
        [(f"sk_ws{i}", t) for i, t in enumerate(ops._sk_ws.values())]


def trace_canonical(calls):
    return "\n".join(json.dumps(c) for c in calls)


def trace_digest(calls):
    return dict(count=len(calls), sha256=hashlib.sha256(trace_canonical(calls).encode()).hexdigest())


def assert_trace(name, calls, want):
    """`calls` of pass `name` against its fixture entry: call for call where the fixture holds them, else count and sha256."""
    calls = json.loads(json.dumps(calls))
    if "calls" in want:
        for i, (got, exp) in enumerate(zip(calls, want["calls"])):
            assert got == exp, f"{name}: call {i} differs\n recorded: {exp}\n this code: {got}"
        assert len(calls) == len(want["calls"]), \
            f"{name}: {len(calls)} calls, recorded {len(want['calls'])}; first extra: {(calls + want['calls'])[min(len(calls), len(want['calls']))]}"
    else:
        assert trace_digest(calls) == want, f"{name}: {trace_digest(calls)} != recorded {want}"


def record_traces(path, passes, run_pass):
    """Write a launch-trace fixture: every pass of `passes` (name -> spec; spec["full"] False: count and sha256 only) through
    `run_pass(spec, monkeypatch)`, twice, the second time in the reverse order on a used allocator, to show that the record
    does not depend on what ran before."""
    import pytest
    import torch
    first = {n: run_pass(s, pytest.MonkeyPatch()) for n, s in passes.items()}
    junk = [torch.empty(n, device="cuda") for n in (100, 5000, 70000, 300, 1 << 20)]
    del junk[::2]
    again = {n: run_pass(passes[n], pytest.MonkeyPatch()) for n in reversed(list(passes))}
    for n in passes:
        assert trace_canonical(first[n]) == trace_canonical(again[n]), f"{n}: the record is not reproducible within one process"
    out = {n: dict(calls=c) if passes[n].get("full", True) else trace_digest(c) for n, c in first.items()}
    with open(path, "w") as f:
        f.write('{"passes": {\n' + ",\n".join(
            f'{json.dumps(n)}: ' + ('{"calls": [\n' + ",\n".join(json.dumps(c) for c in v["calls"]) + "\n]}" if "calls" in v
                                    else json.dumps(v)) for n, v in out.items()) + "\n}}\n")
    print({n: trace_digest(c) for n, c in first.items()}, os.path.getsize(path))
