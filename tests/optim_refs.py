"""fp64 reference of one fused AdamW step (csrc/optim.hip: adamw_kernel) with the elementwise error budget of its fp32
evaluation, and index-hashed test data that is the same on the host and on the device.

The recurrence is torch.optim.AdamW's, with the scalars `AdamArgs` holds taken in double BEFORE their rounding to fp32:
    w <- w (1 - lr wd);  m <- m + (1 - b1)(g - m);  v <- v b2 + (1 - b2) g^2;
    w <- w - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).

BUDGET per step, in fp32 ulps (2^-23 of a term's magnitude, u = half an ulp), added to what the inputs already carry:
  m:  g - m (u |g - m| <= 1 ulp of max(|m|, |g|)), * (1 - b1) (its rounding and the product: 2 u of a term 0.1 |g - m|), the
      sum (u |m'|): below 0.8 ulp of max(|m|, |g|); held to 2 ulps.  The carried error shrinks by b1.
  v:  v * b2 (b2's rounding, the product: 2 u), (1 - b2) * g * g (rounding, two products: 3 u), the sum (u): every term is
      positive, so 4 u = 2 ulps of the new v; held to 3.  The carried error shrinks by b2.
  w:  w * decay (decay's rounding, the product) and the final subtraction: 1.5 ulps of |w|; held to 2.  The update
      lr' m / (sqrt(v) / bc + eps): sqrt (u), bc's rounding and the division (2 u), + eps (u), m / denom (u), lr' (2 u):
      3 ulps of the update; held to 6; plus half of v's relative error (the square root) and m's error times lr' / denom.
With lr = 1e-2 the update is ~1e-2 and |w| <= 0.05, so the whole budget is ~1e-8: an element the kernel skipped is off by 1e-2.
CPU-measured (tests/test_optim_host.py::test_fp32_torch_adamw_stays_inside_the_fp64_budget): fp32 torch.optim.AdamW (foreach)
uses at most 0.16 / 0.05 / 0.45 of the w / m / v budgets over two steps on the first 2^16 elements of the data below, and
0.48 / 0.25 / 0.36 from non-zero moments at steps 1000 and 100000."""
import math

import torch

ULP = 2.0 ** -23
F64 = torch.float64


def hashed(lo, hi, salt, device="cpu"):
    """Elements lo..hi-1 of an endless fp32 sequence, uniform in [-0.5, 0.5): an integer hash of the index, so any slice can
    be rebuilt anywhere, bit for bit."""
    h = (torch.arange(lo, hi, dtype=torch.int64, device=device) * 2654435761 + salt * 40503) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 73244475) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return (h.double() / 2.0 ** 32 - 0.5).float()


def adamw_ref_step(w, m, v, tol, g, lr, b1, b2, eps, wd, step):
    """One step, in place, on fp64 tensors w / m / v and their budgets tol = (tw, tm, tv) (zeros for exact inputs)."""
    tw, tm, tv = tol
    bc2_sqrt = math.sqrt(1.0 - b2 ** step)
    step_size = lr / (1.0 - b1 ** step)
    tm.mul_(b1).add_(2 * ULP * torch.maximum(m.abs(), g.abs()))
    tw.add_(2 * ULP * w.abs())
    w.mul_(1.0 - lr * wd)
    m.add_((1.0 - b1) * (g - m))
    v.mul_(b2).add_((1.0 - b2) * g * g)
    tv.mul_(b2).add_(3 * ULP * v)
    denom = v.sqrt() / bc2_sqrt + eps
    upd = step_size * m / denom
    tw.add_(upd.abs() * (6 * ULP + 0.5 * tv / v.clamp_min(1e-300)) + step_size * tm / denom)
    w.sub_(upd)


def zeros_like3(x):
    return tuple(torch.zeros_like(x, dtype=F64) for _ in range(3))


HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)     # lr 1e-2: a skipped element is off by 1e-2, the budget is ~1e-8


def adamw_data(lo, hi, device="cpu"):
    """(w0, g) of the large-buffer AdamW test, elements lo..hi-1: |w| <= 0.05, |g| <= 0.01."""
    return hashed(lo, hi, 1, device) * 0.1, hashed(lo, hi, 2, device) * 0.02


def torch_adamw_step(w, m, v, g, step, lr, b1, b2, eps, wd):
    """fp32 torch.optim.AdamW (foreach) from the state (m, v) after step - 1 steps: new (w, m, v)."""
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=True)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    p.grad = g.clone()
    opt.step()
    return p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
