"""Host-side LR schedules (mixgrpo_amd/optim.py `get_scheduler`) = the reference's `get_scheduler(args.lr_scheduler, ...)`
(fastvideo/train_grpo_flux.py:726-734; diffusers' optimization.py, absent here).  The pin that IS available: transformers'
same-named LambdaLR schedules (diffusers' file is a copy of them), stepped side by side on a torch optimizer."""
import pytest
import torch

from mixgrpo_amd.optim import SCHEDULER_NAMES, get_scheduler


class _Opt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def _theirs(name, opt, warmup, total, num_cycles, power):
    from transformers import optimization as TO
    if name == "constant":
        return TO.get_constant_schedule(opt)
    if name == "constant_with_warmup":
        return TO.get_constant_schedule_with_warmup(opt, warmup)
    if name == "linear":
        return TO.get_linear_schedule_with_warmup(opt, warmup, total)
    if name == "cosine":
        return TO.get_cosine_schedule_with_warmup(opt, warmup, total)                 # diffusers passes no num_cycles here
    if name == "cosine_with_restarts":
        return TO.get_cosine_with_hard_restarts_schedule_with_warmup(opt, warmup, total, num_cycles=num_cycles)
    return TO.get_polynomial_decay_schedule_with_warmup(opt, warmup, total, lr_end=1e-7, power=power)


@pytest.mark.parametrize("name", SCHEDULER_NAMES)
@pytest.mark.parametrize("warmup,total,num_cycles,power", [(0, 1000000, 1, 1.0), (5, 40, 3, 2.0), (3, 20, 1, 1.0)])
def test_schedules_follow_the_reference_formulas(name, warmup, total, num_cycles, power):
    lr = 1e-5
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.AdamW([p], lr=lr)
    theirs = _theirs(name, topt, warmup, total, num_cycles, power)
    mine = get_scheduler(name, _Opt(lr), num_warmup_steps=warmup, num_training_steps=total, num_cycles=num_cycles, power=power)
    for step in range(60):
        assert mine.get_last_lr()[0] == pytest.approx(theirs.get_last_lr()[0], rel=1e-12, abs=1e-20), (name, step)
        topt.step()
        theirs.step()
        mine.step()


def test_unknown_name_fails_with_the_list():
    with pytest.raises(ValueError, match="constant_with_warmup"):
        get_scheduler("piecewise_constant", _Opt(1e-5))


def test_fp32_torch_adamw_stays_inside_the_fp64_budget():
    """The premise of tests/test_hip_optim.py's elementwise AdamW bounds (derived in tests/optim_refs.py): a plain fp32
    evaluation -- torch.optim.AdamW (foreach) on the first 2^16 elements of the same data -- stays inside the budget around
    the fp64 recurrence, over two steps from zero moments and from non-zero moments at large step counts."""
    import optim_refs as R
    n = 1 << 16
    w0, g = R.adamw_data(0, n)
    worst = [0.0, 0.0, 0.0]

    def compare(got, ref, tol, k):
        for i, (a, b, t) in enumerate(zip(got, ref, tol)):
            frac = ((a.double() - b).abs() / t.clamp_min(1e-300)).max().item()
            assert frac <= 1.0, (k, "wmv"[i], frac)
            worst[i] = max(worst[i], frac)

    w, m, v = w0, torch.zeros(n), torch.zeros(n)
    ref, tol = [w0.double(), torch.zeros(n, dtype=R.F64), torch.zeros(n, dtype=R.F64)], R.zeros_like3(w0)
    for step in (1, 2):
        w, m, v = R.torch_adamw_step(w, m, v, g, step, **R.HP)
        R.adamw_ref_step(*ref, tol, g.double(), step=step, **R.HP)
        compare((w, m, v), ref, tol, step)
    print("two steps, fp32 torch / budget (w, m, v):", [round(x, 3) for x in worst])
    worst = [0.0, 0.0, 0.0]
    m0, v0 = R.hashed(0, n, 3) * 0.01, (R.hashed(0, n, 4) + 0.5) * 1e-4
    for step in (1000, 100000):
        got = R.torch_adamw_step(w0, m0, v0, g, step, **R.HP)
        ref, tol = [w0.double(), m0.double(), v0.double()], R.zeros_like3(w0)
        R.adamw_ref_step(*ref, tol, g.double(), step=step, **R.HP)
        compare(got, ref, tol, step)
    print("late steps, fp32 torch / budget (w, m, v):", [round(x, 3) for x in worst])
