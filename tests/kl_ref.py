"""TEST INFRASTRUCTURE ONLY: the KL penalty of a replayed Flow-GRPO step to a frozen reference policy (`--kl_ref_coeff`),
restated on the CPU oracle's step.

`oracle.solver.flow_grpo_step` returns the step's `mean` (4th) and `sd` (5th).  The policy's step and the reference policy's
are Gaussians of the same sd, so KL(N(mean, sd) || N(mean_ref, sd)) = (mean - mean_ref)^2 / (2 sd^2) per element, averaged
over the sample's elements like the log-prob.  The expression has the form of the quadratic term of `oracle.solver._gauss_logp`
-- a squared fp32 difference over `2 * (sd ** 2)`, then the mean -- so autograd walks it in the order `mgx_flow_step_kl_bwd`
does: grad / n, / den, * 2 (mean - mean_ref), summed with the log-prob's gradient at `mean`."""
import torch

from oracle import solver as O


def kl_to_reference(mean, mean_ref, sd):
    """kl [B] from the two steps' means (fp32 [B, ...]) and their common sd; `mean_ref` carries no gradient."""
    kl = ((mean - mean_ref.detach()) ** 2) / (2 * (sd ** 2))
    return kl.mean(dim=tuple(range(1, kl.ndim)))


def flow_grpo_step_kl(model_output, ref_model_output, latents, eta, sigmas, index, prev_sample):
    """(log_prob [B], kl [B]) of the replayed step: the oracle's step on both model outputs."""
    _, _, logp, mean, sd = O.flow_grpo_step(model_output, latents, eta, sigmas, index, prev_sample)
    with torch.no_grad():
        mean_ref = O.flow_grpo_step(ref_model_output, latents, eta, sigmas, index, prev_sample)[3]
    return logp, kl_to_reference(mean, mean_ref, sd)
