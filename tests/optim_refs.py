"""Float64 reference of the optimizer step of csrc/optim.hip: gradient 2-norm, clip coefficient, one AdamW update.  TEST
INFRASTRUCTURE, plain torch on the CPU; shares no code with optim.hip or with torch.optim.

  total_norm64(grads)            sqrt(sum g^2) over all tensors
  clip_coef64(total, max_norm)   min(1, max_norm / (total + 1e-6)); 1 when max_norm <= 0   (clip_grad_norm_'s coefficient)
  adamw_step64(...)              decoupled decay, the two moments, both bias corrections, the update; returns new p, m, v

The formulas are those of Loshchilov & Hutter, "Decoupled Weight Decay Regularization" (Algorithm 2) in the form torch.optim.AdamW
documents: eps is added to sqrt(v_hat), the decay multiplies the parameter by (1 - lr wd) before the update.
tests/test_optim_refs.py holds this file to torch.optim.AdamW in float64 on the host, negative controls included.
"""
import math

import torch


def total_norm64(grads):
    s = 0.0
    for g in grads:
        s += float((g.detach().double().cpu() ** 2).sum())
    return math.sqrt(s)


def clip_coef64(total, max_norm):
    if max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (total + 1e-6))


def adamw_step64(p, g, m, v, step, lr, betas, eps, wd, coef):
    """One AdamW update of one tensor in float64.  step: the count of THIS update (1 for the first), lr a float, coef the clip
    coefficient the gradient is multiplied with first.  Returns (p, m, v) after the update; the inputs are not modified."""
    beta1, beta2 = betas
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    g = g * coef
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    m_hat = m / (1.0 - beta1 ** step)
    v_hat = v / (1.0 - beta2 ** step)
    p = p - lr * m_hat / (v_hat.sqrt() + eps)
    return p, m, v
