"""tests/optim_refs.py against torch.optim.AdamW (float64, CPU, not fused) after torch.nn.utils.clip_grad_norm_: four steps over
tensors of 1, 5 and 4097 elements, one of which gets no gradient in one step (its step counter then lags the others', so its bias
corrections differ), with the clip active in some steps and not in others.  Agreement to 1e-12 of each tensor's largest value -- both
sides are float64 and differ in the order of a handful of operations (lerp against b m + (1 - b) g, m / bc1 against lr / bc1), i.e.
a few units of 2^-53 = 1.1e-16 per step.  The negative controls are wrong references: they must MISS that bound, or the bound
would hold nothing."""
import pytest
import torch

import optim_refs

SIZES = (1, 5, 4097)
LR, BETAS, EPS, WD, MAX_NORM = 1e-3, (0.9, 0.99), 1e-8, 1e-2, 15.0
BOUND = 1e-12


def _wrong_exponent(p, g, m, v, step, lr, betas, eps, wd, coef):
    """Bias corrections of the step before (the counter read before it is advanced)."""
    return optim_refs.adamw_step64(p, g, m, v, step + 1, lr, betas, eps, wd, coef)


def _decay_after_update(p, g, m, v, step, lr, betas, eps, wd, coef):
    """The decay applied to the updated parameter instead of the one the step started from."""
    q, m1, v1 = optim_refs.adamw_step64(p, g, m, v, step, lr, betas, eps, 0.0, coef)
    return q * (1.0 - lr * wd), m1, v1


def _worst_distance(step_fn):
    """Largest distance (relative to the library tensor's largest value) between `step_fn` and the library over four steps."""
    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in SIZES]
    opt = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=False, foreach=False)
    state = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), step=0) for p in params]
    worst = 0.0
    clipped = []
    for it in range(4):
        scale = (0.01, 30.0, 1.0, 0.3)[it]                      # norms of about 0.6, 1900, 64 and 19: clip off, on, on, on
        grads = [None if (it == 1 and i == 1) else torch.randn(n, generator=gen, dtype=torch.float64) * scale for i, n in enumerate(SIZES)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        have = [g for g in grads if g is not None]
        total = optim_refs.total_norm64(have)
        coef = optim_refs.clip_coef64(total, MAX_NORM)
        clipped.append(coef < 1.0)
        lib_total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        assert abs(total - float(lib_total)) <= BOUND * float(lib_total)
        opt.step()
        for p, g, s in zip(params, grads, state):
            if g is None:
                continue
            s["step"] += 1
            s["p"], s["m"], s["v"] = step_fn(s["p"], g, s["m"], s["v"], s["step"], LR, BETAS, EPS, WD, coef)
            assert float(opt.state[p]["step"]) == s["step"]
            assert (p.grad - g * coef).abs().max().item() <= BOUND * g.abs().max().item()
            for mine, lib in ((s["p"], p.detach()), (s["m"], opt.state[p]["exp_avg"]), (s["v"], opt.state[p]["exp_avg_sq"])):
                worst = max(worst, (mine - lib).abs().max().item() / lib.abs().max().item())
    assert clipped == [False, True, True, True]
    assert [s["step"] for s in state] == [4, 3, 4]              # the tensors' step counters differ
    return worst


def test_reference_equals_the_library_in_float64():
    worst = _worst_distance(optim_refs.adamw_step64)
    print("reference against torch.optim.AdamW (float64): %.3e" % worst)
    assert worst <= BOUND


@pytest.mark.parametrize("wrong", [_wrong_exponent, _decay_after_update])
def test_a_wrong_reference_misses_the_bound(wrong):
    worst = _worst_distance(wrong)
    print("%s against torch.optim.AdamW (float64): %.3e" % (wrong.__name__, worst))
    assert worst > 100 * BOUND


def test_norm_and_coefficient():
    g = [torch.tensor([3.0]), torch.tensor([[4.0, 12.0]])]
    assert optim_refs.total_norm64(g) == 13.0
    assert optim_refs.clip_coef64(13.0, 0.0) == 1.0 and optim_refs.clip_coef64(13.0, -1.0) == 1.0
    assert optim_refs.clip_coef64(13.0, 26.0) == 1.0
    assert optim_refs.clip_coef64(13.0, 6.5) == 6.5 / (13.0 + 1e-6)
