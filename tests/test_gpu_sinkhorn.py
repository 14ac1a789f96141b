"""`ops.sinkhorn` (csrc/transport.hip: the Sinkhorn forward stopped by a flag on the device) against the loop of
GMW/lib/optimal_transport.py:52-75 restated in float64 below.

Yardstick: E_ref = max|P_stock - P_truth| / max P_truth, where P_stock is `RegularisedTransportFn.sinkhorn` in fp32 on the same
device in the same test.  The kernel is held to 2 E_ref: both are fp32 sums of n terms in different orders, and the factor covers
the order and no more.  Iteration counts are compared with the truth's only where the cap or the construction fixes them: at
tolerance 1e-9 they depend on the summation order.

Inputs: a = normalize(randn(B, m, 128)), b = normalize(a' + s randn) with a' = a cut or repeated to n rows, M = cdist(a, b) in
float64, rounded to fp32.  s = 1 converges in a few iterations, s = 0.05 (a near-diagonal plan) in 30 or more."""
import functools
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import transport_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
LMBDA, MAX_DISTANCE = 10.0, 5.0


@functools.lru_cache(maxsize=None)
def distances(B, m, n, s, seed=0):
    """(B, m, n) fp32 on the host; shared, do not modify."""
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(B, m, 128, dtype=torch.float64, generator=g), dim=-1)
    a2 = a.repeat(1, -(-n // m), 1)[:, :n]
    b = torch.nn.functional.normalize(a2 + s * torch.randn(B, n, 128, dtype=torch.float64, generator=g), dim=-1)
    return torch.cdist(a, b).float()


def marginals(M):
    b, m, n = M.shape
    return M.new_full((b, m), 1.0 / m), M.new_full((b, n), 1.0 / n)


def truth_plan(M32, tolerance, max_iterations):
    """The reference loop in float64 on M32's device -> (P, iterations)."""
    M = M32.double()
    r, c = marginals(M)
    K = torch.exp(-LMBDA * M.clamp_max(MAX_DISTANCE))
    Kt = K.transpose(-2, -1)
    r, c = r.unsqueeze(-1), c.unsqueeze(-1)
    u, previous, it = r.clone(), torch.ones_like(r), 0
    for _ in range(max_iterations):
        if bool(((u - previous).abs() <= tolerance).all()):
            break
        previous = u
        u = r / K.matmul(c / Kt.matmul(u))
        it += 1
    v = c / Kt.matmul(u)
    return (u * K) * v.transpose(-2, -1), it


def relative_error(P, truth):
    return ((P.double() - truth).abs().max() / truth.max()).item()


def sums_error(P, truth):
    rows = ((P.double().sum(-1) - truth.sum(-1)).abs().max() / truth.sum(-1).max()).item()
    cols = ((P.double().sum(-2) - truth.sum(-2)).abs().max() / truth.sum(-2).max()).item()
    return rows, cols


def run_case(cuda, M_host, truth_args, tolerance=1e-9, max_iterations=100):
    """Kernel, stock path and truth on one input -> the figures, printed before anybody asserts."""
    from dcd_amd import ops
    from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T
    M = M_host.to(cuda)
    r, c = marginals(M)
    truth, truth_it = truth_plan(M, *truth_args)
    stock = T.sinkhorn(M, r, c, LMBDA, tolerance, max_iterations)
    P, it = ops.sinkhorn(M, r, c, LMBDA, tolerance, max_iterations)
    out = SimpleNamespace(P=P, truth=truth, iterations=int(it), truth_iterations=truth_it, e_ref=relative_error(stock, truth),
                          e=relative_error(P, truth), sums=sums_error(P, truth), stock_sums=sums_error(stock, truth))
    print("sinkhorn %s tol %g cap %d: kernel %d iterations (truth %d), E %.3e, E_ref %.3e, row/col sums %.3e %.3e (stock %.3e %.3e)"
          % (tuple(M.shape), tolerance, max_iterations, out.iterations, truth_it, out.e, out.e_ref, *out.sums, *out.stock_sums))
    return out


def hold(o):
    assert torch.isfinite(o.P).all()
    assert o.e <= 2 * o.e_ref, "plan: %.3e against 2 x %.3e" % (o.e, o.e_ref)
    assert max(o.sums) <= 2 * o.e_ref, "row / column sums: %.3e %.3e against 2 x %.3e" % (*o.sums, o.e_ref)


@pytest.mark.parametrize("B,m,n,s", [(2, 64, 64, 1.0), (3, 101, 101, 1.0), (2, 48, 80, 1.0), (2, 2628, 2628, 0.05)])
def test_converged_plan(cuda, B, m, n, s):
    o = run_case(cuda, distances(B, m, n, s), (1e-15, 1000))
    assert 1 <= o.iterations < 100
    hold(o)


def test_cap_of_100_iterations(cuda):
    o = run_case(cuda, distances(2, 256, 256, 0.05), (0.0, 100))
    assert o.truth_iterations == 100 and o.iterations == 100
    hold(o)


@pytest.mark.parametrize("cap", [3, 0])
def test_small_caps(cuda, cap):
    o = run_case(cuda, distances(2, 256, 256, 0.05), (0.0, cap), max_iterations=cap)
    assert o.truth_iterations == cap and o.iterations == cap
    hold(o)


@pytest.mark.parametrize("n", [64, 2628])
def test_constant_distances_stop_after_one_iteration(cuda, n):
    M = torch.full((2, n, n), 0.7)
    o = run_case(cuda, M, (1e-3, 100), tolerance=1e-3)
    assert o.iterations == 1 and o.truth_iterations == 1
    hold(o)
    uniform = 1.0 / (n * n)
    worst = ((o.P.double() - uniform).abs().max() / uniform).item()
    print("constant M, n = %d: |P - 1/(m n)| / (1/(m n)) = %.3e, 2 E_ref = %.3e" % (n, worst, 2 * o.e_ref))
    assert worst <= 2 * o.e_ref


def same_bits(a, b):
    return bool(R.same_bits(a.cpu(), b.cpu()).all())


@pytest.mark.parametrize("B,m,n,s", [(3, 101, 101, 1.0), (2, 48, 80, 1.0), (2, 2628, 2628, 0.05)])
def test_two_calls_give_the_same_bits(cuda, B, m, n, s):
    from dcd_amd import ops
    M = distances(B, m, n, s).to(cuda)
    r, c = marginals(M)
    P1, it1 = ops.sinkhorn(M, r, c, LMBDA, 1e-9, 100)
    P2, it2 = ops.sinkhorn(M, r, c, LMBDA, 1e-9, 100)
    assert int(it1) == int(it2) and same_bits(P1, P2)


@pytest.mark.parametrize("m,n", [(101, 101), (48, 80), (300, 1100)])
def test_an_objects_plan_does_not_depend_on_its_place(cuda, m, n):
    """Object 0 alone, as the first of a batch and as the last of a batch, wherever the members run the same number of iterations:
    under a cap that every member reaches, and beside a copy of itself under the natural stop."""
    from dcd_amd import ops
    M = distances(3, m, n, 0.05).to(cuda)
    r, c = marginals(M)
    alone, it = ops.sinkhorn(M[:1], r[:1], c[:1], LMBDA, 0.0, 5)
    first, it_first = ops.sinkhorn(M, r, c, LMBDA, 0.0, 5)
    back = M.flip(0).contiguous()
    last, it_last = ops.sinkhorn(back, r, c, LMBDA, 0.0, 5)
    assert int(it) == int(it_first) == int(it_last) == 5
    assert same_bits(alone[0], first[0]) and same_bits(alone[0], last[2])
    alone, it = ops.sinkhorn(M[:1], r[:1], c[:1], LMBDA, 1e-9, 100)
    twice, it_twice = ops.sinkhorn(M[:1].repeat(2, 1, 1), r[:2], c[:2], LMBDA, 1e-9, 100)
    assert int(it) == int(it_twice)
    assert same_bits(alone[0], twice[0]) and same_bits(alone[0], twice[1])


@pytest.mark.parametrize("m,n", [(64, 64), (37, 1028), (5, 3500), (9, 4100)])
def test_four_byte_accesses_give_the_same_bits(cuda, m, n):
    """n % 4 == 0 with M four bytes off a 16-byte boundary takes the 4-byte route; n = 4100 is past what a strip keeps in
    registers (4096 columns), so both routes of that kernel are covered as well."""
    from dcd_amd import ops
    M = distances(2, m, n, 1.0).to(cuda)
    r, c = marginals(M)
    assert M.data_ptr() % 16 == 0
    shifted = torch.empty(M.numel() + 1, dtype=torch.float32, device=cuda)[1:].view_as(M).copy_(M)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    P, it = ops.sinkhorn(M, r, c, LMBDA, 1e-9, 100)
    Q, it_q = ops.sinkhorn(shifted, r, c, LMBDA, 1e-9, 100)
    differ = ~R.same_bits(P.cpu(), Q.cpu())
    print("sinkhorn (2, %d, %d), 16-byte against 4-byte accesses: %d of %d elements differ, by at most %.3e of the largest"
          % (m, n, int(differ.sum()), differ.numel(), ((P - Q).abs().max() / P.max()).item()))
    assert int(it) == int(it_q) and not differ.any()
    truth, _ = truth_plan(M, 1e-15, 1000)
    from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T
    e_ref, e = relative_error(T.sinkhorn(M, r, c, LMBDA, 1e-9, 100), truth), relative_error(P, truth)
    print("sinkhorn (2, %d, %d): %d iterations, E %.3e, E_ref %.3e" % (m, n, int(it), e, e_ref))
    assert e <= 2 * e_ref


def test_bad_arguments_are_refused(cuda):
    from dcd_amd import _lib, ops
    M = torch.rand(2, 8, 8, device=cuda)
    r, c = marginals(M)
    with pytest.raises(_lib.DcdHipError):
        ops.sinkhorn(M, r, c, LMBDA, 1e-9, -1)
    with pytest.raises(_lib.DcdHipError):
        ops.sinkhorn(M, r, c, LMBDA, 1e-9, 5000)
    with pytest.raises(RuntimeError):
        ops.sinkhorn(M, r[:, :7], c)
    with pytest.raises(_lib.DcdHipError):
        ops.sinkhorn(M.cpu(), r.cpu(), c.cpu())


@pytest.mark.parametrize("b,m,n", [(2, 5, 4), (3, 100, 132), (2, 260, 260)])
def test_gradients_through_the_layer_equal_the_default_paths(cuda, b, m, n):
    """`device_sinkhorn=True` changes the forward only: the backward reads a plan that differs by its rounding, so the two gradients
    agree to the bound tests/transport_refs.py gives the device backward (4e-7 cond(S) max|ref|)."""
    from dcd_amd.gmw.optimal_transport import RegularisedTransport
    p = R.transport_problem(b, m, n)
    M0 = torch.rand(b, m, n, dtype=torch.float64, generator=torch.Generator().manual_seed(11)).float()     # transport_problem's M
    W = p.v.reshape(b, m, n).float().to(cuda)
    grads, plans = [], []
    for device_sinkhorn in (False, True):
        layer = RegularisedTransport(R.LMBDA, 1e-9, 100, device_sinkhorn=device_sinkhorn)
        M = M0.to(cuda).requires_grad_()
        r, c = marginals(M.detach())
        P = layer(M, r, c, positive_marginals=device_sinkhorn)
        (P * W).sum().backward()
        grads.append(M.grad.double().cpu())
        plans.append(P.detach())
    bound = R.solver_bound(p.cond, p.ref)
    diff = (grads[0] - grads[1]).abs().max().item()
    print("transport gradient (%d, %d, %d): |device - default| %.3e, bound %.3e, plans differ by %.3e of their maximum"
          % (b, m, n, diff, bound, relative_error(plans[1], plans[0].double())))
    assert torch.isfinite(grads[1]).all() and diff <= bound
