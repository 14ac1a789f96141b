"""tests/transport_refs.py on the host: the references and bounds that the GPU tests of dcd_sgemm, ops.schur_lower and the
transport layer's backward rely on, held to plain fp32 products on the CPU.  A bound that an honest fp32 product misses would
be wrong, and one that it never comes near would check nothing."""
import pytest
import torch

import transport_refs as R
from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T


def test_gemm_cases_cover_what_the_kernel_distinguishes():
    cases = R.GEMM_CASES
    assert {(c.ak, c.bk) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for kc in (0, 1):
        assert {c.K for c in cases if c.M == 5 and c.ak == c.bk == kc} == {1, 3, 16, 17, 33}
    assert {(c.M, c.N, c.K) for c in cases} >= {(128, 128, 16), (129, 1, 20), (1, 129, 20), (261, 260, 128), (300, 300, 99)}
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        p = R.gemm_problem(c)
        assert p.lda % 4 == 0 and p.ldb % 4 == 0 and p.strideA % 4 == 0 and p.strideB % 4 == 0 and p.a_off % 4 == 0 and p.b_off % 4 == 0
        assert p.ldc > c.N and p.c_off >= 2 * p.ldc and p.c_buf.numel() == p.c_off + c.Z * p.strideC + 2 * p.ldc
        assert not torch.isnan(p.A).any() and not torch.isnan(p.B).any()
        if c.name == "schur-form":
            assert p.strideA > c.K * p.lda
        if c.name.startswith("c-4-byte"):
            assert p.c_off % 4 == 1 and p.ldc % 4 != 0


def test_lower_tile_mask_is_the_kernels_skip_rule():
    w = R.lower_tile_mask(261, 260)
    for m0 in range(0, 261, R.TILE):
        for n0 in range(0, 260, R.TILE):
            tile = w[m0:m0 + R.TILE, n0:n0 + R.TILE]
            assert bool(tile.all()) == (n0 < m0 + R.TILE) and bool(tile.any()) == (n0 < m0 + R.TILE)
    assert w[0, 127] and not w[127, 128] and w[128, 255] and w[260, 259]


def test_gemm_bound_holds_for_fp32_host_products_and_is_not_vacuous():
    worst = 0.0
    for c in R.GEMM_CASES:
        p = R.gemm_problem(c)
        host = torch.tensor(c.alpha, dtype=torch.float32) * p.A.matmul(p.B)
        after = p.c_buf.clone()
        out = R.gemm_result(p, after)
        new = host + out if c.accumulate else host
        out.copy_(torch.where(p.written.expand_as(new), new, out))
        worst = max(worst, R.gemm_check(p, after, "host fp32"))
    assert 0.01 <= worst <= 1.0, worst


def test_gemm_check_refuses_what_it_is_there_to_refuse():
    c = next(c for c in R.GEMM_CASES if c.name == "trailing-lower1")
    p = R.gemm_problem(c)
    ref, _ = R.gemm_reference(p)
    good = p.c_buf.clone()
    out = R.gemm_result(p, good)
    out.copy_(torch.where(p.written.expand_as(out), ref.float(), out))
    R.gemm_check(p, good, "rounded reference")
    bad = good.clone()
    R.gemm_result(p, bad)[1, 200, 3] *= 1 + 1e-4                       # one element off by 1e-4 relative
    with pytest.raises(AssertionError, match="ratio"):
        R.gemm_check(p, bad, "one element off")
    bad = good.clone()
    R.gemm_result(p, bad)[0, 5, 130] = 0.0                             # a write into a skipped tile
    with pytest.raises(AssertionError, match="outside the written region"):
        R.gemm_check(p, bad, "skipped tile written")
    bad = good.clone()
    bad[p.c_off + c.N] = 1.0                                           # a write into the padding of row 0
    with pytest.raises(AssertionError, match="outside the written region"):
        R.gemm_check(p, bad, "padding written")


@pytest.mark.parametrize("shape", R.TRANSPORT_SHAPES)
def test_schur_bound_and_solver_bound_hold_for_the_fp32_host_branch(shape):
    """The plain fp32 host product of the Schur term within the section's bound (measured: at most 0.29 of it), and the fp32 LAPACK
    branch of `gradient` within 4e-7 cond(S) max|ref| (measured error / max|ref| and cond(S) per shape, generator seeded 11:
    (2, 5, 4) 1.7e-6 at cond 22, (3, 100, 132) 5.8e-7 at 105, (2, 260, 260) 5.4e-7 at 265, (1, 385, 384) 1.0e-6 at 389,
    (2, 131, 516) 1.3e-7 at 136)."""
    b, m, n = shape
    tp = R.transport_problem(b, m, n)
    G, inv_rows, cols = R.schur_inputs(tp.P32)
    ref, bound = R.schur_reference(G, inv_rows, cols)
    S32 = -G.transpose(1, 2).matmul(inv_rows.unsqueeze(-1) * G)
    S32.diagonal(dim1=-2, dim2=-1).add_(cols)
    ratio = ((S32.double() - ref).abs() / bound).max().item()
    print("schur %s: fp32 host product at %.3f of the bound" % (shape, ratio))
    assert 0.01 <= ratio <= 1.0, ratio
    got = T.gradient(tp.P32, R.LMBDA, tp.v.float())
    err = (got.double() - tp.ref).abs().max().item()
    print("gradient %s: cond(S) %.0f, fp32 host branch error / max|ref| %.2e, bound %.2e" % (
        shape, tp.cond, err / tp.ref.abs().max().item(), 4e-7 * tp.cond))
    assert err <= R.solver_bound(tp.cond, tp.ref), (err, tp.cond)
