"""GPU: dcd_sgemm (csrc/sgemm_f32.inc behind the C ABI of csrc/spd.hip) by element against the float64 product of the same fp32
operands, and ops.schur_lower against the float64 Schur complement.  References, bounds and cases: tests/transport_refs.py."""
import pytest
import torch

import transport_refs as R

pytestmark = pytest.mark.gpu

DCD_ERR_BAD_ARG = 1


def run_sgemm(cuda, p, **override):
    """One call of dcd_sgemm on the buffers of a transport_refs problem; returns (status, C's buffer afterwards on the host)."""
    from dcd_amd import _lib
    c = p.case
    a = p.a_buf.to(cuda)
    b = a if p.b_buf is p.a_buf else p.b_buf.to(cuda)
    cbuf = p.c_buf.to(cuda)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and cbuf.data_ptr() % 16 == 0
    args = dict(A=a.data_ptr() + 4 * p.a_off, lda=p.lda, strideA=p.strideA, ak=c.ak, B=b.data_ptr() + 4 * p.b_off, ldb=p.ldb,
                strideB=p.strideB, bk=c.bk, C=cbuf.data_ptr() + 4 * p.c_off, ldc=p.ldc, strideC=p.strideC, M=c.M, N=c.N, K=c.K, Z=c.Z,
                alpha=c.alpha, accumulate=c.accumulate, lower_only=c.lower_only)
    args["A"] += override.pop("a_shift_bytes", 0)
    args.update(override)
    st = _lib.lib().dcd_sgemm(_lib.stream_of(cbuf), *[args[k] for k in (
        "A", "lda", "strideA", "ak", "B", "ldb", "strideB", "bk", "C", "ldc", "strideC", "M", "N", "K", "Z", "alpha", "accumulate",
        "lower_only")])
    torch.cuda.synchronize()
    return st, cbuf.cpu()


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=lambda c: c.name)
def test_sgemm_by_element_and_leaves_the_rest_of_c_alone(cuda, case):
    """Four operand layouts with padded leading dimensions and batch strides, K around the 16-wide step, M and N around the 128
    tile, the solver's trailing update (alpha = -1, accumulate, both operands one buffer) with and without lower_only, the
    Schur form, and a C that is only 4-byte aligned.  Every written element within the gamma_K bound; every other float of C's
    buffer -- padding columns, spare rows, tiles that lower_only skips -- bit-identical to the sentinel it held."""
    p = R.gemm_problem(case)
    st, after = run_sgemm(cuda, p)
    assert st == 0
    worst = R.gemm_check(p, after, "dcd_sgemm")
    print("dcd_sgemm %s: worst error / bound %.3f" % (case.name, worst))


@pytest.mark.parametrize("what", ["lda", "a-misaligned", "m-zero", "k-zero"])
def test_sgemm_refuses_and_leaves_c_alone(cuda, what):
    """lda % 4 != 0, A 4 bytes off a 16-byte boundary, M = 0, K = 0: DCD_ERR_BAD_ARG, and C keeps its sentinel."""
    case = R.gemm_case("refusal", 130, 67, 37, Z=2, pad_a=4, pad_b=4, off_ab=4)
    p = R.gemm_problem(case)
    # every refused call stays inside its buffers even if it were to run: lda still covers the extent, A moves into its padding
    override = {"lda": dict(lda=p.lda - 2), "a-misaligned": dict(a_shift_bytes=4), "m-zero": dict(M=0), "k-zero": dict(K=0)}[what]
    st, after = run_sgemm(cuda, p, **override)
    assert st == DCD_ERR_BAD_ARG
    assert R.same_bits(after, p.c_buf).all()


@pytest.mark.parametrize("shape", R.TRANSPORT_SHAPES)
def test_schur_lower_matches_float64(cuda, shape):
    """ops.schur_lower on the plan `gradient` would hand it (G a view of lambda P without its first row, so its batch stride is
    larger than its extent), into a solver buffer full of NaN: the lower triangle and the diagonal tiles within
    (m + 3) 2^-24 |G|^T |inv_rows| |G| (+ 2^-23 |cols| on the diagonal) of float64; tiles above the diagonal and the rows from
    n on still NaN."""
    from dcd_amd import ops
    b, m, n = shape
    tp = R.transport_problem(b, m, n)
    G, inv_rows, cols = R.schur_inputs(tp.P32.to(cuda))
    aug = ops.spd_buffer(b, n, cuda)
    aug.fill_(float("nan"))
    ops.schur_lower(G, inv_rows, cols, aug)
    torch.cuda.synchronize()
    ref, bound = R.schur_reference(G, inv_rows, cols)
    out = aug.cpu()
    w = R.lower_tile_mask(n, n).expand(b, n, n)
    d = (out[:, :n].double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    ratio = torch.where(w, d / bound, torch.zeros_like(d))
    worst = ratio.max().item()
    at = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
    print("schur_lower %s: worst error / bound %.3f" % (shape, worst))
    assert worst <= 1.0, "S%s: error %.3e, bound %.3e, ref %.6e: ratio %.3f" % (at, d[at].item(), bound[at].item(), ref[at].item(), worst)
    assert torch.isnan(out[:, :n][~w]).all(), "a tile above the diagonal was written"
    assert torch.isnan(out[:, n:]).all(), "a row below the matrix was written"
