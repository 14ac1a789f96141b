"""References and derived bounds for the device route of the transport layer's backward: `dcd_sgemm`, `ops.schur_lower`,
`ops.spd_solve*` and `RegularisedTransportFn.gradient`.  TEST INFRASTRUCTURE, torch on the CPU.

Every reference is the float64 result of the same fp32 operands, and every bound is derived, never measured:

  GEMM    |C - ref| <= (K + 2) u |alpha| (|A| |B|)_ij + u |ref|_ij (+ u |C0|_ij under accumulate),  u = 2^-24.
          gamma_K of an fp32 dot product of length K holds in any summation order (Higham, Accuracy and Stability of Numerical
          Algorithms, section 3.1), so it covers the order of the matrix instructions; the two extra units and the u |ref| /
          u |C0| terms cover the multiplication by alpha and the addition of C0.
  Schur   S = diag(cols) - G^T diag(inv_rows) G:  (m + 3) u (|G|^T (|inv_rows| |G|))_ij, plus 2 u |cols|_j on the diagonal; m is
          the number of rows of the plan (K = m - 1 rows of G), one more unit than the GEMM for the fp32 rounding of
          inv_rows * G that the wrapper does, the diagonal term for the addition of cols.
  solve   the project's own solver bound 4e-7 cond(S) max|ref| (tests/test_gpu_spd.py), applied to the gradient as well.

tests/test_transport_refs.py holds these helpers to fp32 products on the host; the GPU tests hold the kernels to them.
"""
import functools
from types import SimpleNamespace

import torch

U = 2.0 ** -24
TILE = 128                         # csrc/sgemm_f32.inc: tile edge, and the granularity of `lower_only`
LMBDA = 10.0
NAN_BITS = 0x7FC0D0D1              # a quiet NaN with a payload: where nothing is accumulated
ODD_BITS = 0x4640E6B7              # 12345.68 as fp32: a finite sentinel where the kernel reads C


def lower_tile_mask(M, N):
    """(M, N) bool: the elements `lower_only` writes -- the tiles with n0 < m0 + 128, diagonal tiles complete."""
    m = torch.arange(M).unsqueeze(1) // TILE
    n = torch.arange(N).unsqueeze(0) // TILE
    return n <= m


def sentinel(numel, bits):
    return torch.full((numel,), bits, dtype=torch.int32).view(torch.float32)


def same_bits(a, b):
    """Element-wise bit identity of two fp32 tensors (NaN payloads and signed zeros included)."""
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- GEMM

def gemm_case(name, M, N, K, Z=1, ak=0, bk=0, alpha=1.0, accumulate=0, lower_only=0, pad_a=0, pad_b=0, pad_c=5, off_ab=0, off_c=0,
              pad_stride=0, same_ab=False, skip_a_rows=0):
    """One call of dcd_sgemm.  pad_a / pad_b: leading dimension minus the extent rounded up to a multiple of 4 (the ABI wants lda and
    ldb multiples of 4); pad_c: ldc minus N; off_ab / off_c: floats between the start of the buffer and the operand; pad_stride:
    floats added to each batch stride; same_ab: B is the first N rows of A's buffer (both k-contiguous, the trailing update of
    dcd_spd_solve); skip_a_rows: rows of A's buffer that precede the operand in every
    batch entry (G is the plan without its first row)."""
    return SimpleNamespace(name=name, M=M, N=N, K=K, Z=Z, ak=ak, bk=bk, alpha=alpha, accumulate=accumulate, lower_only=lower_only,
                           pad_a=pad_a, pad_b=pad_b, pad_c=pad_c, off_ab=off_ab, off_c=off_c, pad_stride=pad_stride,
                           same_ab=same_ab, skip_a_rows=skip_a_rows)


def _gemm_cases():
    cases = []
    for ak in (0, 1):
        for bk in (0, 1):
            cases.append(gemm_case("layout-a%d-b%d" % (ak, bk), 130, 67, 37, Z=3, ak=ak, bk=bk, alpha=0.5, pad_a=4, pad_b=8, off_ab=4,
                                   pad_stride=12))
    for kc in (0, 1):
        for K in (1, 3, 16, 17, 33):
            cases.append(gemm_case("k%d-%s" % (K, "kk" if kc else "ff"), 5, 9, K, ak=kc, bk=kc, pad_a=4, pad_b=8))
    for M, N, K in ((128, 128, 16), (129, 1, 20), (1, 129, 20)):
        for kc in (0, 1):
            cases.append(gemm_case("tile-%dx%dx%d-%s" % (M, N, K, "kk" if kc else "ff"), M, N, K, ak=kc, bk=kc))
    for lo in (1, 0):
        cases.append(gemm_case("trailing-lower%d" % lo, 261, 260, 128, Z=2, ak=1, bk=1, alpha=-1.0, accumulate=1, lower_only=lo, pad_a=4,
                               pad_stride=8, same_ab=True))
    cases.append(gemm_case("schur-form", 300, 300, 99, Z=2, alpha=-1.0, lower_only=1, skip_a_rows=1))
    for kc in (0, 1):
        cases.append(gemm_case("c-4-byte-aligned-%s" % ("kk" if kc else "ff"), 130, 67, 37, Z=2, ak=kc, bk=kc, pad_c=3, off_c=1,
                               pad_stride=4))
    return cases


GEMM_CASES = _gemm_cases()


def _stored(buf, off, Z, rows, cols, ld, stride):
    return buf.as_strided((Z, rows, cols), (stride, ld, 1), off)


def gemm_problem(case, seed=5):
    """Host buffers of one case, laid out as the call sees them.  Everything of A's and B's buffers that the product does not
    cover is NaN (a read of it shows in the result); C's buffer is one sentinel with two spare rows before and after and
    `pad_c` spare columns, and holds C0 in the M x N region under accumulate."""
    c = case
    g = torch.Generator().manual_seed(seed)
    p = SimpleNamespace(case=c)
    ar, ac = (c.M, c.K) if c.ak else (c.K, c.M)
    br, bc = (c.N, c.K) if c.bk else (c.K, c.N)
    p.lda, p.ldb, p.ldc = (ac + 3) // 4 * 4 + c.pad_a, (bc + 3) // 4 * 4 + c.pad_b, c.N + c.pad_c
    assert p.lda % 4 == 0 and p.ldb % 4 == 0 and c.off_ab % 4 == 0 and c.pad_stride % 4 == 0, "the ABI wants these multiples of 4"
    p.strideA = (ar + c.skip_a_rows) * p.lda + c.pad_stride
    p.a_off = c.off_ab + c.skip_a_rows * p.lda
    p.a_buf = sentinel(c.off_ab + c.Z * p.strideA, NAN_BITS).clone()
    a_st = _stored(p.a_buf, p.a_off, c.Z, ar, ac, p.lda, p.strideA)
    a_st.copy_(torch.rand(c.Z, ar, ac, generator=g) * 2 - 1)
    p.A = (a_st if c.ak else a_st.transpose(1, 2)).clone()                     # logical (Z, M, K)
    if c.same_ab:
        assert c.ak and c.bk and c.N <= c.M
        p.b_buf, p.b_off, p.ldb, p.strideB = p.a_buf, p.a_off, p.lda, p.strideA
        p.B = p.A[:, :c.N].transpose(1, 2).clone()
    else:
        p.strideB = br * p.ldb + c.pad_stride
        p.b_off = c.off_ab
        p.b_buf = sentinel(c.off_ab + c.Z * p.strideB, NAN_BITS).clone()
        b_st = _stored(p.b_buf, p.b_off, c.Z, br, bc, p.ldb, p.strideB)
        b_st.copy_(torch.rand(c.Z, br, bc, generator=g) * 2 - 1)
        p.B = (b_st.transpose(1, 2) if c.bk else b_st).clone()                 # logical (Z, K, N)
    p.strideC = (c.M + 3) * p.ldc
    p.c_off = c.off_c + 2 * p.ldc
    p.c_buf = sentinel(c.off_c + c.Z * p.strideC + 4 * p.ldc, ODD_BITS if c.accumulate else NAN_BITS).clone()
    p.C0 = None
    if c.accumulate:
        p.C0 = torch.rand(c.Z, c.M, c.N, generator=g) * 2 - 1
        gemm_result(p, p.c_buf).copy_(p.C0)
    p.written = lower_tile_mask(c.M, c.N) if c.lower_only else torch.ones(c.M, c.N, dtype=torch.bool)
    return p


def gemm_result(p, c_buf):
    """The (Z, M, N) view of a C buffer."""
    return _stored(c_buf, p.c_off, p.case.Z, p.case.M, p.case.N, p.ldc, p.strideC)


def gemm_reference(p):
    """(ref, bound), float64 (Z, M, N)."""
    c = p.case
    ref = c.alpha * p.A.double().matmul(p.B.double())
    bound = (c.K + 2) * U * abs(c.alpha) * p.A.double().abs().matmul(p.B.double().abs())
    if p.C0 is not None:
        ref = ref + p.C0.double()
        bound = bound + U * p.C0.double().abs()
    return ref, bound + U * ref.abs()


def gemm_check(p, c_after, what):
    """The whole contract of one call: the written region within the bound, everything else bit-identical to what was there.
    Returns the worst error / bound over the written region."""
    c = p.case
    ref, bound = gemm_reference(p)
    got = gemm_result(p, c_after).double()
    w = p.written.expand(c.Z, c.M, c.N)
    d = (got - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    ratio = torch.where(w & (d > 0), d / bound, torch.zeros_like(d))
    worst = ratio.max().item()
    at = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
    assert worst <= 1.0, "%s %s: |C - ref| = %.3e at (z, m, n) = %s, bound %.3e (ref %.6e, got %.6e): ratio %.3f" % (
        what, c.name, d[at].item(), at, bound[at].item(), ref[at].item(), got[at].item(), worst)
    untouched = torch.ones(c_after.numel(), dtype=torch.bool)
    gemm_result(p, untouched).copy_(~w)
    changed = untouched & ~same_bits(c_after, p.c_buf)
    assert not changed.any(), "%s %s: %d elements outside the written region changed, the first at float %d of C's buffer" % (
        what, c.name, int(changed.sum()), int(torch.nonzero(changed)[0]))
    return worst


# ------------------------------------------------------------------------------------------------- transport layer

TRANSPORT_SHAPES = [(2, 5, 4), (3, 100, 132), (2, 260, 260), (1, 385, 384), (2, 131, 516)]


def schur_inputs(P32):
    """(G, inv_rows, cols) of a plan, formed as `RegularisedTransportFn.gradient` forms them, in P32's dtype and on its device."""
    b, m, n = P32.shape
    lamP = LMBDA * P32
    G = lamP[:, 1:, :]
    inv_rows = G.matmul(lamP.new_ones(n, 1)).squeeze(-1).reciprocal()
    cols = lamP.new_ones(1, m).matmul(lamP).squeeze(-2)
    return G, inv_rows, cols


def schur_reference(G, inv_rows, cols):
    """(S, bound) in float64 from fp32 (G, inv_rows, cols): S = diag(cols) - G^T diag(inv_rows) G."""
    G, inv_rows, cols = G.cpu().double(), inv_rows.cpu().double(), cols.cpu().double()
    S = -G.transpose(1, 2).matmul(inv_rows.unsqueeze(-1) * G)
    S.diagonal(dim1=-2, dim2=-1).add_(cols)
    m = G.shape[1] + 1
    bound = (m + 3) * U * G.abs().transpose(1, 2).matmul(inv_rows.abs().unsqueeze(-1) * G.abs())
    bound.diagonal(dim1=-2, dim2=-1).add_(2 * U * cols.abs())
    return S, bound


@functools.lru_cache(maxsize=None)
def transport_problem(b, m, n):
    """One seeded plan per shape, shared by every test that needs it (do not modify what this returns): P32 the float64 Sinkhorn
    plan rounded to fp32, v the incoming gradient, ref = gradient(P32 in float64), cond = the largest cond(S) of the batch."""
    from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T
    g = torch.Generator().manual_seed(11)
    M = torch.rand(b, m, n, dtype=torch.float64, generator=g)
    r = torch.full((b, m), 1.0 / m, dtype=torch.float64)
    c = torch.full((b, n), 1.0 / n, dtype=torch.float64)
    P32 = T.sinkhorn(M, r, c, LMBDA, 1e-12, 1000).float()
    v = torch.randn(b, m * n, dtype=torch.float64, generator=g)
    ref = T.gradient(P32.double(), LMBDA, v)
    S64, _ = schur_reference(*schur_inputs(P32.double()))
    cond = max(float(torch.linalg.cond(S64[i])) for i in range(b))
    return SimpleNamespace(P32=P32, v=v, ref=ref, cond=cond)


def solver_bound(cond, ref):
    """The project's solver bound without its absolute term: 4e-7 cond max|ref|."""
    return 4e-7 * cond * ref.abs().max().item()
