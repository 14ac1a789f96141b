"""GPU: batched SPD solve (csrc/spd.hip: blocked Cholesky on the fp32 matrix pipe + blocked substitutions) against
torch.linalg.solve in float64 on the host."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def spd(b, n, seed, cond_shift):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(b, n, n, generator=g, dtype=torch.float64)
    S = A @ A.transpose(1, 2) / n + cond_shift * torch.eye(n, dtype=torch.float64)
    return S, torch.randn(b, n, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("case", [(2, 64, 0.5), (3, 128, 0.5), (2, 132, 0.1), (2, 300, 0.05), (1, 1024, 0.05), (8, 2628, 0.02)])
def test_spd_solve_matches_float64(cuda, case):
    from dcd_amd import ops
    b, n, shift = case
    S, r = spd(b, n, 7, shift)
    ref = torch.linalg.solve(S, r.unsqueeze(-1)).squeeze(-1)
    y = ops.spd_solve(S.float().to(cuda).contiguous(), r.float().to(cuda)).cpu().double()
    # fp32 factorisation: error ~ cond(S) * 2^-24 relative to the solution's scale
    cond = float(torch.linalg.cond(S[0]))
    assert (y - ref).abs().max().item() <= 4e-7 * cond * ref.abs().max().item() + 1e-6, (cond, (y - ref).abs().max().item())


def test_transport_schur_system(cuda):
    """The system the transport layer's backward solves (Schur complement of a transport plan), against float64."""
    from dcd_amd import ops
    from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T
    torch.manual_seed(0)
    b, n = 2, 516
    M = torch.rand(b, n, n, dtype=torch.float64)
    r = torch.full((b, n), 1.0 / n, dtype=torch.float64)
    P = T.sinkhorn(M, r, r, 10.0, 1e-12, 500)
    lamP = 10.0 * P
    G = lamP[:, 1:, :]
    S = -G.transpose(1, 2) @ (G.sum(-1).reciprocal().unsqueeze(-1) * G)
    S.diagonal(dim1=-2, dim2=-1).add_(lamP.sum(-2))
    rhs = torch.randn(b, n, dtype=torch.float64)
    ref = torch.linalg.solve(S, rhs.unsqueeze(-1)).squeeze(-1)
    y = ops.spd_solve(S.float().to(cuda).contiguous(), rhs.float().to(cuda)).cpu().double()
    assert (y - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


def test_not_positive_definite_yields_nan(cuda):
    """A matrix that is not positive definite must not produce a finite-looking solution (advisor r2): the kernel poisons the
    factor at the first non-positive pivot, y is NaN (torch.linalg.cholesky would raise), and the train step's non-finite
    guard then skips the update.  The well-conditioned matrix in the same batch is unaffected."""
    from dcd_amd import ops
    S, r = spd(2, 132, 3, 0.5)
    S[1, 40, 40] = -5.0
    y = ops.spd_solve(S.float().to(cuda).contiguous(), r.float().to(cuda)).cpu()
    ref0 = torch.linalg.solve(S[0], r[0])
    assert torch.isfinite(y[0]).all() and (y[0].double() - ref0).abs().max() <= 1e-4 * ref0.abs().max()
    assert torch.isnan(y[1]).any()


# ---- edges of the solver that the transport layer's backward relies on (bound: the one above, per matrix) ----

DCD_ERR_BAD_ARG, DCD_ERR_WORKSPACE = 1, 2
EDGE_N = [4, 8, 124, 128, 256, 260]          # below one 32-column panel, a narrow last block (124, 260 = 2 x 128 + 4), whole blocks


def solve_abi(aug, rows, n, info=None, short=0, s_shift_bytes=0, n_arg=None):
    """dcd_spd_solve on aug's leading (b, rows, n) floats; y starts as NaN with a payload.  Returns (status, y)."""
    from dcd_amd import _lib
    import transport_refs as R
    L = _lib.lib()
    b = aug.shape[0]
    nbytes = L.dcd_spd_solve_workspace_bytes(b, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=aug.device)
    y = R.sentinel(b * n, R.NAN_BITS).to(aug.device).view(b, n)
    st = L.dcd_spd_solve(_lib.stream_of(aug), aug.data_ptr() + s_shift_bytes, y.data_ptr(), b, n if n_arg is None else n_arg, rows,
                         None if info is None else info.data_ptr(), ws.data_ptr(), nbytes - short)
    torch.cuda.synchronize()
    return st, y


def assert_within_solver_bound(y, S, ref):
    for i in range(S.shape[0]):
        cond = float(torch.linalg.cond(S[i]))
        err = (y[i].cpu().double() - ref[i]).abs().max().item()
        assert err <= 4e-7 * cond * ref[i].abs().max().item() + 1e-6, (i, cond, err)


@pytest.fixture(scope="module")
def edge_systems():
    """{n: (S, r, ref)} in float64 on the host, built once."""
    out = {}
    for n in EDGE_N:
        S, r = spd(3, n, 7, 0.5)
        out[n] = (S, r, torch.linalg.solve(S, r.unsqueeze(-1)).squeeze(-1))
    return out


@pytest.mark.parametrize("n", EDGE_N)
def test_spd_solve_reads_only_the_lower_triangle_and_the_rhs_row(cuda, edge_systems, n):
    """In production the buffer comes from torch.empty: schur_lower writes the lower triangle and the diagonal tiles, `gradient`
    row n, nobody rows n+1 .. n+3.  With NaN everywhere strictly above the diagonal and in the rows from n+1 on, y must be
    bit-identical to the y of the full symmetric matrix (the kernels are deterministic, so any read of those entries shows),
    through ops.spd_solve* (rows = n + 4) and at ABI level with rows = n + 1, where the floats behind the last matrix keep
    their sentinel."""
    from dcd_amd import ops
    import transport_refs as R
    S, r, ref = edge_systems[n]
    S32, r32 = S.float().to(cuda), r.float().to(cuda)
    upper = torch.ones(n, n, dtype=torch.bool, device=cuda).triu(1)
    y_clean = ops.spd_solve(S32.contiguous(), r32)
    assert_within_solver_bound(y_clean, S, ref)
    aug = ops.spd_buffer(3, n, cuda).fill_(float("nan"))
    aug[:, :n] = S32.masked_fill(upper, float("nan"))
    aug[:, n] = r32
    y_poison = ops.spd_solve_inplace(aug)
    assert R.same_bits(y_poison.cpu(), y_clean.cpu()).all()
    # rows = n + 1: the matrices lie (n + 1) n floats apart and nothing follows the right-hand side
    guard = 64
    for poison in (False, True):
        flat = R.sentinel(3 * (n + 1) * n + guard, R.NAN_BITS).to(cuda)
        tight = flat[:3 * (n + 1) * n].view(3, n + 1, n)
        tight[:, :n] = S32.masked_fill(upper, float("nan")) if poison else S32
        tight[:, n] = r32
        st, y = solve_abi(tight, n + 1, n)
        assert st == 0
        assert R.same_bits(flat[-guard:].cpu(), R.sentinel(guard, R.NAN_BITS)).all(), "written past the last right-hand side"
        if poison:
            assert R.same_bits(y.cpu(), y_tight.cpu()).all()
        else:
            y_tight = y
            assert_within_solver_bound(y_tight, S, ref)


def test_spd_solve_info_names_the_block_of_the_bad_pivot(cuda):
    """info[b] = 1 + first row of the 128-block whose pivot was not positive: a negative diagonal entry at 200 (second block) and a
    NaN at 259 (third block, 4 wide) in a batch whose first matrix is clean."""
    S, r = spd(3, 260, 7, 0.5)
    S[1, 200, 200] = -5.0
    S[2, 259, 259] = float("nan")
    ref0 = torch.linalg.solve(S[0], r[0])
    aug = torch.empty(3, 261, 260, device=cuda)
    aug[:, :260] = S.float().to(cuda)
    aug[:, 260] = r.float().to(cuda)
    info = torch.zeros(3, dtype=torch.int32, device=cuda)
    st, y = solve_abi(aug, 261, 260, info=info)
    assert st == 0
    assert info.cpu().tolist() == [0, 129, 257]
    y = y.cpu()
    assert torch.isnan(y[1]).any() and torch.isnan(y[2]).any()
    assert torch.isfinite(y[0]).all()
    assert_within_solver_bound(y[:1], S[:1], ref0.unsqueeze(0))


@pytest.mark.parametrize("what", ["n-not-multiple-of-4", "rows-equal-n", "s-misaligned", "workspace-short"])
def test_spd_solve_refuses_and_leaves_y_alone(cuda, what):
    import transport_refs as R
    n = 8
    S, r = spd(2, n, 7, 0.5)
    aug = torch.zeros(2, n + 4, n, device=cuda)
    aug[:, :n] = S.float().to(cuda)
    aug[:, n] = r.float().to(cuda)
    kw, want = {"n-not-multiple-of-4": (dict(n_arg=n - 2), DCD_ERR_BAD_ARG), "rows-equal-n": (dict(rows=n), DCD_ERR_BAD_ARG),
                "s-misaligned": (dict(s_shift_bytes=4), DCD_ERR_BAD_ARG), "workspace-short": (dict(short=1), DCD_ERR_WORKSPACE)}[what]
    st, y = solve_abi(aug, kw.pop("rows", n + 1), n, **kw)
    assert st == want
    assert R.same_bits(y.cpu(), R.sentinel(2 * n, R.NAN_BITS).view(2, n)).all()
