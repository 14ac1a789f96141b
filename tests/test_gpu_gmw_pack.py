"""`ops.gmw_pack_records` / `dcd_gmw_pack_records` (csrc/gmw.hip) against the torch chain it replaces,
`edge_expand(x[src]).transpose(-2, -1).contiguous()` plus slices of the rows.  Pure data movement: every comparison is
`torch.equal`.  The records outside [dst0, dst0 + n) are pre-filled with a sentinel and must come back untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = -7.5
NAMES = ("e4", "e6", "k2", "k3", "rot", "loc", "dim")


def _tables(nk, dev):
    iu = torch.triu_indices(nk, nk, offset=1)
    return iu[0].to(dev), iu[1].to(dev)


def _inputs(nk, n_rows, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_rows, 14, generator=g).to(dev), torch.randn(n_rows, nk, 2, generator=g).to(dev),
            torch.randn(n_rows, nk, 3, generator=g).to(dev))


def _buffers(nk, cap, dev):
    P = nk * (nk - 1) // 2
    return [torch.full((cap,) + s, SENTINEL, device=dev) for s in ((4, P), (6, P), (nk, 2), (nk, 3), (1,), (3,), (3,))]


def _reference(rows, k2, k3, src, pi, pj):
    """The chain of `gmw.refine` on the gathered records; a row number outside the table gives a zero record."""
    n_rows = rows.shape[0]
    src = torch.as_tensor(src, device=rows.device, dtype=torch.long)
    ok = (src >= 0) & (src < n_rows)
    safe = src.clamp(0, n_rows - 1)

    def expand(f):
        return torch.cat((f.index_select(1, pi), f.index_select(1, pj)), dim=-1).transpose(-2, -1).contiguous()
    r, a, b = rows[safe], k2[safe], k3[safe]
    out = [expand(a), expand(b), a, b, r[:, 12:13], r[:, 9:12], r[:, 6:9]]
    return [torch.where(ok.view((-1,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t)) for t in out]


def _pack(rows, k2, k3, src, dst0, pi, pj, bufs):
    from dcd_amd import ops
    src_dev = torch.tensor(src, dtype=torch.int32, device=rows.device)
    return ops.gmw_pack_records(rows, k2, k3, src_dev, dst0, pi.int(), pj.int(), *bufs)


def _check(bufs, want, dst0, n):
    for name, got, ref in zip(NAMES, bufs, want):
        assert torch.equal(got[dst0:dst0 + n], ref), name
        rest = torch.cat((got[:dst0], got[dst0 + n:]))
        assert bool((rest == SENTINEL).all()), name + ": a record outside [dst0, dst0 + n) was written"


def test_native_shape_out_of_order_with_a_repeat(cuda):
    nk = 73
    rows, k2, k3 = _inputs(nk, 8, cuda)
    pi, pj = _tables(nk, cuda)
    assert pi.numel() == 2628
    src = [5, 1, 5]
    bufs = _buffers(nk, 6, cuda)
    assert _pack(rows, k2, k3, src, 2, pi, pj, bufs) == 3
    _check(bufs, _reference(rows, k2, k3, src, pi, pj), 2, 3)
    # the layout is the one `GMW.edge_expand` gives with the model's own tables
    from dcd_amd.gmw import GMW
    model = GMW().to(cuda)
    assert torch.equal(model.pair_i, pi) and torch.equal(model.pair_j, pj)
    pick = torch.tensor(src, device=cuda)
    assert torch.equal(bufs[0][2:5], model.edge_expand(k2[pick]).transpose(-2, -1).contiguous())
    assert torch.equal(bufs[1][2:5], model.edge_expand(k3[pick]).transpose(-2, -1).contiguous())


@pytest.mark.parametrize("nk", [5, 9, 2], ids=["P10_4byte_stores", "P36_16byte_stores_below_a_wave", "P1"])
def test_small_key_point_counts(cuda, nk):
    rows, k2, k3 = _inputs(nk, 7, cuda, seed=nk)
    pi, pj = _tables(nk, cuda)
    src = [6, 0, 3, 3, 2]
    bufs = _buffers(nk, 7, cuda)
    _pack(rows, k2, k3, src, 1, pi, pj, bufs)
    _check(bufs, _reference(rows, k2, k3, src, pi, pj), 1, 5)


@pytest.mark.parametrize("nk", [73, 5])
def test_row_numbers_outside_the_table_give_zero_records(cuda, nk):
    rows, k2, k3 = _inputs(nk, 4, cuda, seed=3)
    pi, pj = _tables(nk, cuda)
    src = [2, -1, 0, 4, 3]                                              # -1 and n_rows
    bufs = _buffers(nk, 5, cuda)
    _pack(rows, k2, k3, src, 0, pi, pj, bufs)
    want = _reference(rows, k2, k3, src, pi, pj)
    _check(bufs, want, 0, 5)
    for name, got in zip(NAMES, bufs):
        assert bool((got[1] == 0).all()) and bool((got[3] == 0).all()), name
    assert torch.equal(bufs[2][0], k2[2]) and torch.equal(bufs[3][4], k3[3])


def _raw_call(rows, k2, k3, nk, src, n, dst0, cap, pi, pj, bufs):
    from dcd_amd import _lib
    return _lib.lib().dcd_gmw_pack_records(_lib.stream_of(rows), rows.data_ptr(), k2.data_ptr(), k3.data_ptr(), rows.shape[0], nk,
                                           src.data_ptr(), n, dst0, cap, pi.data_ptr(), pj.data_ptr(), *(b.data_ptr() for b in bufs))


def test_nothing_to_do_and_refusals_leave_the_buffers_alone(cuda):
    """n = 0 is DCD_OK without a launch; dst0 + n = cap + 1, nk = 129 and a null pointer are refused by the argument check (status
    1, DCD_ERR_BAD_ARG) -- no launch happens, so the sentinel survives everywhere."""
    nk, cap = 73, 4
    rows, k2, k3 = _inputs(nk, 4, cuda)
    pi, pj = (t.int() for t in _tables(nk, cuda))
    src = torch.tensor([0, 1, 2], dtype=torch.int32, device=cuda)
    bufs = _buffers(nk, cap, cuda)
    assert _raw_call(rows, k2, k3, nk, src, 0, 2, cap, pi, pj, bufs) == 0
    assert _raw_call(rows, k2, k3, nk, src, 3, 2, cap, pi, pj, bufs) == 1          # 2 + 3 = cap + 1
    assert _raw_call(rows, k2, k3, 129, src, 3, 0, cap, pi, pj, bufs) == 1
    assert _raw_call(rows, k2, k3, 1, src, 3, 0, cap, pi, pj, bufs) == 1
    from dcd_amd import _lib
    L = _lib.lib()
    args = [rows.data_ptr(), k2.data_ptr(), k3.data_ptr(), 4, nk, None, 3, 0, cap, pi.data_ptr(), pj.data_ptr()] + [b.data_ptr() for b in bufs]
    assert L.dcd_gmw_pack_records(_lib.stream_of(rows), *args) == 1
    torch.cuda.synchronize()
    for name, got in zip(NAMES, bufs):
        assert bool((got == SENTINEL).all()), name
    # the wrapper: the same refusal as an error, and its own shape / dtype checks
    from dcd_amd import ops
    with pytest.raises(_lib.DcdHipError):
        ops.gmw_pack_records(rows, k2, k3, src, 2, pi, pj, *bufs)
    with pytest.raises(ValueError):
        ops.gmw_pack_records(rows, k2, k3, src.long(), 0, pi, pj, *bufs)
    with pytest.raises(ValueError):
        ops.gmw_pack_records(rows[:, :13].contiguous(), k2, k3, src, 0, pi, pj, *bufs)
    with pytest.raises(ValueError):
        ops.gmw_pack_records(rows, k2, k3, src, 0, pi[:-1], pj, *bufs)
    with pytest.raises(_lib.DcdHipError):
        ops.gmw_pack_records(rows.cpu(), k2, k3, src, 0, pi, pj, *bufs)
    for name, got in zip(NAMES, bufs):
        assert bool((got == SENTINEL).all()), name


def test_two_calls_give_the_same_bits(cuda):
    nk = 73
    rows, k2, k3 = _inputs(nk, 8, cuda, seed=11)
    pi, pj = _tables(nk, cuda)
    src = [7, 0, 3, 3, 1]
    first, second = _buffers(nk, 5, cuda), _buffers(nk, 5, cuda)
    _pack(rows, k2, k3, src, 0, pi, pj, first)
    _pack(rows, k2, k3, src, 0, pi, pj, second)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), name
