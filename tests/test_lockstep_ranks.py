"""The sequential rank emulator (tests/lockstep_ranks.py) proved on the CPU, before it is trusted with the HIP kernels
(tests/test_gpu_syncbn.py): tests/cpu_syncbn._SyncStatsCPU makes the same two collective calls as the device path
(forward statistics, backward sums); driven through the emulator on fp64 tensors it must reproduce F.batch_norm + autograd on
the concatenated batch to fp64 rounding (1e-12 of each tensor's max magnitude)."""
import pytest
import torch
from torch.nn import functional as F

import cpu_syncbn
from lockstep_ranks import lockstep

EPS = 1e-5


def _shard(rank, shape, seed):
    """Rank r's inputs, afresh on every call: statistics that differ from rank to rank by tens of per cent."""
    g = torch.Generator().manual_seed(seed * 100 + rank)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * (0.6 + 0.5 * (rank % 3)) + (0.8 - 0.7 * (rank % 4))
    gy = torch.randn(*shape, generator=g, dtype=torch.float64)
    return x, gy


def _params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.3


def _emulated(monkeypatch, R, shape, seed, fault=None):
    C = shape[1]
    with lockstep(monkeypatch, fault=fault) as ranks:
        def fn(rank):
            x, gy = _shard(rank, shape, seed)
            w, b = _params(C, seed)
            x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
            y, mean, var = cpu_syncbn._SyncStatsCPU.apply(x, w, b, EPS, ranks.group)
            y.backward(gy)
            return y.detach(), x.grad, w.grad, b.grad, mean, var
        out = ranks.run(fn, R)
        return out, ranks.calls, ranks.collectives


def _full_batch(R, shape, seed):
    shards = [_shard(r, shape, seed) for r in range(R)]
    x = torch.cat([s[0] for s in shards]).requires_grad_()
    gy = torch.cat([s[1] for s in shards])
    w, b = _params(shape[1], seed)
    w.requires_grad_(), b.requires_grad_()
    y = F.batch_norm(x, None, None, w, b, True, 0.1, EPS)
    y.backward(gy)
    dims = (0, 2, 3)
    return y.detach(), x.grad, w.grad, b.grad, x.detach().mean(dims), x.detach().var(dims, unbiased=False)


def _close(a, ref, what, tol=1e-12):
    err = (a - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert err <= tol * scale, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


def _compare(out, ref, R, B):
    y, gx, gw, gb, mean, var = ref
    for r in range(R):
        sl = slice(r * B, (r + 1) * B)
        _close(out[r][0], y[sl], "y of rank %d" % r)
        _close(out[r][1], gx[sl], "grad_x of rank %d" % r)
        _close(out[r][4], mean, "mean on rank %d" % r)
        _close(out[r][5], var, "var on rank %d" % r)
    _close(sum(o[2] for o in out), gw, "grad_weight summed over the ranks")
    _close(sum(o[3] for o in out), gb, "grad_bias summed over the ranks")


@pytest.mark.parametrize("R,shape", [(2, (2, 6, 5, 7)), (3, (1, 4, 3, 5)), (3, (2, 1, 4, 4))])
def test_emulated_ranks_equal_the_full_batch(monkeypatch, R, shape):
    out, calls, collectives = _emulated(monkeypatch, R, shape, seed=7)
    assert collectives == 2 and calls == 3 * R          # one layer: (collectives + 1) x R calls
    _compare(out, _full_batch(R, shape, seed=7), R, shape[0])


@pytest.mark.parametrize("fault", ["no_reduce:0", "no_reduce:1", "world_size_1"])
def test_the_fault_option_is_seen_by_the_comparison(monkeypatch, fault):
    R, shape = 2, (2, 6, 5, 7)
    out, _, _ = _emulated(monkeypatch, R, shape, seed=7, fault=fault)
    with pytest.raises(AssertionError):
        _compare(out, _full_batch(R, shape, seed=7), R, shape[0])


def test_the_patches_end_with_the_block(monkeypatch):
    import torch.distributed as dist
    before = (dist.all_reduce, dist.get_world_size)
    with lockstep(monkeypatch) as ranks:
        assert dist.all_reduce == ranks.all_reduce and dist.get_world_size == ranks.get_world_size
    assert (dist.all_reduce, dist.get_world_size) == before


def test_a_contribution_that_varies_between_runs_is_reported(monkeypatch):
    import torch.distributed as dist
    with lockstep(monkeypatch) as ranks:
        n = [0]

        def fn(rank):
            n[0] += 1
            t = torch.full((3, 2), float(n[0]), dtype=torch.float64)        # another value on every call
            dist.all_reduce(t, group=ranks.group)
            u = torch.ones((3, 2), dtype=torch.float64)
            dist.all_reduce(u, group=ranks.group)
        with pytest.raises(AssertionError, match="differs between two runs"):
            ranks.run(fn, 2)


def test_unequal_collectives_shapes_and_types_are_reported(monkeypatch):
    import torch.distributed as dist
    with lockstep(monkeypatch) as ranks:
        def uneven(rank):
            for _ in range(1 + rank):
                dist.all_reduce(torch.ones((3, 2), dtype=torch.float64), group=ranks.group)
        with pytest.raises(AssertionError):
            ranks.run(uneven, 2)

        def shapes(rank):
            dist.all_reduce(torch.ones((3 + rank, 2), dtype=torch.float64), group=ranks.group)
        with pytest.raises(AssertionError, match="rank 1 sends"):
            ranks.run(shapes, 2)

        def fp32(rank):
            dist.all_reduce(torch.ones((3, 2)), group=ranks.group)
        with pytest.raises(AssertionError):
            ranks.run(fp32, 2)

        def other_group(rank):
            dist.all_reduce(torch.ones((3, 2), dtype=torch.float64), group=None)
        with pytest.raises(AssertionError, match="not the emulator's"):
            ranks.run(other_group, 2)


def test_the_sum_is_taken_in_rank_order_and_replayed_in_place(monkeypatch):
    import torch.distributed as dist
    vals = [1.0, 1e-17, -1.0]                                   # (1 + 1e-17) - 1 = 0 in rank order, 1e-17 in any other
    with lockstep(monkeypatch) as ranks:
        def fn(rank):
            t = torch.full((1, 2), vals[rank], dtype=torch.float64)
            keep = t
            dist.all_reduce(t, group=ranks.group)
            return keep, dist.get_world_size(ranks.group)
        out = ranks.run(fn, 3)
    assert all(float(o[0][0, 0]) == 0.0 and o[1] == 3 for o in out)
