"""Test infrastructure: R data-parallel ranks run one after the other in ONE process, without a process group.

The synchronised BatchNorm paths exchange nothing but fp64 per-channel sums, through `torch.distributed.all_reduce(t, group=g)`
and `torch.distributed.get_world_size(g)` (looked up on the module at call time: `import torch.distributed as dist` inside the
functions of dcd_amd/ops.py, dcd_amd/model/head/trunk_moments.py and tests/cpu_syncbn.py).  Every reduction in csrc/norm.hip
has a fixed order, so a rank's contribution to a collective is the same on every run.  `lockstep` patches the two functions and
`run(fn, R)` calls `fn(rank)` for every rank in PASSES; collectives are numbered per rank in call order (one BN layer: 0 =
forward statistics, 1 = backward sums):

    pass p:  collective j < p   REPLAYED: the tensor is overwritten in place with the recorded sum over the ranks (fp64, rank order),
                                after asserting that the rank contributed, bit for bit, what it contributed when j was recorded;
             collective j == p  RECORDED (a clone); the rank runs on with its local value and everything it computes afterwards
                                in this pass is dropped (no exception is thrown through autograd);
             collective j > p   left alone (its input is already meaningless).
    The pass that meets no unrecorded collective is the last; its return values are the result.  n collectives cost (n + 1) R
    calls of `fn`, so `fn` must build its modules and inputs afresh from the rank and a seed on every call (the running buffers are
    updated in place by each forward).

The process group is the sentinel `ranks.group`; put it into `BatchNorm2d.sync_group`.  `fault=` runs the negative controls:
"no_reduce:<j>" replays the rank's OWN contribution for collective j (a sum left unreduced), "world_size_1" makes
`get_world_size` answer 1 (the element count not scaled).  Neither touches product code.
"""
import contextlib

import torch


class _Group:
    """Stands in for a process group (only its identity is used)."""

    def __repr__(self):
        return "<lockstep group>"


class LockstepRanks:
    def __init__(self, fault=None):
        self.group = _Group()
        self.fault = fault
        self.no_reduce = None
        if fault is not None:
            if fault.startswith("no_reduce:"):
                self.no_reduce = int(fault.split(":", 1)[1])
            elif fault != "world_size_1":
                raise ValueError("unknown fault %r" % (fault,))
        self.world = None          # set by run()
        self.recorded = []         # recorded[j][rank]: the rank's contribution to collective j
        self.calls = 0             # fn calls of the last run (cost check)
        self._rank = self._pass = self._next = None

    # ---- the two patched functions --------------------------------------------------------------------------------------
    def get_world_size(self, group=None):
        assert group is self.group, "get_world_size on a group that is not the emulator's: %r" % (group,)
        assert self.world is not None, "get_world_size outside run()"
        return 1 if self.fault == "world_size_1" else self.world

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        assert group is self.group, "all_reduce on a group that is not the emulator's: %r" % (group,)
        assert self._rank is not None, "all_reduce outside run()"
        assert op is None or op == torch.distributed.ReduceOp.SUM, "only sums are exchanged"
        assert not async_op
        # include/dcd_hip.h: `stats` / `sums` are C x 2 doubles (the trunks: R x 2)
        assert tensor.dtype == torch.float64 and tensor.dim() == 2 and tensor.shape[1] == 2, (tensor.dtype, tuple(tensor.shape))
        j, r, p = self._next, self._rank, self._pass
        self._next += 1
        if j > p:
            return None
        if j == p:
            if len(self.recorded) == j:
                assert r == 0, "rank %d issues collective %d, the ranks before it do not" % (r, j)
                self.recorded.append([])
            assert len(self.recorded[j]) == r, "collective %d: rank %d recorded out of turn" % (j, r)
            if r > 0:
                assert self.recorded[j][0].shape == tensor.shape, \
                    "collective %d: rank %d sends %s, rank 0 %s" % (j, r, tuple(tensor.shape), tuple(self.recorded[j][0].shape))
            self.recorded[j].append(tensor.detach().clone())
            return None
        mine = self.recorded[j][r]
        assert mine.shape == tensor.shape and torch.equal(tensor, mine), \
            "collective %d, rank %d: the contribution differs between two runs (a reduction whose order varies?)" % (j, r)
        if self.no_reduce == j:
            return None
        total = self.recorded[j][0].clone()
        for other in self.recorded[j][1:]:
            total += other
        with torch.no_grad():
            tensor.copy_(total)
        return None

    # ---- the driver -----------------------------------------------------------------------------------------------------
    def run(self, fn, R):
        """`fn(rank)` for rank 0..R-1, pass after pass, until a pass needs no new collective: the list of its R return values."""
        assert R >= 1
        self.world, self.recorded, self.calls = R, [], 0
        p = 0
        try:
            while True:
                results, issued = [], []
                for r in range(R):
                    self._rank, self._pass, self._next = r, p, 0
                    results.append(fn(r))
                    self.calls += 1
                    issued.append(self._next)
                assert len(set(issued)) == 1, "the ranks issue different numbers of collectives: %s" % (issued,)
                if issued[0] <= p:
                    assert issued[0] == len(self.recorded) and all(len(c) == R for c in self.recorded)
                    return results
                assert len(self.recorded) == p + 1 and len(self.recorded[p]) == R
                results = None
                p += 1
        finally:
            self._rank = self._pass = self._next = None
            self.world = None

    @property
    def collectives(self):
        """Collectives per rank of the last run."""
        return len(self.recorded)


@contextlib.contextmanager
def lockstep(monkeypatch, fault=None):
    """`with lockstep(monkeypatch) as ranks: out = ranks.run(fn, R)` -- torch.distributed's all_reduce / get_world_size answer from
    the emulator inside the block (and until the test's monkeypatch is undone; the block's end undoes them itself)."""
    import torch.distributed as dist
    ranks = LockstepRanks(fault)
    with monkeypatch.context() as m:
        m.setattr(dist, "all_reduce", ranks.all_reduce)
        m.setattr(dist, "get_world_size", ranks.get_world_size)
        yield ranks
