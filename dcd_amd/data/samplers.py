"""The index streams of the reference's samplers (DGDE/data/samplers/distributed_sampler.py), as host code without a data loader.

`TrainingSampler` is the reference's infinite stream (:12-57): `randperm(size)` after `randperm(size)` drawn from ONE
`torch.Generator().manual_seed(seed)`, of which rank r of w takes positions r, r + w, r + 2w, ...  `InferenceSampler` gives
each rank one contiguous shard (:175-202).  The reference reads rank and world size from `comm`; here they are constructor
arguments, so one process can state every rank's stream (tests) and a batch source can be rebuilt for any rank.

The stream is never stored: `indices(start)` regenerates it from the seed and skips whole epochs without unpacking them, so
"position k of the stream" is a pure function of (size, shuffle, seed, rank, world_size, k).  That is what makes a resumed
run continue where it stopped (dcd_amd/data/batches.py)."""
import torch


class TrainingSampler:
    def __init__(self, size, shuffle=True, seed=0, rank=0, world_size=1):
        if size <= 0:
            raise ValueError("TrainingSampler needs a positive size, got %d" % size)
        if not 0 <= rank < world_size:
            raise ValueError("rank %d outside a world of %d" % (rank, world_size))
        self.size, self.shuffle, self.seed = int(size), bool(shuffle), int(seed)
        self.rank, self.world_size = int(rank), int(world_size)

    def _epochs(self):
        g = torch.Generator()
        g.manual_seed(self.seed)
        while True:
            yield (torch.randperm(self.size, generator=g) if self.shuffle else torch.arange(self.size)).tolist()

    def indices(self, start=0):
        """This rank's stream from its position `start` on: an endless generator of ints."""
        if start < 0:
            raise ValueError("start %d" % start)
        pos = self.rank + start * self.world_size           # position in the global stream
        skip, pos = divmod(pos, self.size)
        for e, epoch in enumerate(self._epochs()):           # skipped epochs are still drawn: the generator's state moves on
            if e < skip:
                continue
            while pos < self.size:
                yield epoch[pos]
                pos += self.world_size
            pos -= self.size

    def take(self, start, n):
        """Positions [start, start + n) of this rank's stream as a list."""
        it = self.indices(start)
        return [next(it) for _ in range(n)]

    def __iter__(self):
        return self.indices(0)


class InferenceSampler:
    def __init__(self, size, rank=0, world_size=1):
        if size <= 0:
            raise ValueError("InferenceSampler needs a positive size, got %d" % size)
        if not 0 <= rank < world_size:
            raise ValueError("rank %d outside a world of %d" % (rank, world_size))
        shard = (size - 1) // world_size + 1
        self.local = range(min(shard * rank, size), min(shard * (rank + 1), size))

    def __iter__(self):
        return iter(self.local)

    def __len__(self):
        return len(self.local)
