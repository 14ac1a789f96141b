"""Fixture of dcd_amd/data/samplers.py, produced by RUNNING THE REFERENCE'S OWN `TrainingSampler` and `InferenceSampler`
(DGDE/data/samplers/distributed_sampler.py) where they lie, imported with make_golden.install_stubs as the other generators do.
Build container only.  The .npz holds index arrays, nothing of the reference's program text.

The reference reads rank and world size from `comm` in the constructor; in a single process that is rank 0 of 1, so for the
other ranks `_rank` and `_world_size` are set on the object after construction (the `InferenceSampler` computes its shard in
the constructor, so its shard is recomputed by constructing it with `comm` patched for the duration of the call).

Writes sampler.npz:
  train_s<size>_seed<seed>_sh<0|1>_w<world>_r<rank>   the first 3 * size / world + 5 indices of that rank's stream (int64)
  infer_s<size>_w<world>_r<rank>                      that rank's shard (int64, may be empty)
for sizes 1, 7, 64; seeds 0, 63; shuffle on and off; worlds 1, 2, 3 with every rank."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SIZES, SEEDS, WORLDS = (1, 7, 64), (0, 63), (1, 2, 3)


def count(size, world):
    return 3 * (-(-size // world)) + 5


def main():
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    from data.samplers import distributed_sampler as D
    out = {}
    for size, world in itertools.product(SIZES, WORLDS):
        for rank in range(world):
            for seed, shuffle in itertools.product(SEEDS, (True, False)):
                s = D.TrainingSampler(size, shuffle=shuffle, seed=seed)
                s._rank, s._world_size = rank, world
                got = [int(v) for v in itertools.islice(iter(s), count(size, world))]
                out["train_s%d_seed%d_sh%d_w%d_r%d" % (size, seed, int(shuffle), world, rank)] = np.array(got, np.int64)
            keep = D.comm.get_rank, D.comm.get_world_size
            D.comm.get_rank, D.comm.get_world_size = (lambda r=rank: r), (lambda w=world: w)
            try:
                shard = [int(v) for v in D.InferenceSampler(size)]
            finally:
                D.comm.get_rank, D.comm.get_world_size = keep
            out["infer_s%d_w%d_r%d" % (size, world, rank)] = np.array(shard, np.int64)
    first = out["train_s7_seed63_sh1_w1_r0"][:16].tolist()
    assert first == [0, 3, 2, 6, 1, 5, 4, 0, 5, 6, 2, 1, 4, 3, 4, 1], first
    np.savez_compressed(os.path.join(HERE, "sampler.npz"), **out)
    print("sampler.npz: %d arrays" % len(out))


if __name__ == "__main__":
    main()
