"""Batch sources of a training run, and the prefetcher that runs one a batch ahead of the step.

Two sources share one interface -- `source.batch_size`, `len(source)` (images) and `source.get(k) -> (images, targets)`:

    ResidentBatches(split, batch_size, seed, rank=0, world_size=1, is_train=True)       a `ResidentSplit` in device memory
    StreamingBatches(files, pipeline, batch_size, seed, rank=0, world_size=1, workers=None)
                                                 PNG decode in a thread pool -> `DeviceInputPipeline` with explicit `flip=`;
                                                 for a split that does not fit in device memory, and the plain path

`len(source)` counts the indices of the `files` object behind it: with `DATASETS.USE_RIGHT_IMAGE` those are 2 n views of n images
(`KittiFiles`), the sampler draws from all of them, and a resident split's tables have 4 n rows (two views times two flips).

Batch k is a PURE FUNCTION of (seed, rank, world_size, k) for both: its images are positions [k B, (k + 1) B) of the rank's
`TrainingSampler` stream, its flip flags are draws [k B, (k + 1) B) of one `random.Random` stream seeded from (seed, rank), each
`random() < INPUT.AUG_PARAMS[0][0]` as `DeviceInputPipeline.draw_flips` draws them; an evaluation source walks the images in
order and never flips.  So `get(k)` after a restart gives the batch an uninterrupted run would have had at iteration k.  (The
reference restarts its sampler on resume, DGDE/data/samplers/distributed_sampler.py:43-54: a resumed run there sees the first
images of epoch 0 again.  The difference is deliberate.)  Asking for the batches in order costs nothing extra: the position in
both streams is kept, and only a jump regenerates them from the seed.

`Prefetcher(source, device, depth=1)` computes batch k + 1 on a side stream when batch k is handed over, so its copy and
kernels run while the step consumes batch k.  Before a batch is handed over the consuming stream waits for the side stream's
work on it, and every tensor handed over -- the images and every tensor field of every target -- is `record_stream`'d on the
consuming stream: the caching allocator would otherwise give their memory back to the side stream's pool, for the batch after
next to overwrite, while the step still reads it.

Evaluation over a split has a FINITE plan of its own: `EvalPlan(size, batch_size)` gives batch k = images
[k B, min((k + 1) B, size)) in file order -- the last batch may be short, nothing wraps around, nothing flips -- and
`EvalBatches(files, pipeline, batch_size, workers=None)` decodes them in a thread pool; `EvalPrefetcher` is the `Prefetcher` that
stops at the last batch; `eval_batches(files, pipeline, batch_size, workers=None, keep_frames=False)` is the two together, as the
passes walk them; `keep_frames` is the pipeline's keyword: the targets then carry the staged uint8 frames for the renderer.
`mirrored=True` (test-time augmentation) makes batch k twice as long: its B images as they are, then the same B mirrored, the
frames staged once and the samples of the second half through `flip_sample` (the pipeline's `frame_of`)."""
import random
from concurrent.futures import ThreadPoolExecutor

import torch

from dcd_amd.data.resident import default_workers
from dcd_amd.data.samplers import TrainingSampler


class _Plan:
    """Indices and flip flags of batch k; sequential requests continue the two streams, a jump regenerates them."""

    def __init__(self, size, batch_size, seed, rank, world_size, flip_p):
        if batch_size < 1:
            raise ValueError("batch size %d" % batch_size)
        self.size, self.batch_size, self.seed, self.rank = int(size), int(batch_size), int(seed), int(rank)
        self.flip_p = flip_p                                          # None: an evaluation source
        self.sampler = TrainingSampler(size, shuffle=flip_p is not None, seed=seed, rank=rank, world_size=world_size)
        self._next = None                                             # the batch number both streams stand at

    def __call__(self, k):
        B = self.batch_size
        if k < 0:
            raise ValueError("batch %d" % k)
        if self._next != k:
            self._indices = self.sampler.indices(k * B)
            self._rng = random.Random(self.seed * 1000003 + self.rank)
            for _ in range(k * B):
                self._rng.random()
        indices = [next(self._indices) for _ in range(B)]
        draws = [self._rng.random() for _ in range(B)]
        self._next = k + 1
        flips = [False] * B if self.flip_p is None else [d < self.flip_p for d in draws]
        return indices, flips


class ResidentBatches:
    def __init__(self, split, batch_size, seed, rank=0, world_size=1, is_train=True):
        self.split, self.batch_size, self.is_train = split, int(batch_size), is_train
        flip_p = float(split.cfg.INPUT.AUG_PARAMS[0][0]) if is_train else None
        self.plan = _Plan(len(split), batch_size, seed, rank, world_size, flip_p)

    def __len__(self):
        return len(self.split)

    def get(self, k):
        indices, flips = self.plan(k)
        return self.split.batch(indices, flips, img_ids=[self.split.files.img_id(i) for i in indices])


class StreamingBatches:
    def __init__(self, files, pipeline, batch_size, seed, rank=0, world_size=1, workers=None):
        self.files, self.pipeline, self.batch_size = files, pipeline, int(batch_size)
        self.is_train = pipeline.is_train
        self.plan = _Plan(len(files), batch_size, seed, rank, world_size, pipeline.flip_p if pipeline.is_train else None)
        self._pool = ThreadPoolExecutor(max_workers=default_workers(workers))

    def __len__(self):
        return len(self.files)

    def _read(self, i):
        return self.files.frame(i), self.files.sample(i)

    def get(self, k):
        indices, flips = self.plan(k)
        read = list(self._pool.map(self._read, indices))
        return self.pipeline([f for f, _ in read], [s for _, s in read], img_ids=[self.files.img_id(i) for i in indices], flip=flips)

    def close(self):
        self._pool.shutdown(wait=True)


def batch_tensors(images, targets):
    """Every device tensor of a batch: the images and each tensor field of each target."""
    out = [images]
    for t in targets:
        for name in t.fields():
            v = t.get_field(name)
            if torch.is_tensor(v) and v.is_cuda:
                out.append(v)
    return out


class Prefetcher:
    def __init__(self, source, device, depth=1):
        if depth < 1:
            raise ValueError("depth %d" % depth)
        self.source, self.device, self.depth = source, torch.device(device), int(depth)
        self.batch_size = source.batch_size
        self.side = torch.cuda.Stream(device=self.device)
        self._ready = {}                                              # k -> (batch, event recorded on the side stream after it)

    def __len__(self):
        return len(self.source)

    def _produce(self, k):
        with torch.cuda.stream(self.side):
            batch = self.source.get(k)
            event = torch.cuda.Event()
            event.record(self.side)
        self._ready[k] = (batch, event)

    def get(self, k):
        if k not in self._ready:                                      # not the one prefetched: simply compute it
            self._ready.clear()
            self._produce(k)
        batch, event = self._ready.pop(k)
        for stale in [j for j in self._ready if j < k]:
            del self._ready[stale]
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(event)
        for t in batch_tensors(*batch):
            t.record_stream(consumer)
        for j in range(k + 1, k + 1 + self.depth):
            if j not in self._ready:
                self._produce(j)
        return batch


class EvalPlan:
    """Batch k of an evaluation pass: images [k B, min((k + 1) B, size)) in order, never flipped; `len` = number of batches."""

    def __init__(self, size, batch_size):
        if batch_size < 1:
            raise ValueError("batch size %d" % batch_size)
        if size < 0:
            raise ValueError("size %d" % size)
        self.size, self.batch_size = int(size), int(batch_size)

    def __len__(self):
        return (self.size + self.batch_size - 1) // self.batch_size

    def __call__(self, k):
        if not 0 <= k < len(self):
            raise IndexError("batch %d of %d" % (k, len(self)))
        indices = list(range(k * self.batch_size, min((k + 1) * self.batch_size, self.size)))
        return indices, [False] * len(indices)


class EvalBatches:
    """`get(k) -> (images, targets)` of `EvalPlan`'s batch k through a `DeviceInputPipeline(is_train=False)`; the frames are read
    and decoded by `default_workers(workers)` threads."""

    def __init__(self, files, pipeline, batch_size, workers=None, keep_frames=False, mirrored=False):
        if pipeline.is_train:
            raise ValueError("evaluation needs a DeviceInputPipeline(is_train=False): it never flips")
        self.files, self.pipeline, self.batch_size, self.is_train = files, pipeline, int(batch_size), False
        self.keep_frames, self.mirrored = bool(keep_frames), bool(mirrored)
        self.plan = EvalPlan(len(files), batch_size)
        self._pool = ThreadPoolExecutor(max_workers=default_workers(workers))

    def __len__(self):
        return len(self.files)

    @property
    def num_batches(self):
        return len(self.plan)

    def _read(self, i):
        return self.files.frame(i), self.files.sample(i)

    def get(self, k):
        indices, _ = self.plan(k)
        read = list(self._pool.map(self._read, indices))
        extra = {"keep_frames": True} if self.keep_frames else {}
        frames, samples, ids = [f for f, _ in read], [s for _, s in read], [self.files.img_id(i) for i in indices]
        if self.mirrored:                                              # the B frames as they are, then the same B mirrored
            B = len(frames)
            return self.pipeline(frames, samples + samples, img_ids=ids + ids, flip=[False] * B + [True] * B,
                                 frame_of=list(range(B)) * 2, **extra)
        return self.pipeline(frames, samples, img_ids=ids, **extra)

    def close(self):
        self._pool.shutdown(wait=True)


class EvalPrefetcher(Prefetcher):
    """`Prefetcher` over a finite source: nothing is produced past `source.num_batches`."""

    def _produce(self, k):
        if k < self.source.num_batches:
            super()._produce(k)


class eval_batches:
    """A split in evaluation order, one batch ahead: `EvalBatches` behind an `EvalPrefetcher` on the pipeline's device.

        with eval_batches(files, pipeline, batch_size, workers) as walk:
            for k, indices, images, targets in walk:          # k = 0 .. num_batches - 1; indices: the batch's image numbers

    Leaving the `with` block, by its end or by an exception, shuts the thread pool down."""

    def __init__(self, files, pipeline, batch_size, workers=None, keep_frames=False, mirrored=False):
        self.source = EvalBatches(files, pipeline, batch_size, workers, keep_frames, mirrored) if mirrored else \
            EvalBatches(files, pipeline, batch_size, workers, keep_frames)
        self._batches = EvalPrefetcher(self.source, pipeline.device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.source.close()

    def __iter__(self):
        for k in range(self.source.num_batches):
            images, targets = self._batches.get(k)
            yield k, self.source.plan(k)[0], images, targets
