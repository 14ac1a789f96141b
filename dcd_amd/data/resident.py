"""A KITTI split that stays in device memory: decoded ONCE, then every batch is B row numbers from the host.

    split = ResidentSplit(files, cfg, device, workers=None, max_bytes=None)
    images, targets = split.batch(indices, flips, img_ids=None, stream=None)

Why: the train step consumes a few hundred images per second and GPU, a PNG decode of a KITTI frame is host work of the order
of 10 ms, and a process may use 16 CPUs -- one GPU can be fed from a thread pool, the eight ranks of a node cannot.  The whole
`trainval` split is 7 481 frames x 1.4 MB = 10.4 GB as uint8, a few per cent of an MI355X's HBM, and `dcd_preprocess_images`
already reads frames out of one device buffer through per-image records.  So the frames are decoded once, by a THREAD pool
(never processes: the device must stay open in one process only, and a forked child of a process that has initialised the GPU
is not safe), go up in chunks through one reused pinned staging buffer, and stay.

What is resident:
  frames    one uint8 tensor, every frame packed HWC at a multiple of 64 bytes (the layout of `DeviceInputPipeline._pack`)
  six tables of 2 N rows, row 2 i + flip for index i of `files`, built on the host with `pack_raw` from `files.sample(i)` and
  from `flip_sample(files.sample(i))` -- the flip arithmetic stays the host's (float64; float32 for the box of a right-camera
  view, as the reference flips it), nothing changes numerically:
    records (5) int64 (byte offset, pitch, h, w, flip) | objs (M,16) f64 | kpts3d (M,n_extra,3) f64 | P (3,4) f64 |
    size (2) i32 | count () i32
  Both P matrices of every index stay on the host as well, for the `Calibration` objects of the targets.
N is `len(files)`, the number of VIEWS: with `DATASETS.USE_RIGHT_IMAGE` a `KittiFiles` of n images has N = 2 n indices (index
i >= n: the right-camera view of image i - n), so the frame buffer holds both cameras' frames -- `trainval` is then 14 962 frames,
about 20.8 GB -- and the tables have 4 n rows, two views times two flips per image.  Frame size, byte offset and `P` are looked up
per index, never per image id (two indices share one), and `nbytes`, which `max_bytes` refuses, is computed from the views.

`batch` checks the indices on the host, copies B int32 row numbers from a two-slot pinned buffer (events guard the slots, as in
the pipeline), gathers the six tables' rows in one launch (`dcd_gather_rows`), and runs the pipeline's own two kernels on the
gathered arrays: `dcd_preprocess_images` on the resident frames, `dcd_encode_targets` through `encode_packed`.  The result
equals `DeviceInputPipeline(cfg, device)(frames, samples, img_ids, flip=flips)` bit for bit (tests/test_gpu_resident.py).
There is no CPU path, and no multi-scale input (one entry in INPUT.AUG_PARAMS), as for the pipeline."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from dcd_amd import _lib
from dcd_amd.data.augment import flip_sample
from dcd_amd.data.input_pipeline import _ALIGN, _REC, _Slot, normalisation_table
from dcd_amd.data.target_encoder import encode_packed, pack_raw

_STAGE_BYTES = 64 << 20         # the pinned staging buffer of the load (grown to the largest frame if that is larger)


def default_workers(workers=None):
    """Decoding threads: at most 16, from OMP_NUM_THREADS when that is set -- never from the machine's CPU count."""
    if workers is None:
        workers = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
    return max(1, min(16, int(workers)))


class ResidentSplit:
    def __init__(self, files, cfg, device, workers=None, max_bytes=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DcdHipError("dcd_amd.data.resident keeps the split in device memory; there is no CPU path")
        if len(cfg.INPUT.AUG_PARAMS) > 1:
            raise NotImplementedError("more than one entry in AUG_PARAMS is the reference's RandomResize (multi-scale); not built")
        self.cfg, self.files = cfg, files
        self.in_w, self.in_h = cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN
        self.to_bgr = bool(cfg.INPUT.TO_BGR)
        self.workers = default_workers(workers)
        M, n_extra = cfg.DATASETS.MAX_OBJECTS, cfg.MODEL.HEAD.EXTRA_KPTS_NUM
        N = self.n_images = len(files)
        if N < 1:
            raise ValueError("the split has no images")

        # 1. host: label values (the image size comes from the file's header, nothing is decoded yet), layout, byte count
        samples = [files.sample(i) for i in range(N)]
        offsets, pos = [], 0
        for i, s in enumerate(samples):
            w, h = (int(v) for v in s["image_size"])
            if h > self.in_h or w > self.in_w or h < 1 or w < 1:
                raise ValueError("frame %d is %d x %d, the input canvas is %d x %d (multi-scale inputs are not built)"
                                 % (i, w, h, self.in_w, self.in_h))
            offsets.append(pos)
            pos += -(-3 * w * h // _ALIGN) * _ALIGN
        self.frame_bytes = pos
        both = [v for s in samples for v in (s, flip_sample(s))]             # row 2 i + flip
        objs, kpts, P, size, count = pack_raw(both, M, n_extra)
        rec = np.zeros((2 * N, _REC), np.int64)
        for i, s in enumerate(samples):
            w, h = (int(v) for v in s["image_size"])
            rec[2 * i] = (offsets[i], 3 * w, h, w, 0)
            rec[2 * i + 1] = (offsets[i], 3 * w, h, w, 1)
        tables = (rec, objs, kpts, P, size, count)
        self.nbytes = self.frame_bytes + sum(t.nbytes for t in tables)
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if self.nbytes > max_bytes:
            raise _lib.DcdHipError("the split needs %d bytes of device memory, the limit is %d (max_bytes; by default half of what is "
                                   "free): use StreamingBatches for a split that does not fit" % (self.nbytes, max_bytes))
        self._P_host = P                                                     # (2 N, 3, 4) float64
        self._sizes = [(int(s["image_size"][0]), int(s["image_size"][1])) for s in samples]
        self._offsets = offsets

        # 2. device: tables, then the frames in chunks through one pinned buffer
        with torch.cuda.device(self.device):
            self._tables = [torch.from_numpy(np.ascontiguousarray(t)).to(self.device) for t in tables]
            self._table = normalisation_table(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD).to(self.device)
            self.frames = torch.empty(self.frame_bytes, dtype=torch.uint8, device=self.device)
            self._upload()
        self._row_bytes = [t.nbytes // (2 * N) for t in tables]
        n_t = len(tables)
        self._src = (ctypes.c_void_p * n_t)(*[t.data_ptr() for t in self._tables])
        self._row_bytes_c = (ctypes.c_int64 * n_t)(*self._row_bytes)
        self._src_rows = (ctypes.c_int64 * n_t)(*([2 * N] * n_t))
        self._tails = [tuple(t.shape[1:]) for t in self._tables]
        self._slots = (_Slot(), _Slot())
        self._calls = 0

    def __len__(self):
        return self.n_images

    def _decode_into(self, view, base, i):
        w, h = self._sizes[i]
        f = self.files.frame(i)
        if f.dtype != np.uint8 or f.shape != (h, w, 3):
            raise ValueError("frame %d: expected a (%d, %d, 3) uint8 RGB array, got %s %s" % (i, h, w, f.dtype, f.shape))
        off = self._offsets[i] - base
        np.copyto(view[off:off + f.size].reshape(h, w, 3), f)

    def _upload(self):
        N = self.n_images
        ends = [self._offsets[i + 1] if i + 1 < N else self.frame_bytes for i in range(N)]
        stage_bytes = min(self.frame_bytes, max(_STAGE_BYTES, max(e - o for o, e in zip(self._offsets, ends))))
        stage = torch.zeros(stage_bytes, dtype=torch.uint8).pin_memory()      # zeros: the alignment gaps are defined bytes
        view = stage.numpy()
        done = torch.cuda.Event()
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            first = 0
            while first < N:
                last, base = first, self._offsets[first]
                while last < N and ends[last] - base <= stage_bytes:
                    last += 1
                list(pool.map(lambda i: self._decode_into(view, base, i), range(first, last)))
                used = ends[last - 1] - base
                self.frames[base:base + used].copy_(stage[:used], non_blocking=True)
                done.record()
                done.synchronize()                                           # the one buffer is free again
                first = last

    def batch(self, indices, flips, img_ids=None, stream=None):
        indices = [int(i) for i in indices]
        B = len(indices)
        if B == 0 or len(flips) != B:
            raise ValueError("%d indices for %d flip flags" % (B, len(flips)))
        if img_ids is not None and len(img_ids) != B:
            raise ValueError("%d indices for %d image ids" % (B, len(img_ids)))
        for i in indices:
            if not 0 <= i < self.n_images:
                raise IndexError("image index %d outside a split of %d images" % (i, self.n_images))
        rows = [2 * i + int(bool(f)) for i, f in zip(indices, flips)]
        slot = self._slots[self._calls % 2]
        self._calls += 1
        if slot.event is not None:
            slot.event.synchronize()                                         # the copy that last read this slot has finished
        if slot.buf is None or slot.buf.numel() < B:
            slot.buf = torch.empty(max(B, 32), dtype=torch.int32).pin_memory()
        slot.buf[:B] = torch.tensor(rows, dtype=torch.int32)
        L = _lib.lib()
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            index = torch.empty(B, dtype=torch.int32, device=dev)
            index.copy_(slot.buf[:B], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record()
            got = [torch.empty((B,) + tail, dtype=t.dtype, device=dev) for t, tail in zip(self._tables, self._tails)]
            dst = (ctypes.c_void_p * len(got))(*[t.data_ptr() for t in got])
            raw = _lib.stream_of(index)
            _lib.check(L.dcd_gather_rows(raw, len(got), self._src, dst, self._row_bytes_c, self._src_rows, index.data_ptr(), B),
                       "dcd_gather_rows")
            images = torch.empty((B, 3, self.in_h, self.in_w), dtype=torch.float32, device=dev)
            _lib.check(L.dcd_preprocess_images(raw, self.frames.data_ptr(), self.frame_bytes, got[0].data_ptr(),
                                               self._table.data_ptr(), B, self.in_h, self.in_w, int(self.to_bgr), images.data_ptr()),
                       "dcd_preprocess_images")
            targets = encode_packed(got[1:], [self._P_host[r] for r in rows], self.cfg, dev, img_ids)
        return images, targets
