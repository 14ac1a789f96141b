"""GMW's training records (`gen_data_train.json`, dcd_amd/engine/gen_data.py) as flat tables that stay in device memory.

The reference reads the file into a `torch.utils.data.Dataset` of numpy rows (GMW/utilities/dataset_utilities.py:11-73) and lets a
`DataLoader` with a `DistributedSampler` collate batches of 16 on worker processes (GMW/main.py:95-121).  An object is 1.5 KB --
73 x 2 + 73 x 3 + 1 + 3 floats -- so KITTI's cars are about 20 MB: the four tables go up once and a batch is B row numbers from
the host plus ONE `dcd_gather_rows` launch.

  load_train_data   {'kpts_2d': [iteration][object][73][2], 'kpts_3d': [..][73][3], 'pred_rot': [..], 'gt_location': [..][3]}
                    (a path or the parsed JSON) -> float32 `kpts_2d` (N,73,2), `kpts_3d` (N,73,3), `pred_rot` (N,1),
                    `gt_location` (N,3), iteration after iteration, object after object (the reference's order); an iteration
                    without objects adds nothing.
  ResidentRecords   the four tables on `device`; `batch(index)` -> (kpts_2d, kpts_3d, pred_rot, gt_location) of those rows.  On
                    the CPU the same call is an `index_select`.
  epoch_order       the indices `DistributedSampler(shuffle=True, seed=seed)` yields after `set_epoch(epoch)`.  The reference's
                    single-GPU branch shuffles from the global generator instead and cannot be reproduced; the distributed rule is
                    used at EVERY world size on purpose: batch k of epoch e is a function of (seed, e, k, rank, world_size), so a
                    resumed run continues its stream.
"""
import ctypes
import json
import math
import os

import numpy as np
import torch

KEYS = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location")
_TAILS = {"kpts_2d": (73, 2), "kpts_3d": (73, 3), "pred_rot": (1,), "gt_location": (3,)}


def load_train_data(path_or_dict):
    if isinstance(path_or_dict, (str, os.PathLike)):
        with open(path_or_dict, "r") as f:
            path_or_dict = json.load(f)
    data = path_or_dict
    rows = {k: [] for k in KEYS}
    for i in range(len(data["kpts_2d"])):
        for j in range(len(data["kpts_2d"][i])):
            rows["kpts_2d"].append(np.array(data["kpts_2d"][i][j]))
            rows["kpts_3d"].append(np.array(data["kpts_3d"][i][j]))
            rows["pred_rot"].append([data["pred_rot"][i][j]])
            rows["gt_location"].append(np.array(data["gt_location"][i][j]))
    n = len(rows["kpts_2d"])
    if n == 0:
        return {k: np.zeros((0,) + _TAILS[k], np.float32) for k in KEYS}
    out = {k: np.array(rows[k], dtype=np.float32) for k in KEYS}          # float64 values rounded once, as the reference does
    out["pred_rot"] = out["pred_rot"].reshape(n, 1)
    out["gt_location"] = out["gt_location"].reshape(n, 3)
    return out


def epoch_order(n, epoch, seed=0, rank=0, world_size=1):
    """`list(DistributedSampler(range(n), num_replicas=world_size, rank=rank, shuffle=True, seed=seed))` after `set_epoch(epoch)`:
    randperm(n) from a generator seeded with seed + epoch, padded with its own head to a multiple of the world size, strided."""
    if n < 1:
        raise ValueError("epoch_order needs a positive size, got %d" % n)
    if not 0 <= rank < world_size:
        raise ValueError("rank %d outside a world of %d" % (rank, world_size))
    g = torch.Generator()
    g.manual_seed(int(seed) + int(epoch))
    indices = torch.randperm(n, generator=g).tolist()
    total = int(math.ceil(n / world_size)) * world_size
    pad = total - len(indices)
    if pad <= len(indices):
        indices += indices[:pad]
    else:
        indices += (indices * int(math.ceil(pad / len(indices))))[:pad]
    return indices[rank:total:world_size]


class _Slot:
    buf = None
    event = None


class ResidentRecords:
    def __init__(self, data, device):
        self.device = torch.device(device)
        self.n = int(data["kpts_2d"].shape[0])
        if self.n < 1:
            raise ValueError("no training records")
        self._adopt([torch.from_numpy(np.ascontiguousarray(data[k], dtype=np.float32)).to(self.device) for k in KEYS])

    @classmethod
    def from_device(cls, tables):
        """Records that already lie in device (or host) memory: {key: float32 tensor (n, ...)} for the four `KEYS`, all on one
        device, adopted as they are -- views of larger tables included, nothing is copied (gmw/collect.py)."""
        ts = [tables[k] for k in KEYS]
        for k, t in zip(KEYS, ts):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != ts[0].device:
                raise ValueError("from_device: %s must be a contiguous float32 tensor on %s" % (k, ts[0].device))
        self = cls.__new__(cls)
        self.device = ts[0].device
        self.n = int(ts[0].shape[0])
        if self.n < 1:
            raise ValueError("no training records")
        self._adopt(ts)
        return self

    def _adopt(self, tables):
        self.tables = list(tables)
        for t in self.tables:
            if t.shape[0] != self.n:
                raise ValueError("the tables of the records disagree in length")
        self._tails = [tuple(t.shape[1:]) for t in self.tables]
        if self.device.type == "cuda":
            n_t = len(self.tables)
            row_bytes = [t[0].numel() * 4 for t in self.tables]
            self._src = (ctypes.c_void_p * n_t)(*[t.data_ptr() for t in self.tables])
            self._row_bytes = (ctypes.c_int64 * n_t)(*row_bytes)
            self._src_rows = (ctypes.c_int64 * n_t)(*([self.n] * n_t))
            self._slots = (_Slot(), _Slot())
            self._calls = 0

    def __len__(self):
        return self.n

    def batch(self, index):
        rows = [int(i) for i in index]
        B = len(rows)
        if B == 0:
            raise ValueError("an empty batch")
        for i in rows:
            if not 0 <= i < self.n:
                raise IndexError("record %d outside a table of %d rows" % (i, self.n))
        if self.device.type != "cuda":
            idx = torch.tensor(rows, dtype=torch.long)
            return tuple(t.index_select(0, idx) for t in self.tables)
        from dcd_amd import _lib
        slot = self._slots[self._calls % 2]
        self._calls += 1
        if slot.event is not None:
            slot.event.synchronize()                                         # the copy that last read this slot has finished
        if slot.buf is None or slot.buf.numel() < B:
            slot.buf = torch.empty(max(B, 32), dtype=torch.int32).pin_memory()
        slot.buf[:B] = torch.tensor(rows, dtype=torch.int32)
        dev = self.device
        with torch.cuda.device(dev):
            idx = torch.empty(B, dtype=torch.int32, device=dev)
            idx.copy_(slot.buf[:B], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record()
            got = [torch.empty((B,) + tail, dtype=torch.float32, device=dev) for tail in self._tails]
            dst = (ctypes.c_void_p * len(got))(*[t.data_ptr() for t in got])
            _lib.check(_lib.lib().dcd_gather_rows(_lib.stream_of(idx), len(got), self._src, dst, self._row_bytes, self._src_rows,
                                                  idx.data_ptr(), B), "dcd_gather_rows")
        return tuple(got)
