"""GMW's training records collected on the device, batch after batch (csrc/records.hip, `dcd_gmw_train_records`).

The reference's collection pass (DGDE/engine/trainer.py:97-129, :208-215) runs the whole loss under TEST.GENERATE_GMW and keeps, per
iteration, what `Loss_Computation.generate_data` copies to the host; the file `gen_data_train.json` is the only way to GMW.  Here
the same records go from the predictor's `reg_pois` and the target tables straight into six tables in device memory:

    collector = TrainRecordCollector(cfg, device, capacity, max_calls)
    collector.add(reg_pois, targets, image_numbers)        # one C call: three launches, nothing read back
    records = collector.finish()                           # the ONLY host read: the cursor and the per-call counts
    data = collector.gen_data()                            # on request: the `Loss_Computation.gen_data` dict, one bulk copy

`records_spec(cfg)` names the configurations the kernel covers and refuses the others with NotImplementedError, as
`PostProcessor.decode_spec` does for the fused decode: multi-bin orientation with at most 4 bins, at most 128 key points,
`CORNER_LOSS_DEPTH == 'edges'`.
"""
import ctypes

import numpy as np
import torch

from dcd_amd import _lib
from dcd_amd.model.layers.utils import Converter_key2channel
from dcd_amd.structures.params_3d import _typed, stack_field
from .data import KEYS, ResidentRecords

TABLES = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "pred_location")
_HEADS = {"ch_offset": "3d_offset", "ch_ori_cls": "ori_cls", "ch_ori_off": "ori_offset", "ch_kpts2d": "extra_kpts_2d",
          "ch_kpts3d": "extra_kpts_3d"}
# (field of the targets, dtype the kernel reads), in the entry point's order
_TARGETS = (("reg_mask", torch.uint8), ("target_centers", torch.int32), ("offset_3D", torch.float32), ("rotys", torch.float32),
            ("locations", torch.float32), ("Calib_P", torch.float32), ("pad_size", torch.int64))


def records_spec(cfg):
    """The configuration `dcd_gmw_train_records` needs, or NotImplementedError with the reason."""
    head = cfg.MODEL.HEAD
    if cfg.INPUT.ORIENTATION != 'multi-bin':
        raise NotImplementedError("gmw_records: head-axis orientation is not covered by the kernel (multi-bin only)")
    n_bins = int(cfg.INPUT.ORIENTATION_BIN_SIZE)
    if not 1 <= n_bins <= 4:
        raise NotImplementedError("gmw_records: %d orientation bins (4 at most)" % n_bins)
    if head.CORNER_LOSS_DEPTH != 'edges':
        raise NotImplementedError("gmw_records: MODEL.HEAD.CORNER_LOSS_DEPTH = %r (the records take their depth from the edges)"
                                  % (head.CORNER_LOSS_DEPTH,))
    k2c = Converter_key2channel(keys=head.REGRESSION_HEADS, channels=head.REGRESSION_CHANNELS)
    missing = [name for name in _HEADS.values() if name not in k2c.keys]
    if missing:
        raise NotImplementedError("gmw_records needs the heads %s" % ", ".join(missing))
    nk = int(head.EXTRA_KPTS_NUM) + 10
    if nk > 128:
        raise NotImplementedError("gmw_records: %d key points (128 at most)" % nk)
    spec = {f: k2c(name).start for f, name in _HEADS.items()}
    if k2c('extra_kpts_2d').stop - k2c('extra_kpts_2d').start != 2 * nk or k2c('extra_kpts_3d').stop - k2c('extra_kpts_3d').start != 3 * nk:
        raise NotImplementedError("gmw_records: the key-point heads do not hold %d key points" % nk)
    spec.update(nk=nk, n_bins=n_bins, down_ratio=float(cfg.MODEL.BACKBONE.DOWN_RATIO), C=sum(sum(g) for g in head.REGRESSION_CHANNELS),
                M=int(cfg.DATASETS.MAX_OBJECTS))
    return spec


def _entry(device):
    """(workspace size query, entry point) for tensors on `device`.  The library has no host path; the tests put the host build
    of csrc/records_math.h here."""
    if torch.device(device).type != "cuda":
        raise _lib.DcdHipError("dcd_amd.gmw.collect runs on the GPU only; there is no CPU path")
    L = _lib.lib()
    return L.dcd_gmw_train_records_workspace_bytes, L.dcd_gmw_train_records


def calib_rows(calibs):
    """(B, 6) float32 rows [c_u, c_v, f_u, f_v, b_x, b_y] on the host: the values of `Anno_Encoder._calib_table`."""
    return np.array([(float(c.c_u), float(c.c_v), float(c.f_u), float(c.f_v), float(c.b_x), float(c.b_y)) for c in calibs],
                    dtype=np.float32).reshape(len(calibs), 6)


class _Staging:
    """Two pinned host rows used alternately for the (B, 6) calibration table of a call: the copy is asynchronous, and a row is
    rewritten only after the copy that last read it has finished (the rule of `ResidentRecords.batch`)."""

    def __init__(self):
        self.slots, self.calls = [[None, None], [None, None]], 0

    def upload(self, rows, device):
        host = torch.from_numpy(rows)
        if device.type != "cuda":
            return host.clone()
        slot = self.slots[self.calls % 2]
        self.calls += 1
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < host.numel():
            slot[0] = torch.empty(max(host.numel(), 6 * 32), dtype=torch.float32).pin_memory()
        slot[0][:host.numel()].copy_(host.reshape(-1))
        with torch.cuda.device(device):
            out = torch.empty(tuple(host.shape), dtype=torch.float32, device=device)
            out.view(-1).copy_(slot[0][:host.numel()], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
        return out


class TrainRecordCollector:
    def __init__(self, cfg, device, capacity, max_calls):
        self.device = torch.device(device)
        self.spec = records_spec(cfg)
        self.capacity, self.max_calls = int(capacity), int(max_calls)
        if self.capacity < 1 or self.max_calls < 1:
            raise ValueError("capacity %d, max_calls %d" % (self.capacity, self.max_calls))
        nk, dev = self.spec["nk"], self.device
        tails = {"kpts_2d": (nk, 2), "kpts_3d": (nk, 3), "pred_rot": (1,), "gt_location": (3,), "pred_location": (3,)}
        self.tables = {k: torch.zeros((self.capacity,) + tails[k], dtype=torch.float32, device=dev) for k in TABLES}
        self.image = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=dev)
        self.per_call = torch.zeros(self.max_calls, dtype=torch.int32, device=dev)
        self.calls = 0
        self.img_ids = []                      # per call: the images' `img_idx` strings, for the wire format
        self._workspace = None
        self._staging = _Staging()
        self._counts = None
        self._numbers = []                     # per call: the image numbers as handed in (device), for the wire format

    # ------------------------------------------------------------------------------------------------------------------
    def args(self, B, M, C):
        a = _lib.RecordsArgs()
        a.B, a.M, a.C, a.nk, a.n_bins = int(B), int(M), int(C), self.spec["nk"], self.spec["n_bins"]
        for k in _HEADS:
            setattr(a, k, int(self.spec[k]))
        a.down_ratio = self.spec["down_ratio"]
        return a

    def add(self, reg_pois, targets, image_numbers):
        """reg_pois (B, M, C): the predictor's output at the target centres; targets: the batch's [ParamsList]; image_numbers:
        B int32 numbers on the device (the split's row numbers), stored with each record."""
        if self._counts is not None:
            raise RuntimeError("the collection is finished")
        if self.calls >= self.max_calls:
            raise RuntimeError("more than max_calls = %d calls" % self.max_calls)
        dev = self.device
        sizer, entry = _entry(dev)
        pois = reg_pois.detach()
        if pois.dtype != torch.float32:
            pois = pois.float()
        pois = pois.contiguous()
        B, M, C = pois.shape
        fields = [_typed(stack_field(targets, name), dt) for name, dt in _TARGETS]
        if tuple(fields[0].shape) != (B, M):
            raise ValueError("reg_mask is %s, reg_pois %s" % (tuple(fields[0].shape), tuple(pois.shape)))
        calib = self._staging.upload(calib_rows([t.get_field("calib") for t in targets]), dev)
        numbers = _typed(image_numbers, torch.int32)
        if numbers.numel() != B or numbers.device != pois.device:
            raise ValueError("image_numbers: %d entries on %s for a batch of %d on %s" % (numbers.numel(), numbers.device, B, pois.device))
        a = self.args(B, M, C)
        need = int(sizer(B, M, a.nk))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        stream = _lib.stream_of(pois) if dev.type == "cuda" else None
        st = entry(stream, pois.data_ptr(), ctypes.byref(a), *[t.data_ptr() for t in fields], calib.data_ptr(), numbers.data_ptr(),
                   self.capacity, *[self.tables[k].data_ptr() for k in TABLES], self.image.data_ptr(), self.cursor.data_ptr(),
                   self.per_call.data_ptr(), self.calls, self.max_calls, self._workspace.data_ptr(), self._workspace.numel())
        _lib.check(st, "dcd_gmw_train_records")
        self.img_ids.append([t.get_field("img_idx") if t.has_field("img_idx") else None for t in targets])
        self._numbers.append(numbers)
        self.calls += 1

    # ------------------------------------------------------------------------------------------------------------------
    def _read_counts(self):
        """The one host read: (records in all, [records of call 0, 1, ...])."""
        if self._counts is None:
            if self.calls == 0:
                raise RuntimeError("nothing was collected")
            host = torch.cat((self.cursor, self.per_call[:self.calls])).cpu().tolist()
            total, per_call = host[self.calls & 1], host[2:]
            if total > self.capacity:
                raise RuntimeError("%d records were produced, the tables hold %d: the surplus was not written" % (total, self.capacity))
            self._counts = (int(total), [int(c) for c in per_call])
        return self._counts

    def __len__(self):
        return self._read_counts()[0]

    def finish(self):
        """`ResidentRecords` over the first n rows of the device tables: views, nothing passes through the host."""
        n, _ = self._read_counts()
        return ResidentRecords.from_device({k: self.tables[k][:n] for k in KEYS})

    def images(self):
        """The `image` column of the records (int32, on the device)."""
        return self.image[:self._read_counts()[0]]

    def gen_data(self):
        """The dict `Loss_Computation.gen_data` holds after the same batches (engine/gen_data.py): lists per call, `img_idx` the
        images' id strings (an image without one gives its number), `weight_img` empty.  ONE device-to-host copy: the tables,
        the `image` column and the calls' image numbers (which must be distinct within a call) as one flat buffer."""
        n, per_call = self._read_counts()
        nk = self.spec["nk"]
        as_f32 = lambda t: t.reshape(-1).view(torch.float32)  # noqa: E731  (int32 words travel as they are)
        parts = [self.tables[k][:n].reshape(-1) for k in TABLES] + [as_f32(self.image[:n])] + [as_f32(t) for t in self._numbers]
        flat = torch.cat(parts).cpu().numpy()
        sizes = [nk * 2, nk * 3, 1, 3, 3]
        cols, at = {}, 0
        for k, w in zip(TABLES, sizes):
            cols[k] = flat[at:at + n * w].reshape(n, w)
            at += n * w
        image = flat[at:at + n].view(np.int32)
        at += n
        cuts = np.cumsum([0] + per_call)
        out = {k: [] for k in ('kpts_2d', 'kpts_3d', 'pred_rot', 'gt_location', 'pred_location', 'weight_img', 'img_idx')}
        for c, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            names = self.img_ids[c]
            numbers = flat[at:at + len(names)].view(np.int32).tolist()
            at += len(names)
            name_of = {v: (names[b] if names[b] is not None else str(v)) for b, v in enumerate(numbers)}
            out['kpts_2d'].append(cols['kpts_2d'][lo:hi].reshape(-1, nk, 2).tolist())
            out['kpts_3d'].append(cols['kpts_3d'][lo:hi].reshape(-1, nk, 3).tolist())
            out['pred_rot'].append(cols['pred_rot'][lo:hi, 0].tolist())
            out['gt_location'].append(cols['gt_location'][lo:hi].tolist())
            out['pred_location'].append(cols['pred_location'][lo:hi].tolist())
            out['img_idx'].append([name_of[v] for v in image[lo:hi].tolist()])
        return out
