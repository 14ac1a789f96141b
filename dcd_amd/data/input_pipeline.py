"""The input pipeline on the device: decoded uint8 frames and parsed label values in, the `(images, targets)` pair of
`KeypointDetector.forward` / `train_step` / `GraphedTrainStep` out -- flipped, padded and normalised as the reference's
`KITTIDataset.__getitem__` would have (DGDE/data/datasets/kitti.py:299-320, :608), with targets that agree with the flipped image.

    pipe = DeviceInputPipeline(cfg, device, is_train=True, seed=None)
    images, targets = pipe(frames, samples, img_ids=None, flip=None, stream=None, keep_frames=False)

What runs where: the flip of the label values on the host (dcd_amd/data/augment.py, a few dozen scalars per image), the image
work -- `RandomHorizontallyFlip`, `pad_image`, `ToTensor`, `Normalize`, `TO_BGR` -- in ONE launch per batch (csrc/images.hip,
`dcd_preprocess_images`), the target encoding in one more (`encode_targets`).  The frames travel as uint8: they are packed, with
their per-image records in front, into one pinned host buffer and go up in one non-blocking copy (11 MB for eight KITTI frames
instead of 47 MB of fp32).  There are two pinned slots, each guarded by an event recorded after its copy and waited on before
the slot is overwritten, so a caller may run the pipeline on a side stream one batch ahead of the step that consumes it (the
results are allocated on that stream: the consumer waits on it, `torch.cuda.current_stream().wait_stream(side)`, as for any tensor).

The normalisation is a 3 x 256 table built here once with the torch operations `ToTensor` / `Normalize` apply, so the kernel
only moves data and the images are bit-equal to the reference's.  There is no CPU path."""
import random

import numpy as np
import torch

from dcd_amd import _lib
from dcd_amd.data.augment import flip_sample
from dcd_amd.data.target_encoder import encode_targets

_REC = 5            # int64 per image in front of the pixels: byte offset, row pitch, height, width, flip (include/dcd_hip.h)
_ALIGN = 64


def normalisation_table(mean, std):
    """(3, 256) fp32: entry [k][v] is what `ToTensor` + `Normalize` (transforms.py:14-25) make of byte v in channel k."""
    v = torch.arange(256, dtype=torch.uint8).float().div(255)
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    return v[None, :].repeat(3, 1).sub(mean[:, None]).div(std[:, None]).contiguous()


class _Slot:
    def __init__(self):
        self.buf = None         # pinned uint8
        self.event = None       # recorded after the last copy out of `buf`


class DeviceInputPipeline:
    def __init__(self, cfg, device, is_train=True, seed=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DcdHipError("dcd_amd.data.input_pipeline runs on the GPU only; there is no CPU path")
        aug = cfg.INPUT.AUG_PARAMS if is_train else cfg.DATASETS.TTA_AUG_PARAMS
        if len(aug) > 1:
            raise NotImplementedError("more than one entry in AUG_PARAMS is the reference's RandomResize (multi-scale); not built")
        self.cfg, self.is_train = cfg, is_train
        self.flip_p = float(cfg.INPUT.AUG_PARAMS[0][0]) if is_train else 0.0
        self.in_w, self.in_h = cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN
        self.to_bgr = bool(cfg.INPUT.TO_BGR)
        self._table_host = normalisation_table(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD)
        self._table = None
        self._rng = random.Random(seed)
        self._slots = (_Slot(), _Slot())
        self._calls = 0
        self.last_flip = []

    def draw_flips(self, n):
        """n flags from the object's own generator: p = INPUT.AUG_PARAMS[0][0] in training, never in evaluation."""
        if not self.is_train:
            return [False] * n
        return [self._rng.random() < self.flip_p for _ in range(n)]

    def _pack(self, frames, flags, frame_of=None):
        """Frames -> (pinned buffer slot, used bytes).  Layout: (B, 5) int64 records, then the images, each packed HWC.
        frame_of: None, one record per frame in order; or, for every record, the index of the frame it reads: a record names its
        pixels by byte offset, so two records (a frame and its mirrored view) share one copy of them."""
        B = len(frames) if frame_of is None else len(frame_of)
        arrays, offsets = [], []
        nbytes = -(-B * _REC * 8 // _ALIGN) * _ALIGN
        for i, f in enumerate(frames):
            a = f.numpy() if torch.is_tensor(f) else np.asarray(f)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("frame %d: expected a (h, w, 3) uint8 RGB array, got %s %s" % (i, a.dtype, a.shape))
            if a.shape[0] > self.in_h or a.shape[1] > self.in_w or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError("frame %d is %d x %d, the input canvas is %d x %d (multi-scale inputs are not built)"
                                 % (i, a.shape[1], a.shape[0], self.in_w, self.in_h))
            arrays.append(a)
            offsets.append(nbytes)
            nbytes += -(-a.size // _ALIGN) * _ALIGN
        slot = self._slots[self._calls % 2]
        self._calls += 1
        if slot.event is not None:
            slot.event.synchronize()                    # the copy that last read this slot has finished
        if slot.buf is None or slot.buf.numel() < nbytes:
            slot.buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        view = slot.buf.numpy()
        rec = view[:B * _REC * 8].view(np.int64).reshape(B, _REC)
        for a, off in zip(arrays, offsets):
            np.copyto(view[off:off + a.size].reshape(a.shape), a)
        for i, j in enumerate(range(B) if frame_of is None else frame_of):
            h, w = arrays[j].shape[:2]
            rec[i] = (offsets[j], 3 * w, h, w, int(bool(flags[i])))
        return slot, nbytes

    def __call__(self, frames, samples, img_ids=None, flip=None, stream=None, keep_frames=False, frame_of=None):
        """frame_of: None, or for each of the R samples the index of its frame in `frames`: R images come back from len(frames)
        staged frames, each staged once however many samples name it (a frame and its mirrored view, as the evaluation with
        test-time augmentation asks for them: `EvalBatches(mirrored=True)`); every target then also carries "image_size", the
        image's own (w, h) on the host.
        keep_frames: every target also carries "frames" -- the staged uint8 buffer on the device, `_pack`'s layout, the same
        tensor for all B -- "frame_records", its (B, 5) int64 record table (a view of its head), and "frame_size", the image's own
        (w, h) on the host: what `ops.render_detections` draws on.  Without the flag the staged buffer is let go as before."""
        if frame_of is not None:
            frame_of = [int(j) for j in frame_of]
            if len(frames) == 0 or any(not 0 <= j < len(frames) for j in frame_of):
                raise ValueError("frame_of %s names a frame outside 0 .. %d" % (frame_of, len(frames) - 1))
        B = len(frames) if frame_of is None else len(frame_of)
        if B == 0 or len(samples) != B:
            raise ValueError("%d frames for %d samples" % (B, len(samples)))
        of_sample = frames if frame_of is None else [frames[j] for j in frame_of]
        for i, (f, s) in enumerate(zip(of_sample, samples)):
            if tuple(int(v) for v in s["image_size"]) != (int(f.shape[1]), int(f.shape[0])):
                raise ValueError("sample %d: image_size %s, frame is %d x %d" % (i, tuple(s["image_size"]), f.shape[1], f.shape[0]))
        flags = self.draw_flips(B) if flip is None else [bool(v) for v in flip]
        if len(flags) != B:
            raise ValueError("%d flip flags for %d frames" % (len(flags), B))
        slot, nbytes = self._pack(frames, flags) if frame_of is None else self._pack(frames, flags, frame_of)
        L = _lib.lib()
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if self._table is None:
                self._table = self._table_host.to(self.device)
            staged = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            staged.copy_(slot.buf[:nbytes], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record()
            images = torch.empty((B, 3, self.in_h, self.in_w), dtype=torch.float32, device=self.device)
            _lib.check(L.dcd_preprocess_images(_lib.stream_of(images), staged.data_ptr(), nbytes, staged.data_ptr(),
                                               self._table.data_ptr(), B, self.in_h, self.in_w, int(self.to_bgr), images.data_ptr()),
                       "dcd_preprocess_images")
            targets = encode_targets([flip_sample(s) if f else s for s, f in zip(samples, flags)], self.cfg, self.device, img_ids)
            if frame_of is not None:
                for t, s in zip(targets, samples):
                    t.add_field("image_size", tuple(int(v) for v in s["image_size"]))
            if keep_frames:
                records = staged[:B * _REC * 8].view(torch.int64).view(B, _REC)
                for t, f in zip(targets, of_sample):
                    t.add_field("frames", staged)
                    t.add_field("frame_records", records)
                    t.add_field("frame_size", (int(f.shape[1]), int(f.shape[0])))
        self.last_flip = flags
        return images, targets
