"""GMW inference: from a detector's `gen_data_infer.json` records to refined KITTI result files and their AP.

The reference does this inside its training script: `load_data('valid')` (GMW/utilities/dataset_utilities.py:38-54) flattens the
records, `validate` (GMW/main.py:524-548) re-weights the 2628 edge depths of every detection and moves the box along its viewing
ray, `GMW_data` (main.py:123-215) rewrites the result files and calls the KITTI evaluation.  Here:

  load_infer_data   the records (a path, the parsed JSON, or the numpy-view records of `engine.gen_data.infer_records_batch`)
                    as flat float32 arrays;
  extract_features  one extractor under no_grad, every residual block's tail (context norm -> ReLU -> + input) as one kernel;
  refine            batches of 256 objects: `ops.compute_z`, the two extractors, `ops.gmw_refine`.  Neither the 2628 x 2628
                    distance matrix nor the transport plan is formed -- refinement reads `1 / diag(M)` only.  `fused=False` is the
                    stock chain (`F.normalize`, the diagonal of `pairwise_l2_dist`, `compute_reg_loss`) in the model's dtype on
                    any device: what the tests measure against, and in float64 their reference;
  refine_packed     the body of that loop on device tensors that are already in the extractors' layout;
  PackBuffers       a group of records in that layout on the device: the buffers `ops.gmw_pack_records` fills and
                    `refine_packed` reads, with the checks both users need;
  RecordRefiner     the same refinement fed from a detector's decode on the device: `ops.gmw_pack_records` gathers the kept
                    candidates of each image batch into `batch_size` accumulation buffers (`plan_packs` splits a call at the
                    capacity), a full buffer is refined and its result copied to a pinned slot behind an event;
  writer_fields     what `write_results` needs beside the locations, from the detector's float32 rows;
  write_results     the files of `GMW_data`, byte for byte;
  evaluate          refine -> write -> `eval.kitti_ap.evaluate`.
"""
import json
import math
import os

import numpy as np
import torch
from torch.nn import functional as F

from .model import pairwise_l2_dist
from .step import compute_reg_loss

NUM_KPTS = 73


def _scalar(v):
    """`pred_rot` / `score` of a record: a number, a one-element list (engine.gen_data) or a one-element array."""
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def load_infer_data(path_or_dict):
    """{img_id: [record, ...]} -> dict of flat arrays, one row per record in file order (dataset_utilities.py:38-54):
    float32 `kpts_2d` (N,73,2), `kpts_3d` (N,73,3), `pred_rot` (N,1), `pred_location` (N,3), `dim` (N,3); `img_idx`, the list of
    (img_id, index in the image's list); and what only the writer needs, in float64 as the JSON holds it: `box` (N,4), `score`
    (N), `dim_out` (N,3), `rot_out` (N).  Only the first 73 keypoints of a record are kept."""
    if isinstance(path_or_dict, (str, os.PathLike)):
        with open(path_or_dict, "r") as f:
            path_or_dict = json.load(f)
    k2, k3, rot, loc, dim, idx, box, score = [], [], [], [], [], [], [], []
    for img, records in path_or_dict.items():
        for i, a in enumerate(records):
            k2.append(np.asarray(a["kpts_2d"], dtype=np.float32).reshape(-1, 2)[:NUM_KPTS])
            k3.append(np.asarray(a["kpts_3d"], dtype=np.float32).reshape(-1, 3)[:NUM_KPTS])
            rot.append(_scalar(a["pred_rot"]))
            loc.append(np.asarray(a["pred_location"], dtype=np.float64).reshape(3))
            dim.append(np.asarray(a["dim"], dtype=np.float64).reshape(3))
            box.append(np.asarray(a["box"], dtype=np.float64).reshape(4))
            score.append(_scalar(a["score"]))
            idx.append((img, i))
    n = len(idx)
    dim64, rot64 = np.array(dim, np.float64).reshape(n, 3), np.array(rot, np.float64).reshape(n)
    return {
        "kpts_2d": np.array(k2, np.float32).reshape(n, NUM_KPTS, 2),
        "kpts_3d": np.array(k3, np.float32).reshape(n, NUM_KPTS, 3),
        "pred_rot": rot64.astype(np.float32).reshape(n, 1),
        "pred_location": np.array(loc, np.float64).reshape(n, 3).astype(np.float32),
        "dim": dim64.astype(np.float32),
        "img_idx": idx,
        "box": np.array(box, np.float64).reshape(n, 4),
        "score": np.array(score, np.float64).reshape(n),
        "dim_out": dim64,
        "rot_out": rot64,
    }


def extract_features(model, which, x):
    """`model.<which>` ("FeatureExtractor4d" / "FeatureExtractor6d") on x (B, C_in, K) -> (B, 128, K) without gradients, walking
    `conv_in` and the residual blocks with each block's tail -- context norm, ReLU, + input -- as one kernel
    (`ops.context_norm_relu_add`) instead of three launches and five passes over the activation.  Device fp32 only."""
    from dcd_amd import ops
    mod = getattr(model, which)
    with torch.no_grad():
        h = mod.conv_in(x)
        for i in range(mod.numlayer):
            block = getattr(mod, "conv_%d" % i)
            t = block.conv2[0](block.conv1(block.preconv(h)))
            h = ops.context_norm_relu_add(t, h, 1e-3)
    return h


def _stock_weights(model, e4, e6, chunk=4):
    """1 / diag(M) as `GMW.graph_matching` forms it, `chunk` objects at a time (M is 2628 x 2628 per object)."""
    out = []
    for s in range(0, e4.shape[0], chunk):
        f4 = model.FeatureExtractor4d(e4[s:s + chunk].transpose(-2, -1)).transpose(-2, -1)
        f6 = model.FeatureExtractor6d(e6[s:s + chunk].transpose(-2, -1)).transpose(-2, -1)
        M = pairwise_l2_dist(F.normalize(f4, p=2, dim=-1), F.normalize(f6, p=2, dim=-1))
        out.append(1.0 / M.diagonal(offset=0, dim1=-2, dim2=-1))
    return torch.cat(out, 0)


def relocate(raw_location, dim, pred_depth):
    """The location rule of main.py:542-547: about the object's centre (y is the bottom face), along the viewing ray."""
    loc = raw_location.clone()
    scale = pred_depth / loc[:, 2]
    h = dim[:, 0]
    loc[:, 1] -= h / 2
    pred_location = scale.unsqueeze(-1) * loc
    pred_location[:, 1] += h / 2
    return pred_location


def refine_packed(model, e4, e6, k2, k3, rot, loc, dim, compute_z=None):
    """The refinement of B records that already lie on the device in the layout the extractors take: e4 (B, 4, P) / e6 (B, 6, P)
    = `edge_expand(k).transpose(-2, -1).contiguous()` (what `ops.gmw_pack_records` writes), k2 (B, 73, 2), k3 (B, 73, 3),
    rot (B, 1), loc / dim (B, 3), float32.  Returns (pred_depth (B), pred_location (B, 3)) on the device; nothing is read back.
    `compute_z` defaults to the HIP solver kernel."""
    from dcd_amd import ops
    with torch.no_grad():
        pre_depths, good_idx = (compute_z or ops.compute_z)(k2, k3, rot)
        f4 = extract_features(model, "FeatureExtractor4d", e4)
        f6 = extract_features(model, "FeatureExtractor6d", e6)
        _, z, ploc = ops.gmw_refine(f4, f6, pre_depths, good_idx, loc, dim)
    return z, ploc


def plan_packs(n_new, filled, cap):
    """How one `RecordRefiner.add` of n_new records goes into buffers of `cap` records that already hold `filled` (< cap): the
    list of (start, count, flush) pieces -- records [start, start + count) of the call are packed behind what is there, and the
    buffers are flushed after a piece that fills them.  The pieces cover [0, n_new) in order and none crosses the capacity."""
    if cap < 1 or not 0 <= filled < cap or n_new < 0:
        raise ValueError("plan_packs: n_new %d, filled %d, capacity %d" % (n_new, filled, cap))
    pieces, start = [], 0
    while start < n_new:
        count = min(n_new - start, cap - filled)
        filled += count
        pieces.append((start, count, filled == cap))
        start += count
        filled %= cap
    return pieces


class PackBuffers:
    """`cap` records in the extractors' layout on `device`: the seven buffers `ops.gmw_pack_records` writes and `refine_packed`
    reads, and the model's pair tables as the kernel takes them.  `who` names the caller in the refusals, which come before
    anything is allocated."""

    def __init__(self, model, device, cap, nk, who):
        if nk != NUM_KPTS or int(model.num_kpts) != NUM_KPTS:
            raise ValueError("%s: %d key points (model: %d); GMW's pair tables are for %d" % (who, nk, int(model.num_kpts), NUM_KPTS))
        if cap < 1:
            raise ValueError("%s: %d records per refinement call" % (who, cap))
        if next(model.parameters()).dtype != torch.float32:
            raise ValueError("%s runs in float32 (the model is %s)" % (who, next(model.parameters()).dtype))
        self.model, self.cap = model, int(cap)
        P = nk * (nk - 1) // 2
        self.pair_i = model.pair_i.to(device=device, dtype=torch.int32).contiguous()
        self.pair_j = model.pair_j.to(device=device, dtype=torch.int32).contiguous()
        shapes = ((4, P), (6, P), (nk, 2), (nk, 3), (1,), (3,), (3,))        # e4, e6, k2, k3, rot, loc, dim
        self.buffers = [torch.zeros((self.cap,) + s, dtype=torch.float32, device=device) for s in shapes]

    def pack(self, rows, k2, k3, src, dst0):
        """Records `src` (int32 row numbers on the device) of a decoded batch into the buffers from row `dst0` on: one launch."""
        from dcd_amd import ops
        ops.gmw_pack_records(rows, k2, k3, src, dst0, self.pair_i, self.pair_j, *self.buffers)

    def refine(self, count):
        """`refine_packed` of the first `count` records: (pred_depth (count), pred_location (count, 3)) on the device."""
        return refine_packed(self.model, *(b[:count] for b in self.buffers))


class RecordRefiner:
    """GMW's refinement fed by a detector's batched decode, without leaving the device: `add` gathers the named candidates of a
    decoded image batch into `batch_size` accumulation buffers in the extractors' layout (one `ops.gmw_pack_records` launch per
    piece), and every time the buffers fill they are refined (`refine_packed`) and (z, location) is copied asynchronously into
    one of two pinned slots with an event.  The records are refined in the groups [0, bs), [bs, 2 bs), ... of the order they
    were added in -- the partition `refine(data, batch_size=bs)` makes over the same records, so the two give the same bits.
    The host never waits for a flush it has just issued: a flush first collects the one before it (one `Event.synchronize` per
    flush, one flush late) and `finish` collects the last.  The row numbers of an `add` go up through two pinned slots, each
    guarded by the event of the copy that last read it (waited on only if that copy, two calls back, has not finished).
    Everything is enqueued on the stream current at the call."""

    def __init__(self, model, device, batch_size=256, nk=NUM_KPTS):
        self.model, self.device, self.nk = model, torch.device(device), nk
        self.packs = PackBuffers(model, self.device, batch_size, nk, "RecordRefiner")
        self.cap = self.packs.cap
        self.filled = 0
        self.flushes = 0
        self._out = [torch.empty((self.cap, 4), dtype=torch.float32).pin_memory() for _ in range(2)]      # z | location
        self._out_events = [torch.cuda.Event() for _ in range(2)]
        self._waiting = None                                   # (slot, count) of the flush that has not been collected
        self._index = [None, None]
        self._index_events = [None, None]
        self._adds = 0
        self._done = []                                        # (count, 4) host arrays, in order
        self.host_rows, self.host_ids = [], []                 # the caller's notes for the writer: the added records' host rows
                                                               # (n, 14) per image and each record's image id

    def _upload(self, src_host):
        slot = self._adds % 2
        self._adds += 1
        n = len(src_host)
        ev = self._index_events[slot]
        if ev is not None and not ev.query():
            ev.synchronize()                                   # the copy that last read this slot has finished
        if self._index[slot] is None or self._index[slot].numel() < n:
            self._index[slot] = torch.empty(max(n, 1024), dtype=torch.int32).pin_memory()
        self._index[slot].numpy()[:n] = src_host
        src = self._index[slot][:n].to(self.device, non_blocking=True)
        self._index_events[slot] = torch.cuda.Event()
        self._index_events[slot].record()
        return src

    def _collect(self):
        if self._waiting is not None:
            slot, count = self._waiting
            self._out_events[slot].synchronize()
            self._done.append(self._out[slot].numpy()[:count].copy())
            self._waiting = None

    def _flush(self):
        count, slot = self.filled, self.flushes % 2
        z, ploc = self.packs.refine(count)
        self._collect()                                        # the flush before this one: its slot is the other one
        self._out[slot][:count].copy_(torch.cat((z.unsqueeze(1), ploc), dim=1), non_blocking=True)
        self._out_events[slot].record()
        self._waiting = (slot, count)
        self.flushes += 1
        self.filled = 0

    def add(self, rows, k2, k3, src_host):
        """rows (n_rows, 14), k2 (n_rows, nk, 2), k3 (n_rows, nk, 3): a decoded batch on the device; src_host: the row numbers to
        keep, in order (a sequence of ints on the host)."""
        src_host = np.asarray(src_host, dtype=np.int32).reshape(-1)
        if k2.shape[1] != self.nk:
            raise ValueError("RecordRefiner.add: %d key points per record, %d expected" % (k2.shape[1], self.nk))
        if len(src_host) == 0:
            return
        src = self._upload(src_host)
        for start, count, flush in plan_packs(len(src_host), self.filled, self.cap):
            self.packs.pack(rows, k2, k3, src[start:start + count], self.filled)
            self.filled += count
            if flush:
                self._flush()

    def finish(self):
        """Flush what is left; returns pred_location (N, 3) float32 on the host (a tensor), in the order the records were added.
        `pred_depth` (N) is kept as `self.pred_depth`."""
        if self.filled:
            self._flush()
        self._collect()
        out = np.concatenate(self._done, 0) if self._done else np.zeros((0, 4), np.float32)
        self._done = []
        self.pred_depth = torch.from_numpy(out[:, 0].copy())
        return torch.from_numpy(out[:, 1:].copy())


def writer_fields(rows, img_ids):
    """What `write_results` reads beside the refined locations, from the detector's float32 rows (N, 14) on the host and each
    row's image id: `img_idx`, and `box`, `score`, `dim_out`, `rot_out` in float64.  A float32 survives `gen_data_infer.json`
    exactly, so these are the values `load_infer_data` gives for the same records."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 14).astype(np.float64)
    seen, idx = {}, []
    for img in img_ids:
        idx.append((img, seen.get(img, 0)))
        seen[img] = idx[-1][1] + 1
    if len(idx) != len(rows):
        raise ValueError("writer_fields: %d rows, %d image ids" % (len(rows), len(idx)))
    return {"img_idx": idx, "box": rows[:, 2:6].copy(), "score": rows[:, 13].copy(), "dim_out": rows[:, 6:9].copy(),
            "rot_out": rows[:, 12].copy()}


def refine(model, data, device, batch_size=256, fused=True, compute_z=None):
    """`validate`'s refinement over all N records of `data` (load_infer_data) -> (pred_depth (N), pred_location (N, 3)) on the
    host, in the model's dtype.  `compute_z` defaults to the HIP solver kernel; the last, shorter batch goes through as it is."""
    device = torch.device(device)
    dtype = next(model.parameters()).dtype
    if compute_z is None:
        from dcd_amd import ops
        compute_z = ops.compute_z
    if fused and dtype != torch.float32:
        raise ValueError("refine(fused=True) runs in float32 (the model is %s); use fused=False" % dtype)
    n = len(data["img_idx"])
    depths, locations = [], []
    with torch.no_grad():
        for s in range(0, n, batch_size):
            k2, k3, rot, loc, dim = (torch.from_numpy(data[k][s:s + batch_size]).to(device=device, dtype=dtype)
                                     for k in ("kpts_2d", "kpts_3d", "pred_rot", "pred_location", "dim"))
            e4, e6 = model.edge_expand(k2), model.edge_expand(k3)
            if fused:
                z, ploc = refine_packed(model, e4.transpose(-2, -1).contiguous(), e6.transpose(-2, -1).contiguous(), k2, k3, rot,
                                        loc, dim, compute_z)
            else:
                pre_depths, good_idx = compute_z(k2, k3, rot)
                _, z = compute_reg_loss(pre_depths, _stock_weights(model, e4, e6), loc[:, -1], good_idx)
                ploc = relocate(loc, dim, z)
            depths.append(z.cpu())
            locations.append(ploc.cpu())
    if not depths:
        return torch.zeros(0, dtype=dtype), torch.zeros((0, 3), dtype=dtype)
    return torch.cat(depths, 0), torch.cat(locations, 0)


def _wrap_yaw(ori):
    """`write_detection_results`' wrapping (main.py:158-169) as it stands: a yaw below -pi becomes 3 pi."""
    pi = np.pi
    if ori > 2 * pi:
        while ori > 2 * pi:
            ori -= 2 * pi
    if ori < -2 * pi:
        while ori < -2 * pi:
            ori += 2 * pi
    if ori > pi:
        ori = 2 * pi - ori
    if ori < -pi:
        ori = 2 * pi + pi
    return ori


def write_results(data, pred_location, result_dir, image_ids):
    """The result files of `GMW_data` (main.py:123-205): one empty file per id of the split, then one line per record, appended
    in record order, with the refined location in place of the detector's.  Returns result_dir."""
    os.makedirs(result_dir, exist_ok=True)
    for img in image_ids:
        open(os.path.join(result_dir, img + ".txt"), "w").close()
    pos = pred_location.detach().cpu().numpy() if hasattr(pred_location, "detach") else np.asarray(pred_location)
    pos = pos.tolist()
    lines = {}
    for i, (img, _) in enumerate(data["img_idx"]):
        img_id = "{:06d}".format(int(img))
        px, py, pz = pos[i]
        h, w, l = data["dim_out"][i].tolist()
        box = data["box"][i].tolist()
        ori = _wrap_yaw(float(data["rot_out"][i]))
        alpha = ori - math.atan2(px, pz)
        s = "Car " + "%.2f %.d " % (-1, -1)
        s += "%.7f %.7f %.7f %.7f %.7f " % (alpha, box[0], box[1], box[2], box[3])
        s += "%.7f %.7f %.7f %.7f %.7f %.7f %.7f %.7f \n" % (h, w, l, px, py, pz, ori, float(data["score"][i]))
        lines.setdefault(img_id, []).append(s)
    for img_id, rows in lines.items():
        with open(os.path.join(result_dir, img_id + ".txt"), "a") as f:
            f.write("".join(rows))
    return result_dir


def evaluate(model, data, kitti_root, split_file=None, out_dir=".", device="cuda:0", batch_size=256, metric="R40", fused=True,
             compute_z=None):
    """`validate` + `GMW_data.eval_all_results`: refine every record, write `<out_dir>/kitti_results_for_eval`, and score it
    against `<kitti_root>/training/label_2` over the ids of `split_file` (default `<kitti_root>/training/ImageSets/val.txt`).
    Returns (text, dict, moderate 3-D AP at the strict overlap -- the number the reference keeps its best checkpoint by)."""
    from dcd_amd.eval import kitti_annos, kitti_ap
    if split_file is None:
        split_file = os.path.join(kitti_root, "training", "ImageSets", "val.txt")
    _, pred_location = refine(model, data, device, batch_size=batch_size, fused=fused, compute_z=compute_z)
    result_dir = write_results(data, pred_location, os.path.join(out_dir, "kitti_results_for_eval"),
                               kitti_annos.read_imageset(split_file))
    text, result = kitti_ap.evaluate(os.path.join(kitti_root, "training", "label_2"), result_dir, split_file, 0, metric,
                                     device=device)
    return text, result, float(text.split("\n")[3].split(",")[1])
