"""Shared pieces of the tests of `dcd_gmw_train_records` (csrc/records.hip): the host build of csrc/records_math.h
(tests/host/host_records.cpp) behind the entry point's own signature, a raw call on tensors of either device, seeded target
tables and the hand-made masks of the compaction rules.  TEST INFRASTRUCTURE."""
import ctypes
import os
import subprocess

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "pred_location")
NK, C, M = 73, 415, 40
POISON = float.fromhex("0x1.8p+100")          # a finite value no record can hold


def build_host(tmp_dir):
    from dcd_amd import _lib
    out = os.path.join(str(tmp_dir), "libhost_records.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_records.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    for host, ours in (("host_gmw_train_records_workspace_bytes", "dcd_gmw_train_records_workspace_bytes"),
                       ("host_gmw_train_records", "dcd_gmw_train_records")):
        fn = getattr(lib, host)
        fn.restype, fn.argtypes = _lib.SIGNATURES[ours]
    return lib


def host_entry(lib):
    """What `dcd_amd.gmw.collect._entry` returns, from the host build."""
    return lambda device: (lib.host_gmw_train_records_workspace_bytes, lib.host_gmw_train_records)


def device_entry(device):
    from dcd_amd.gmw import collect
    return collect._entry(device)


def default_args(B, m=M, c=C, nk=NK):
    """`dcd_records_args` of the default configuration: the channel starts `records_spec` reads from DGDE.yaml's channel map."""
    from dcd_amd.config import get_cfg
    from dcd_amd.gmw.collect import TrainRecordCollector, records_spec
    spec = records_spec(get_cfg(opts=["MODEL.PRETRAIN", False]))
    assert spec["nk"] == NK and spec["C"] == C and spec["M"] == M
    holder = TrainRecordCollector.__new__(TrainRecordCollector)
    holder.spec = dict(spec, nk=nk)
    return holder.args(B, m, c)


def seeded_batch(B, seed, m=M):
    """Target tables and head outputs of a batch with EVERY slot usable: what `encode_packed` would hand over for B images with
    m objects each, with values in KITTI's ranges.  Returns a dict of CPU tensors in the entry point's dtypes."""
    rng = np.random.RandomState(seed)
    P = np.zeros((B, m, 3, 4), np.float32)
    calib = np.zeros((B, 6), np.float32)
    for b in range(B):
        f, cu, cv = 707.0 + 7.0 * b, 604.0 + 3.0 * b, 180.0 - 4.0 * b
        Pb = np.array([[f, 0, cu, 45.0 - b], [0, f, cv, -0.3 + 0.1 * b], [0, 0, 1, 0.004 + 0.001 * b]], np.float64)
        P[b, :] = Pb.astype(np.float32)
        calib[b] = [Pb[0, 2], Pb[1, 2], Pb[0, 0], Pb[1, 1], Pb[0, 3] / -Pb[0, 0], Pb[1, 3] / -Pb[1, 1]]
    centers = np.stack((rng.randint(0, 80, (B, m)), rng.randint(0, 24, (B, m))), axis=-1).astype(np.int32)
    loc = np.concatenate((rng.uniform(-20, 20, (B, m, 2)), rng.uniform(5, 60, (B, m, 1))), axis=-1).astype(np.float32)
    t = torch.from_numpy
    return {"reg_pois": t((rng.normal(size=(B, m, C)) * 0.5).astype(np.float32)),
            "reg_mask": torch.ones((B, m), dtype=torch.uint8),
            "target_centers": t(centers), "offset_3D": t(rng.uniform(0, 1, (B, m, 2)).astype(np.float32)),
            "rotys": t(rng.uniform(-np.pi, np.pi, (B, m)).astype(np.float32)), "locations": t(loc), "Calib_P": t(P),
            "pad_size": t(np.stack((rng.randint(0, 3, B), rng.randint(0, 9, B)), axis=-1).astype(np.int64)),
            "calib": t(calib), "image_numbers": t((100 + 7 * np.arange(B)).astype(np.int32))}


FIELDS = ("reg_mask", "target_centers", "offset_3D", "rotys", "locations", "Calib_P", "pad_size", "calib", "image_numbers")


class Tables:
    """Six tables of `rows` rows filled with POISON (image: -1), a zeroed cursor pair and per-call counts, on `device`."""

    def __init__(self, rows, device, n_calls=2, nk=NK, make=None):
        tails = {"kpts_2d": (nk, 2), "kpts_3d": (nk, 3), "pred_rot": (1,), "gt_location": (3,), "pred_location": (3,)}
        self.rows, self.n_calls = rows, n_calls
        self.t = {k: torch.full((rows,) + tails[k], POISON, dtype=torch.float32, device=device) for k in TABLES}
        self.image = torch.full((rows,), -1, dtype=torch.int32, device=device)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=device)
        self.per_call = torch.full((n_calls,), -1, dtype=torch.int32, device=device)

    def pointers(self):
        return [self.t[k].data_ptr() for k in TABLES] + [self.image.data_ptr(), self.cursor.data_ptr(), self.per_call.data_ptr()]

    def host(self):
        out = {k: v.cpu().numpy() for k, v in self.t.items()}
        out["image"], out["cursor"], out["per_call"] = self.image.cpu().numpy(), self.cursor.cpu().numpy(), self.per_call.cpu().numpy()
        return out


def raw_call(entry, batch, tables, cap, call, device, args=None, workspace=None):
    """One call of the entry point (`entry` = (size query, function)) on `batch` moved to `device`; returns the status."""
    from dcd_amd import _lib
    sizer, fn = entry
    dev = torch.device(device)
    on = {k: v.to(dev).contiguous() for k, v in batch.items()}
    B, m, c = on["reg_pois"].shape
    a = args if args is not None else default_args(B, m, c)
    if workspace is None:
        workspace = torch.empty(max(int(sizer(B, m, a.nk)), 4), dtype=torch.uint8, device=dev)
    stream = _lib.stream_of(on["reg_pois"]) if dev.type == "cuda" else None
    st = fn(stream, on["reg_pois"].data_ptr(), ctypes.byref(a), *[on[k].data_ptr() for k in FIELDS], cap, *tables.pointers(),
            call, tables.n_calls, workspace.data_ptr(), workspace.numel())
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return st


def hand_masks():
    """name -> (B, mask (B, 40) uint8): the compaction rules' cases."""
    def mask(B, rows):
        m = torch.zeros((B, M), dtype=torch.uint8)
        for b, slots in rows.items():
            m[b, slots] = 1
        return m
    return {"empty image in the middle": mask(3, {0: [0, 3, 39], 2: [1, 2, 17]}),
            "image 0 empty": mask(3, {1: [0, 5], 2: [38, 39]}),
            "all 40 slots of one image": mask(2, {0: [4, 9], 1: list(range(M))})}


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def fixture_batch():
    """The pinned loss inputs as a batch of the collector: (reg_pois (2, 40, 415) gathered at the target centres, targets)."""
    import golden_inputs as gi
    from oracle import torch_ops
    from dcd_amd.structures.params_3d import stack_field
    preds, targets = gi.loss_inputs()
    reg = torch.from_numpy(preds["reg"])
    pois = torch_ops.select_point_of_interest(reg.shape[0], stack_field(targets, "target_centers"), reg)
    return preds, pois, targets


def small_cfg(device="cpu", *more):
    from dcd_amd.config import get_cfg
    return get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(device), "MODEL.USE_SYNC_BN", False, "INPUT.WIDTH_TRAIN", 320,
                         "INPUT.HEIGHT_TRAIN", 96] + list(more))
