"""`dcd_gmw_train_records` (csrc/records.hip) on the device against the host build of the same header (tests/host/host_records.cpp),
the reference's fixture and the collection pass it replaces: `do_train(TEST.GENERATE_GMW)` -> `gen_data_train.json` ->
`load_train_data`.  96 x 320 inputs (a 24 x 80 map), B = 2, M = 40 for the kernel tests; the fixture directory for the pass."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import records_refs as R  # noqa: E402
import test_input_host as IH  # noqa: E402
from test_host_golden import load  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS5 = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "pred_location")
MARGIN = 4          # the project's margin for a reordered fp32 sum


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("host_records"))


@pytest.fixture(scope="module")
def E(cuda):
    """Per key: the distance of the op-by-op GPU path (`Loss_Computation` under TEST.GENERATE_GMW on the device, what
    `check_gen_data` runs) from the reference's fixture.  The kernel may differ from the host build of its own header by
    MARGIN times that: both evaluate the same expressions, apart from sin / cos / atan2 / exp of the device and the order of the
    1 500-term mean."""
    import golden_inputs as gi
    from dcd_amd.model.head.detector_loss import Loss_Computation
    g = load("gen_data")
    preds, targets = gi.loss_inputs()
    lc = Loss_Computation(R.small_cfg(cuda, "TEST.GENERATE_GMW", True))
    with torch.no_grad():
        lc({"cls": torch.from_numpy(preds["cls"]).to(cuda), "reg": torch.from_numpy(preds["reg"]).to(cuda)}, [t.to(cuda) for t in targets])
    out = {k: float(np.abs(np.array(lc.gen_data[k][0], np.float32) - g[k]).max()) for k in KEYS5}
    print("E (op-by-op GPU path against gen_data.npz): %s" % {k: "%.3e" % v for k, v in out.items()})
    return out


def both_entries(host_lib):
    from dcd_amd.gmw import collect
    host, real = R.host_entry(host_lib), collect._entry
    return lambda device: host(device) if torch.device(device).type == "cpu" else real(device)


def compare(got, want, n, E, what):
    """Counts, order and `image` equal, kpts_3d bit-equal, the other keys within MARGIN * E."""
    assert got["cursor"].tolist() == want["cursor"].tolist() and got["per_call"].tolist() == want["per_call"].tolist(), what
    assert got["image"].tolist() == want["image"].tolist(), what
    assert R.bit_equal(got["kpts_3d"], want["kpts_3d"]), what
    for k in KEYS5:
        err = float(np.abs(got[k][:n] - want[k][:n]).max()) if n else 0.0
        print("%s %s: kernel - host build %.3e, bar %.3e" % (what, k, err, MARGIN * E[k]))
        assert err <= MARGIN * E[k], (what, k, err, MARGIN * E[k])
        assert R.bit_equal(got[k][n:], want[k][n:]), (what, k)          # the untouched rows: the same poison


def test_kernel_against_the_host_build_on_the_fixture(cuda, host_lib, E, monkeypatch):
    from dcd_amd.gmw import collect
    monkeypatch.setattr(collect, "_entry", both_entries(host_lib))
    g = load("gen_data")
    _, pois, targets = R.fixture_batch()
    cols = {}
    for dev in ("cpu", cuda):
        col = collect.TrainRecordCollector(R.small_cfg(dev), dev, capacity=80, max_calls=1)
        col.add(pois.to(dev), [t.to(dev) for t in targets], torch.arange(2, dtype=torch.int32, device=dev))
        cols[str(torch.device(dev).type)] = col
    dev_col, host_col = cols["cuda"], cols["cpu"]
    n = len(dev_col)
    assert n == len(host_col) == g["kpts_2d"].shape[0]
    assert dev_col.images().cpu().tolist() == host_col.images().tolist()
    gd = dev_col.gen_data()
    assert list(gd["img_idx"][0]) == list(g["img_idx"])
    for k in KEYS5:
        got, want = dev_col.tables[k][:n].cpu().numpy(), host_col.tables[k][:n].numpy()
        if k == "kpts_3d":
            assert R.bit_equal(got, want)
        err = float(np.abs(got - want).max())
        print("%s: kernel - host build %.3e, bar %.3e" % (k, err, MARGIN * E[k]))
        assert err <= MARGIN * E[k], (k, err)
        ref = g[k]
        assert np.abs(got.reshape(ref.shape) - ref).max() <= 2e-3 * max(np.abs(ref).max(), 1.0), k     # test_gpu_golden.py:128


@pytest.mark.parametrize("case", sorted(R.hand_masks()))
def test_kernel_against_the_host_build_on_hand_made_masks(cuda, host_lib, E, case):
    mask = R.hand_masks()[case]
    B = mask.shape[0]
    batch = dict(R.seeded_batch(B, seed=B), reg_mask=mask)
    rows, n = B * R.M, int(mask.sum())
    out = {}
    for dev, entry in (("cpu", R.host_entry(host_lib)("cpu")), (cuda, R.device_entry(cuda))):
        tab = R.Tables(rows, dev, n_calls=1)
        assert R.raw_call(entry, batch, tab, rows, 0, dev) == 0
        out[torch.device(dev).type] = tab.host()
    assert out["cuda"]["cursor"].tolist() == [0, n]
    compare(out["cuda"], out["cpu"], n, E, case)


def test_two_calls_append_and_overflow_is_counted(cuda, host_lib, E):
    masks = R.hand_masks()
    batch = R.seeded_batch(3, seed=3)
    out = {}
    for dev, entry in (("cpu", R.host_entry(host_lib)("cpu")), (cuda, R.device_entry(cuda))):
        tab = R.Tables(12, dev, n_calls=2)
        assert R.raw_call(entry, dict(batch, reg_mask=masks["empty image in the middle"]), tab, 8, 0, dev) == 0
        assert R.raw_call(entry, dict(batch, reg_mask=masks["image 0 empty"]), tab, 8, 1, dev) == 0
        out[torch.device(dev).type] = tab.host()
    got = out["cuda"]
    assert got["per_call"].tolist() == [6, 4] and got["cursor"].tolist() == [10, 6]     # 10 records produced, 8 rows written
    assert all((got[k][8:] == R.POISON).all() for k in KEYS5) and (got["image"][8:] == -1).all()
    compare(got, out["cpu"], 8, E, "two calls, cap 8")


def test_two_calls_on_the_same_inputs_give_the_same_bits(cuda):
    mask = R.hand_masks()["all 40 slots of one image"]
    batch = dict(R.seeded_batch(2, seed=2), reg_mask=mask)
    entry = R.device_entry(cuda)
    runs = []
    for _ in range(2):
        tab = R.Tables(2 * R.M, cuda, n_calls=1)
        assert R.raw_call(entry, batch, tab, 2 * R.M, 0, cuda) == 0
        runs.append(tab.host())
    for k in KEYS5 + ("image", "cursor", "per_call"):
        assert R.bit_equal(runs[0][k], runs[1][k]), k


def test_guarded_buffers_with_overflow_and_an_inf_row(cuda):
    """Tables and workspace between poisoned guards (tests/arena.py), cap = 30 of 42 records, the head outputs of one object all
    inf: the guards and the rows >= cap keep their poison, every row < cap is written, only that object's record is non-finite.
    Valid pointers only."""
    from arena import Arena
    from dcd_amd import _lib
    sizer, fn = R.device_entry(cuda)
    mask = R.hand_masks()["all 40 slots of one image"]
    batch = dict(R.seeded_batch(2, seed=2), reg_mask=mask)
    batch["reg_pois"] = batch["reg_pois"].clone()
    batch["reg_pois"][0, 9] = float("inf")                              # slot (0, 9): the second record
    cap, rows, n = 30, 48, 42
    ar = Arena(cuda)
    ins = {k: ar.place(batch[k], k) for k in ("reg_pois",) + R.FIELDS if k != "reg_mask"}
    ins["reg_mask"] = mask.to(cuda)
    tails = {"kpts_2d": (R.NK, 2), "kpts_3d": (R.NK, 3), "pred_rot": (1,), "gt_location": (3,), "pred_location": (3,)}
    outs = {}
    for k in KEYS5:
        written = torch.zeros((rows,) + tails[k], dtype=torch.bool)
        written[:cap] = True
        outs[k] = ar.out((rows,) + tails[k], k, written=written)
    wi = torch.zeros(rows, dtype=torch.bool)
    wi[:cap] = True
    image = ar.out((rows,), "image", dtype=torch.int32, written=wi)
    cursor = ar.place(torch.zeros(2, dtype=torch.int32), "cursor", inplace=True)
    per_call = ar.out((1,), "per_call", dtype=torch.int32)
    a = R.default_args(2)
    nbytes = int(sizer(2, R.M, R.NK))
    assert nbytes == 4 * 2 * R.M * (R.NK * 5 + 13 + 2 * 1500)
    ws = ar.scratch(nbytes, "workspace")
    st = fn(_lib.stream_of(ins["reg_pois"]), ins["reg_pois"].data_ptr(), ctypes.byref(a), *[ins[k].data_ptr() for k in R.FIELDS], cap,
            *[outs[k].data_ptr() for k in KEYS5], image.data_ptr(), cursor.data_ptr(), per_call.data_ptr(), 0, 1, Arena.ptr(ws), nbytes)
    assert st == 0
    ar.check("dcd_gmw_train_records")
    assert cursor.cpu().tolist() == [0, n] and per_call.cpu().tolist() == [n]
    for k in KEYS5:
        body = outs[k][:cap].cpu().reshape(cap, -1)
        finite = torch.isfinite(body).all(dim=1)
        assert finite[0] and finite[2:].all(), k
        # gt_location is a function of the targets only; the yaw of an all-inf object is finite (atan2(inf, inf) = pi / 4, and the
        # solver's clamp turns its NaN depths into 2: the viewing ray is atan2(inf, 2))
        if k in ("kpts_2d", "kpts_3d", "pred_location"):
            assert not finite[1], k
    assert torch.isfinite(outs["gt_location"][1]).all()


def test_argument_errors_are_return_codes(cuda):
    batch = R.seeded_batch(2, seed=2)
    entry = R.device_entry(cuda)
    tab = R.Tables(8, cuda, n_calls=1)
    big = torch.empty(1 << 22, dtype=torch.uint8, device=cuda)
    bad = []
    for field, value in (("nk", 1), ("nk", 129), ("n_bins", 0), ("n_bins", 5), ("ch_kpts3d", R.C - 3 * R.NK + 1), ("ch_kpts2d", -2),
                         ("ch_offset", R.C - 1), ("B", 0), ("M", 0)):
        a = R.default_args(2)
        setattr(a, field, value)
        bad.append(R.raw_call(entry, batch, tab, 8, 0, cuda, args=a, workspace=big))
    bad.append(R.raw_call(entry, batch, tab, 0, 0, cuda))               # cap < 1
    bad.append(R.raw_call(entry, batch, tab, 8, 1, cuda))               # call outside [0, n_calls)
    bad.append(R.raw_call(entry, batch, tab, 8, -1, cuda))
    # a null pointer in every pointer position
    sizer, fn = entry
    a = R.default_args(2)
    on = {k: v.to(cuda) for k, v in batch.items()}
    ptrs = [on["reg_pois"].data_ptr()] + [on[k].data_ptr() for k in R.FIELDS]
    for i in range(len(ptrs)):
        p = list(ptrs)
        p[i] = None
        bad.append(fn(None, p[0], ctypes.byref(a), *p[1:], 8, *tab.pointers(), 0, 1, big.data_ptr(), big.numel()))
    for i in range(8):
        q = tab.pointers()
        q[i] = None
        bad.append(fn(None, ptrs[0], ctypes.byref(a), *ptrs[1:], 8, *q, 0, 1, big.data_ptr(), big.numel()))
    bad.append(fn(None, ptrs[0], None, *ptrs[1:], 8, *tab.pointers(), 0, 1, big.data_ptr(), big.numel()))
    bad.append(fn(None, ptrs[0], ctypes.byref(a), *ptrs[1:], 8, *tab.pointers(), 0, 1, None, big.numel()))
    assert bad == [1] * len(bad)
    assert R.raw_call(entry, batch, tab, 8, 0, cuda, workspace=torch.empty(64, dtype=torch.uint8, device=cuda)) == 2
    assert sizer(0, 40, 73) == 0 and sizer(2, 40, 129) == 0
    got = tab.host()                                                    # nothing was launched
    assert all((got[k] == R.POISON).all() for k in KEYS5) and got["per_call"].tolist() == [-1] and got["cursor"].tolist() == [0, 0]


# ---- the pass --------------------------------------------------------------------------------------------------------------
ITERATIONS = 3


class _Replay:
    """Forward hook on the predictor.  The detector's forward is not bit-reproducible from one run to the next (a channel that is
    only copied differed by 1.5e-8 between two passes over the same batches), so a comparison of two routes at the arithmetic's
    own bar needs both to see the same head outputs: while `log` is recording the hook keeps every call's (predictions, targets);
    while replaying, the backbone and the predictor still run, and the hook hands on the recorded predictions of that call."""

    def __init__(self):
        self.log, self.replay_at = [], None

    def __call__(self, module, inputs, output):
        if self.replay_at is None:
            self.log.append(({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in output.items()}, inputs[1]))
            return None
        preds = self.log[self.replay_at][0]
        self.replay_at += 1
        return dict(preds)


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """The fixture directory (three training images with objects), the real detector with `name_hashed_init`, batches of 2, and
    the parent route's file: `do_train` under TEST.GENERATE_GMW with the keyword off, its predictor's outputs recorded."""
    import golden_inputs as gi
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    base = tmp_path_factory.mktemp("gmw_collect")
    root, _ = IH.write_kitti_dir(base, [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    # IMS_PER_BATCH 1 only sets the length of the pass: len(batches) // 1 = 3 iterations, each a batch of 2
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.GENERATE_GMW", True, "SOLVER.IMS_PER_BATCH", 1])
    files = KittiFiles(root, cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    assert len(files) == ITERATIONS
    split = ResidentSplit(files, cfg, cuda, workers=2)
    model = KeypointDetector(cfg).to(cuda)
    gi.name_hashed_init(model)
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    out = str(base / "parent")
    replay = _Replay()
    handle = model.heads.predictor.register_forward_hook(replay)
    try:
        args = do_train(cfg, model, optimizer, scheduler, warmup, ResidentBatches(split, 2, seed=0), {"iteration": 0}, out)
    finally:
        handle.remove()
    assert args["iteration"] == ITERATIONS and "gmw_records" not in args and len(replay.log) == ITERATIONS
    path = os.path.join(out, "gen_data", "gen_data_train.json")
    return dict(cfg=cfg, files=files, split=split, model=model, optimizer=optimizer, schedulers=(scheduler, warmup), base=base,
                json_path=path, batches=lambda: ResidentBatches(split, 2, seed=0), replay=replay)


def test_default_is_unchanged(cuda, world):
    """With the keyword off `do_train` writes what a run through `Loss_Computation` directly gives on the predictions and targets
    its own pass handed to the loss."""
    from dcd_amd.model.head.detector_loss import Loss_Computation
    lc = Loss_Computation(world["cfg"])
    with torch.no_grad():
        for preds, targets in world["replay"].log:
            lc(dict(preds), targets)
    assert json.load(open(world["json_path"])) == json.loads(json.dumps(lc.gen_data))


def test_collection_pass_equals_the_file_route(cuda, world, E):
    from dcd_amd.engine.train import collect_gmw_records
    from dcd_amd.gmw import GMW
    from dcd_amd.gmw.data import KEYS, ResidentRecords, load_train_data
    from dcd_amd.gmw.train import build_gmw_optimizer, train_iteration
    want = load_train_data(world["json_path"])
    parent = json.load(open(world["json_path"]))
    model, replay = world["model"], world["replay"]
    # 1. the pass as it is, its own forward on both sides: the records' number and order, values at the bar the op-by-op GPU path
    #    is held to against the reference (test_gpu_golden.py:128)
    free = collect_gmw_records(model, world["batches"](), ITERATIONS)
    assert isinstance(free, ResidentRecords) and len(free) == want["kpts_2d"].shape[0] > 0
    for t, k in zip(free.tables, KEYS):
        got = t.cpu().numpy()
        assert got.shape == want[k].shape and np.abs(got - want[k]).max() <= 2e-3 * max(np.abs(want[k]).max(), 1.0), k
    # 2. on the head outputs the file route saw: the kernel tests' bar per key
    replay.replay_at = 0
    handle = model.heads.predictor.register_forward_hook(replay)
    try:
        records = collect_gmw_records(model, world["batches"](), ITERATIONS)
    finally:
        handle.remove()
        replay.replay_at = None
    assert isinstance(records, ResidentRecords) and len(records) == want["kpts_2d"].shape[0]
    assert all(t.is_cuda for t in records.tables)
    for t, k in zip(records.tables, KEYS):
        got = t.cpu().numpy()
        err = float(np.abs(got - want[k]).max())
        print("%s: pass - file route %.3e, bar %.3e" % (k, err, MARGIN * E[k]))
        assert got.shape == want[k].shape and err <= MARGIN * E[k], (k, err)
    gd = records.collector.gen_data()
    assert gd["img_idx"] == parent["img_idx"] and [len(x) for x in gd["pred_rot"]] == [len(x) for x in parent["pred_rot"]]
    pl = np.array([r for it in gd["pred_location"] for r in it], np.float32)
    ref = np.array([r for it in parent["pred_location"] for r in it], np.float32)
    # pred_location is not one of the four tables GMW trains on; it is held to the same margin, with E taken RELATIVE to the
    # fixture's largest coordinate: the error of the reordered 1 500-term mean is relative to the depth, and this detector's
    # untrained heads put objects at up to 80 m where the fixture's lie within 37 m
    scale = max(1.0, float(np.abs(ref).max()) / float(np.abs(load("gen_data")["pred_location"]).max()))
    err = float(np.abs(pl - ref).max())
    print("pred_location: pass - file route %.3e, bar %.3e (largest coordinate %.1f)" % (err, MARGIN * E["pred_location"] * scale,
                                                                                       np.abs(ref).max()))
    assert err <= MARGIN * E["pred_location"] * scale
    # the default capacity: the labelled objects of the images the pass saw
    assert records.collector.capacity >= len(records)
    # one iteration of GMW's training on the resident records
    torch.manual_seed(0)
    gmw = GMW(device_sinkhorn=True).to(cuda)
    values = train_iteration(gmw, build_gmw_optimizer(gmw), records.batch([0, len(records) - 1]), 0.1, 1.0)
    assert values.shape == (4,) and bool(torch.isfinite(values).all())


def test_loop_body_has_no_host_synchronisation(cuda, world):
    from dcd_amd.engine.train import collect_step, freeze_bn
    from dcd_amd.gmw.collect import TrainRecordCollector
    model, batches = world["model"], world["batches"]()
    col = TrainRecordCollector(world["cfg"], cuda, capacity=3 * 2 * 40, max_calls=3)
    numbers = torch.tensor([[0, 1], [2, 0], [1, 2]], dtype=torch.int32).to(cuda)
    model.train()
    freeze_bn(model)
    got = [batches.get(k) for k in range(3)]
    with torch.no_grad():
        for k in range(2):                                              # warm-up: both pinned slots, the workspace
            collect_step(model, col, got[k][0], got[k][1], numbers[k])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            collect_step(model, col, got[2][0], got[2][1], numbers[2])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert len(col) > 0 and col.calls == 3


def test_do_train_with_the_keyword(cuda, world, tmp_path):
    from dcd_amd.engine.train import do_train
    from dcd_amd.gmw.data import ResidentRecords, load_train_data
    scheduler, warmup = world["schedulers"]
    out = str(tmp_path / "records")
    args = do_train(world["cfg"], world["model"], world["optimizer"], scheduler, warmup, world["batches"](), {"iteration": 0}, out,
                    gmw_records=True)
    assert isinstance(args["gmw_records"], ResidentRecords) and args["iteration"] == ITERATIONS
    assert not os.path.exists(os.path.join(out, "gen_data", "gen_data_train.json"))
    out = str(tmp_path / "json")
    args = do_train(world["cfg"], world["model"], world["optimizer"], scheduler, warmup, world["batches"](), {"iteration": 0}, out,
                    gmw_records="json")
    back = load_train_data(os.path.join(out, "gen_data", "gen_data_train.json"))
    for t, k in zip(args["gmw_records"].tables, ("kpts_2d", "kpts_3d", "pred_rot", "gt_location")):
        assert R.bit_equal(back[k], t.cpu().numpy()), k
    cfg = world["cfg"].clone()
    cfg.merge_from_list(["MODEL.HEAD.CORNER_LOSS_DEPTH", "direct"])
    with pytest.raises(NotImplementedError, match="CORNER_LOSS_DEPTH"):
        do_train(cfg, world["model"], world["optimizer"], scheduler, warmup, world["batches"](), {"iteration": 0}, out, gmw_records=True)


def test_records_from_a_detector_checkpoint(cuda, world, tmp_path):
    """The one-command route of `python -m dcd_amd.gmw.train --detector-ckpt`: checkpoint -> collection pass -> resident records."""
    from dcd_amd.engine.train import save_checkpoint
    from dcd_amd.gmw.data import ResidentRecords
    from dcd_amd.gmw.train import build_parser, records_from_detector
    scheduler, _ = world["schedulers"]
    ckpt = save_checkpoint(str(tmp_path), "model_final", world["model"], world["optimizer"], scheduler, {"iteration": 0})
    args = build_parser().parse_args(["--detector-ckpt", ckpt, "--root", world["files"].root, "--detector-batch", "2",
                                      "--detector-opts", "MODEL.USE_SYNC_BN", "False"])
    records = records_from_detector(args.detector_ckpt, args.root, args.split, args.detector_batch, args.detector_opts)
    assert isinstance(records, ResidentRecords) and records.collector.calls == 1 and len(records) > 0
    assert records.collector.images().cpu().unique().tolist() == [0, 1]           # file order, no shuffle, whole batches only
    assert bool(torch.isfinite(records.tables[3]).all())
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--detector-ckpt", ckpt, "--train_data_path", "x.json"])
    with pytest.raises(SystemExit):
        build_parser().parse_args([])
