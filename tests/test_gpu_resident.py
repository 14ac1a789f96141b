"""A training run fed from device memory, on the GPU: `dcd_gather_rows` (csrc/resident.hip) through the C ABI against
`index_select` on byte views; `ResidentSplit` (dcd_amd/data/resident.py) against `DeviceInputPipeline` on the same frames, samples
and flags; the batch sources and the `Prefetcher` of dcd_amd/data/batches.py inside `do_train` (dcd_amd/engine/train.py); and
two real iterations from the fixture directory to a checkpoint that loads.

No tolerance anywhere: both sides run the same kernels on the same bytes, or move bytes."""
import ctypes
import logging
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_input_host as IH  # noqa: E402
from test_gpu_input import noise_frames, tensor_fields  # noqa: E402,F401

# the six tables of a resident batch at M = 40, n_extra = 63: count, size, record, P, objs, kpts3d
ROW_BYTES = (4, 8, 40, 96, 5120, 60480)
SRC_ROWS = (11, 11, 11, 9, 11, 11)          # the (3, 4) table is shorter: row 10 exists in five tables and is outside the sixth
GUARD, FILL = 64, 0xA5


# ---------------------------------------------------------------------------------------------------------- dcd_gather_rows
class Tables:
    """Source tables of seeded bytes and guarded destinations; `shift` = (which, bytes) moves the base of the two large tables'
    sources or destinations off their 16-byte alignment."""

    def __init__(self, cuda, B, shift=(None, 0), row_bytes=ROW_BYTES, src_rows=SRC_ROWS):
        g = torch.Generator().manual_seed(17)
        self.B, self.row_bytes, self.src_rows = B, row_bytes, src_rows
        self.src, self.dst_buf, self.dst = [], [], []
        for t, (rb, rows) in enumerate(zip(row_bytes, src_rows)):
            off = shift[1] if t >= 4 else 0
            s = torch.randint(1, 256, (rows * rb + 16,), dtype=torch.uint8, generator=g).to(cuda)     # no zero bytes: a zero row shows
            self.src.append(s[off:off + rows * rb] if shift[0] == "src" else s[:rows * rb])
            d = torch.full((GUARD + B * rb + 16 + GUARD,), FILL, dtype=torch.uint8, device=cuda)
            self.dst_buf.append(d)
            o = GUARD + (off if shift[0] == "dst" else 0)
            self.dst.append(d[o:o + B * rb])

    def arrays(self, n=None):
        n = len(self.src) if n is None else n
        pick = [i % len(self.src) for i in range(n)]
        return ((ctypes.c_void_p * n)(*[self.src[i].data_ptr() for i in pick]), (ctypes.c_void_p * n)(*[self.dst[i].data_ptr() for i in pick]),
                (ctypes.c_int64 * n)(*[self.row_bytes[i] for i in pick]), (ctypes.c_int64 * n)(*[self.src_rows[i] for i in pick]))

    def expected(self, index):
        out = []
        for s, rb, rows in zip(self.src, self.row_bytes, self.src_rows):
            idx = torch.as_tensor(index, dtype=torch.int64, device=s.device)
            ok = (idx >= 0) & (idx < rows)
            got = s.view(rows, rb).index_select(0, torch.where(ok, idx, torch.zeros_like(idx)))
            out.append(torch.where(ok[:, None], got, torch.zeros_like(got)).reshape(-1))
        return out

    def check(self, index, what):
        for t, (want, d, buf) in enumerate(zip(self.expected(index), self.dst, self.dst_buf)):
            assert torch.equal(d, want), (what, "table", t)
            start = d.data_ptr() - buf.data_ptr()
            outside = torch.cat((buf[:start], buf[start + d.numel():]))
            assert bool((outside == FILL).all()), (what, "guard bytes of table", t)

    def untouched(self):
        return all(bool((b == FILL).all()) for b in self.dst_buf)


def gather(tables, index_dev, arrays=None, n=None, B=None):
    from dcd_amd import _lib
    src, dst, rb, rows = arrays if arrays is not None else tables.arrays()
    return _lib.lib().dcd_gather_rows(_lib.stream_of(index_dev), len(src) if n is None else n, src, dst, rb, rows, index_dev.data_ptr(),
                                      tables.B if B is None else B)


@pytest.mark.parametrize("shift", [(None, 0), ("src", 4), ("dst", 4)], ids=["aligned", "src+4", "dst+4"])
@pytest.mark.parametrize("index", [[10], [-1], [0, 11, 10], [0, 10, 3, 3, -1, 11, 8, 5]], ids=["B1-last", "B1-outside", "B3", "B8"])
def test_gather_rows_equals_index_select(cuda, index, shift):
    """5. Row 0, the last row, a repeat, -1 and `src_rows` (zero rows), row 10 outside the shorter table only; 16-byte and 4-byte
    paths (a base 4 bytes off its alignment); every byte outside the destinations' B rows keeps its fill."""
    tb = Tables(cuda, len(index), shift)
    if shift[0] is not None:
        side = tb.src if shift[0] == "src" else tb.dst
        assert side[5].data_ptr() % 16 == 4 and side[3].data_ptr() % 16 == 0
    assert gather(tb, torch.tensor(index, dtype=torch.int32, device=cuda)) == 0
    tb.check(index, (index, shift))
    if 0 in index:
        assert bool((tb.dst[5][:ROW_BYTES[5]] != 0).all())                  # a real row: the comparison is not of zeros


def test_gather_rows_rejects_bad_arguments(cuda):
    """Status 1 for every bad argument of the header, and nothing written."""
    tb = Tables(cuda, 3)
    index = torch.tensor([0, 1, 2], dtype=torch.int32, device=cuda)
    src, dst, rb, rows = tb.arrays()

    def edited(which, t, value):
        a = list(tb.arrays())
        a[which][t] = value
        return a
    cases = {
        "null src": (None, dst, rb, rows), "null dst": (src, None, rb, rows), "null row_bytes": (src, dst, None, rows),
        "null src_rows": (src, dst, rb, None), "null table": edited(0, 2, None), "null destination": edited(1, 5, None),
        "row_bytes 0": edited(2, 1, 0), "row_bytes 6": edited(2, 1, 6), "row_bytes -4": edited(2, 0, -4),
        "src base 2 off": edited(0, 4, tb.src[4].data_ptr() + 2), "dst base 2 off": edited(1, 4, tb.dst[4].data_ptr() + 2),
    }
    for name, arrays in cases.items():
        assert gather(tb, index, arrays, n=6) == 1, name
    assert gather(tb, index, n=0) == 1 and gather(tb, index, tb.arrays(9), n=9) == 1
    assert gather(tb, index, B=0) == 1 and gather(tb, index, B=-2) == 1
    from dcd_amd import _lib
    assert _lib.lib().dcd_gather_rows(_lib.stream_of(index), 6, src, dst, rb, rows, None, 3) == 1
    torch.cuda.synchronize(cuda)
    assert tb.untouched()
    assert gather(tb, index, tb.arrays(8), n=8) == 0                        # eight tables are allowed
    tb.check([0, 1, 2], "eight tables")


def test_gather_rows_in_a_captured_graph_follows_the_index(cuda):
    """The table descriptors travel in the kernel arguments, only `index` is read from the device: a replay after the index
    tensor's contents changed gathers the new rows."""
    tb = Tables(cuda, 3)
    index = torch.tensor([0, 1, 2], dtype=torch.int32, device=cuda)
    assert gather(tb, index) == 0                                           # the kernel is loaded before anything is captured
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert gather(tb, index) == 0
    for new in ([10, 10, 0], [4, -1, 8]):
        index.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize(cuda)
        tb.check(new, ("replay", new))


# ------------------------------------------------------------------------------------------------------------ ResidentSplit
@pytest.fixture(scope="module")
def kitti(cuda, tmp_path_factory):
    """The committed fixture directory with seeded-noise PNGs at the default 384 x 1280 canvas, read once and made resident."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path_factory.mktemp("resident"), [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False])
    files = KittiFiles(root, cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    assert len(files) == 3
    frames = [files.frame(i) for i in range(3)]
    samples = [files.sample(i) for i in range(3)]
    return dict(cfg=cfg, files=files, frames=frames, samples=samples, split=ResidentSplit(files, cfg, cuda, workers=2))


def assert_same_batch(got, want, what):
    """Every respect in which two `(images, targets)` pairs can differ."""
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape and torch.equal(got[0], want[0]), (what, "images")
    assert len(got[1]) == len(want[1])
    for b, (a, r) in enumerate(zip(got[1], want[1])):
        assert a.fields() == r.fields() and a.size == r.size and a.is_train == r.is_train, (what, b)
        fa, fr = tensor_fields(a), tensor_fields(r)
        assert set(fa) == set(fr) >= {"hm", "reg_mask", "Calib_P", "final_output_w", "final_output_h", "pad_size", "edge_indices"}
        for name in fa:
            assert fa[name].dtype == fr[name].dtype and fa[name].shape == fr[name].shape, (what, b, name)
            np.testing.assert_array_equal(fa[name], fr[name], err_msg="%s image %d field %s" % (what, b, name))
        np.testing.assert_array_equal(a.get_field("calib").P, r.get_field("calib").P)
        assert a.get_field("img_idx") == r.get_field("img_idx")


def snapshot(batch):
    """A batch whose tensors no later call can touch."""
    images, targets = batch
    out = []
    for t in targets:
        c = type(t)(t.size, t.is_train)
        for name in t.fields():
            v = t.get_field(name)
            c.add_field(name, v.clone() if torch.is_tensor(v) else v)
        out.append(c)
    return images.clone(), out


@pytest.mark.parametrize("indices,flags,ids", [
    ([1], [True], None), ([2], [False], ["x"]),
    ([0, 1, 2], [True, False, True], ["a", "b", "c"]), ([0, 1, 2], [False, True, False], None),
    ([1, 1, 0], [True, False, True], ["p", "q", "r"])], ids=["B1-flip", "B1-plain", "B3-101", "B3-010", "B3-repeat"])
def test_resident_batch_equals_the_pipeline(cuda, kitti, indices, flags, ids):
    """6. `ResidentSplit.batch` == `DeviceInputPipeline` on the same frames, samples and flags: images, every tensor field,
    `calib.P`, `img_idx`, the output size, `ParamsList.size`; the images also equal the pinned restatement."""
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    cfg = kitti["cfg"]
    got = kitti["split"].batch(indices, flags, img_ids=ids)
    frames, samples = [kitti["frames"][i] for i in indices], [kitti["samples"][i] for i in indices]
    want = DeviceInputPipeline(cfg, cuda)(frames, samples, ids, flip=flags)
    assert_same_batch(got, want, (indices, flags))
    ref = IH.restate_images(frames, flags, 384, 1280, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR)
    assert torch.equal(got[0].cpu(), ref)
    assert sum(int(t.get_field("reg_mask").sum()) for t in got[1]) >= 1
    if any(flags) and not all(flags):                                        # flipped and plain targets of one image do differ
        i = indices[0]
        a, b = kitti["split"].batch([i], [True])[1][0], kitti["split"].batch([i], [False])[1][0]
        assert not torch.equal(a.get_field("Calib_P"), b.get_field("Calib_P"))


def test_resident_split_limits(cuda, kitti):
    from dcd_amd import _lib
    from dcd_amd.data.resident import ResidentSplit
    split, cfg, files = kitti["split"], kitti["cfg"], kitti["files"]
    assert len(split) == 3 and split.nbytes > sum(f.size for f in kitti["frames"]) and split.frames.numel() % 64 == 0
    torch.cuda.synchronize(cuda)
    before = torch.cuda.memory_allocated(cuda)
    with pytest.raises(_lib.DcdHipError) as e:
        ResidentSplit(files, cfg, cuda, max_bytes=1)
    assert str(split.nbytes) in str(e.value) and " 1 " in str(e.value)
    assert torch.cuda.memory_allocated(cuda) == before                       # refused before anything was allocated
    with pytest.raises(_lib.DcdHipError):
        ResidentSplit(files, cfg, "cpu")
    for bad in ([3], [0, -1]):
        with pytest.raises(IndexError):
            split.batch(bad, [False] * len(bad))
    with pytest.raises(ValueError):
        split.batch([0, 1], [True])
    with pytest.raises(ValueError):                                          # a canvas smaller than the frames, as for the pipeline
        from dcd_amd.config import get_cfg
        ResidentSplit(files, get_cfg(opts=["INPUT.WIDTH_TRAIN", 1200]), cuda)


def test_prefetcher_hands_over_what_a_direct_call_computes(cuda, kitti):
    """Four consecutive batches through `Prefetcher` (computed on its side stream, one ahead) == the same batches computed
    directly; a batch that was not prefetched is simply computed."""
    from dcd_amd.data.batches import Prefetcher, ResidentBatches
    direct = ResidentBatches(kitti["split"], 3, seed=7)
    want = [snapshot(direct.get(k)) for k in range(4)]
    pre = Prefetcher(ResidentBatches(kitti["split"], 3, seed=7), cuda)
    assert pre.batch_size == 3 and len(pre) == 3
    sums = []
    for k in range(4):
        got = pre.get(k)
        assert list(pre._ready) == [k + 1]
        sums.append(got[0].double().sum())                                   # consumed on the current stream
        assert_same_batch(got, want[k], ("prefetched", k))
    assert [float(s) for s in sums] == [float(w[0].double().sum()) for w in want]
    assert_same_batch(pre.get(1), want[1], "not the prefetched one")
    assert not torch.equal(want[0][0], want[1][0]) or not torch.equal(want[1][0], want[2][0])


# -------------------------------------------------------------------------------------------------------------- do_train
def tiny_run(cuda, cfg_opts):
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False] + cfg_opts)
    model = torch.nn.Linear(2, 1).to(cuda)
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    return cfg, model, optimizer, scheduler, warmup


@pytest.mark.parametrize("prefetch", [False, True], ids=["direct", "prefetched"])
@pytest.mark.parametrize("kind", ["resident", "streaming"])
def test_do_train_feeds_the_step_batch_k_at_iteration_k(cuda, kitti, tmp_path, kind, prefetch):
    """7. A recording step inside `do_train`, four iterations at B = 2: what the step received at iteration k == `get(k)` of a
    fresh source, for both sources, with and without the prefetcher; the two sources agree bit for bit."""
    from dcd_amd.data.batches import Prefetcher, ResidentBatches, StreamingBatches
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.engine.train import do_train
    cfg, model, optimizer, scheduler, warmup = tiny_run(cuda, ["SOLVER.MAX_ITERATION", 4, "SOLVER.IMS_PER_BATCH", 2])

    def make(k):
        if k == "resident":
            return ResidentBatches(kitti["split"], 2, seed=11)
        return StreamingBatches(kitti["files"], DeviceInputPipeline(cfg, cuda, is_train=True), 2, seed=11, workers=2)
    fresh = {k: make(k) for k in ("resident", "streaming")}
    want = {k: [snapshot(s.get(i)) for i in range(4)] for k, s in fresh.items()}
    for i in range(4):
        assert_same_batch(want["resident"][i], want["streaming"][i], ("the two sources", i))
    assert len({tuple(t.get_field("img_idx") for t in w[1]) for w in want["resident"]}) > 1
    seen = []
    const = torch.tensor(0.25, device=cuda)

    def step(images, targets):
        seen.append(snapshot((images, targets)))
        return {"hm_loss": const}, {"hm_loss": const, "2D_IoU": const * 2}
    source = make(kind)
    batches = Prefetcher(source, cuda) if prefetch else source
    args = do_train(cfg, model, optimizer, scheduler, warmup, batches, {"iteration": 0}, str(tmp_path), step=step, log_every=3)
    assert args["iteration"] == 4 and len(seen) == 4 and os.path.exists(os.path.join(str(tmp_path), "model_final.pth"))
    for i in range(4):
        assert_same_batch(seen[i], want[kind][i], (kind, prefetch, i))
    for s in list(fresh.values()) + [source]:
        if hasattr(s, "close"):
            s.close()


def test_two_real_iterations_from_the_fixture_directory(cuda, kitti, tmp_path, caplog):
    """8. `train_step` on `KeypointDetector` fed by the resident split through the prefetcher: finite logged losses, parameters
    that moved, and a `model_final` that loads into a fresh model with an equal state dict at iteration 2."""
    from dcd_amd.data.batches import Prefetcher, ResidentBatches
    from dcd_amd.engine.train import do_train, resume
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, init_like_trained
    from dcd_amd.config import get_cfg
    from dcd_amd.model.detector import KeypointDetector
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "SOLVER.MAX_ITERATION", 2, "SOLVER.IMS_PER_BATCH", 2])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda).train()
    init_like_trained(model)
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    batches = Prefetcher(ResidentBatches(kitti["split"], 2, seed=0), cuda)
    with caplog.at_level(logging.INFO, logger="dcd_amd.trainer"):
        args = do_train(cfg, model, optimizer, scheduler, warmup, batches, {"iteration": 0}, str(tmp_path))
    assert args["iteration"] == 2
    line = [r.getMessage() for r in caplog.records if "iter: 2" in r.getMessage()][-1]
    logged = {k: float(v) for k, v in re.findall(r"(\S+): (\S+) \(", line)}
    losses = {k: v for k, v in logged.items() if "loss" in k}
    assert "loss" in losses and "hm_loss" in losses and len(losses) >= 8 and all(math.isfinite(v) for v in losses.values()), line
    assert losses["loss"] > 0 and "time" in logged and "data" in logged
    final = model.state_dict()
    moved = [k for k in initial if initial[k].is_floating_point() and not torch.equal(initial[k], final[k])]
    assert len(moved) > len(initial) // 2
    torch.manual_seed(1)
    fresh = KeypointDetector(cfg).to(cuda).train()
    fresh_opt = build_optimizer(fresh, cfg)
    fresh_sched, _ = build_scheduler(fresh_opt, cfg)
    loaded = resume(os.path.join(str(tmp_path), "model_final.pth"), fresh, fresh_opt, fresh_sched)
    assert loaded["iteration"] == 2
    got = fresh.state_dict()
    assert set(got) == set(final)
    for k in final:
        assert torch.equal(got[k], final[k]), k


def test_collection_pass_with_a_validation_split(cuda, kitti, tmp_path):
    """`TEST.GENERATE_GMW` with `val=(files, pipeline)` on the real detector: start + len(batches) // IMS_PER_BATCH forwards that
    change nothing in the model, `gen_data_train.json`, `gen_data_infer.json` with the records of every validation image (written
    through `forward_batch` / `infer_records_batch` / `dump_gen_data_infer`), the evaluation's dict in the arguments, no checkpoint."""
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.GENERATE_GMW", True, "TEST.DETECTIONS_THRESHOLD", 0.0,
                        "SOLVER.IMS_PER_BATCH", 1])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    val_files = KittiFiles(kitti["files"].root, cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=False)
    assert len(val_files) == 4
    out = str(tmp_path / "out")
    args = do_train(cfg, model, optimizer, scheduler, warmup, ResidentBatches(kitti["split"], 1, seed=0), {"iteration": 0}, out,
                    val=(val_files, DeviceInputPipeline(cfg, cuda, is_train=False)))
    assert args["iteration"] == 3 and model.training
    after = model.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert all(p.grad is None for p in model.parameters()) and optimizer.state_dict()["state"] == {}
    assert sorted(os.listdir(out)) == ["gen_data", "inference"]
    assert sorted(os.listdir(os.path.join(out, "gen_data"))) == ["gen_data_infer.json", "gen_data_train.json"]
    train = json.load(open(os.path.join(out, "gen_data", "gen_data_train.json")))
    assert len(train["img_idx"]) == 3 and len(train["kpts_2d"]) == 3 and sum(len(x) for x in train["pred_rot"]) >= 3
    infer = json.load(open(os.path.join(out, "gen_data", "gen_data_infer.json")))
    assert sorted(infer) == [val_files.img_id(i) for i in range(4)]
    records = [r for v in infer.values() for r in v]
    assert records and all(len(v) <= cfg.TEST.DETECTIONS_PER_IMG for v in infer.values())
    for r in records:
        assert set(r) == {"kpts_2d", "kpts_3d", "pred_rot", "box", "dim", "pred_location", "score", "cat"}
        assert np.asarray(r["kpts_2d"]).shape == (73, 2) and np.asarray(r["kpts_3d"]).shape == (73, 3) and len(r["box"]) == 4
        assert np.isfinite(np.asarray(r["pred_location"])).all()
    assert "R40" in args["eval"]
    assert sorted(os.listdir(os.path.join(out, "inference", "data"))) == [val_files.img_id(i) + ".txt" for i in range(4)]


def test_command_line_trains_and_resumes(cuda, kitti, tmp_path):
    """`python -m dcd_amd.engine.train`'s `main`: one iteration from the fixture directory, then a second call with a larger
    SOLVER.MAX_ITERATION picks up `last_checkpoint` and goes on from iteration 1."""
    from dcd_amd.engine.train import main
    out = str(tmp_path / "run")
    argv = ["--root", kitti["files"].root, "--output-dir", out, "--batch", "2", "--log-every", "1",
            "MODEL.PRETRAIN", "False", "MODEL.USE_SYNC_BN", "False", "SOLVER.SAVE_CHECKPOINT_INTERVAL", "1000", "SOLVER.MAX_ITERATION"]
    assert main(argv + ["1"])["iteration"] == 1
    first = torch.load(os.path.join(out, "model_final.pth"), weights_only=False)
    assert first["iteration"] == 1 and open(os.path.join(out, "last_checkpoint")).read() == os.path.join(out, "model_final.pth")
    assert main(argv + ["2", "--streaming"])["iteration"] == 2
    second = torch.load(os.path.join(out, "model_final.pth"), weights_only=False)
    assert second["iteration"] == 2
    moved = [k for k, v in first["model"].items() if v.is_floating_point() and not torch.equal(v, second["model"][k])]
    assert len(moved) > len(first["model"]) // 2
