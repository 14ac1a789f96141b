"""`dcd_depth_estimates` / `dcd_depth_accumulate` (csrc/depth_report.hip) on the device -- against the host build of the same
header, against the decode kernel whose reported depth method 7 is, isolation, run-to-run bits, guard bands, refusals --
`_predictor.heads_at` against the sparse evaluation path it was cut out of and against the dense map, and
`engine.depth_report.depth_report` end to end on the four-image fixture directory.  Kernel shapes: 24 x 80 maps, 2 images, 16 slots
each, 73 key points (the candidates of test_decode_host on which every clamp of the decode occurs)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_decode_host as DH  # noqa: E402
import test_depth_report_host as RH  # noqa: E402
import test_input_host as IH  # noqa: E402
from arena import Arena  # noqa: E402
from test_depth_report_host import host_report  # noqa: E402,F401  (the fixture: the host build of the header)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False]
N = DH.BRANCH_B * DH.BRANCH_K


def _np(t):
    return t.detach().cpu().numpy()


def _device_call(cuda, pp, vectors, ys, xs, classes, gt_z, valid, targets, edges=RH.EDGES_SMALL, poison=True):
    """Both entry points on buffers of one `Arena`: (est, table, outside) as numpy arrays after the guard bands were checked."""
    from dcd_amd import _lib, ops
    arena = Arena(cuda, poison=poison)
    B, M, C = vectors.shape
    f = lambda t, name: arena.place(t.detach().cpu().float().reshape(-1), name)  # noqa: E731
    vec = arena.place(vectors.detach().cpu().float().reshape(B * M, C), "vectors")
    per_slot = [f(t, n) for t, n in ((ys, "ys"), (xs, "xs"), (classes, "classes"), (gt_z, "gt_z"))]
    val = arena.place(valid.detach().cpu().to(torch.int32), "valid32")           # (the arena places 4- and 8-byte words)
    val8 = val.to(torch.uint8)
    table_in = arena.place(pp._image_table(targets, cuda).cpu(), "image_table")
    est = arena.out((B * M, RH.ROW), "est")
    n_bins = len(edges) - 1
    table = arena.place(torch.zeros((RH.NUM_CLASSES, n_bins, RH.NM, RH.STATS), dtype=torch.float64), "table", inplace=True)
    outside = arena.place(torch.zeros(RH.NUM_CLASSES, dtype=torch.int64), "outside", inplace=True)
    a = ops.decode_args(pp.decode_spec(), B, M, C)
    L = _lib.lib()
    st = L.dcd_depth_estimates(_lib.stream_of(vec), vec.data_ptr(), *[t.data_ptr() for t in per_slot], val8.data_ptr(),
                               table_in.data_ptr(), a, est.data_ptr())
    assert st == 0
    c_edges = (ctypes.c_float * len(edges))(*edges)
    st = L.dcd_depth_accumulate(_lib.stream_of(vec), est.data_ptr(), B * M, c_edges, n_bins, RH.NUM_CLASSES, table.data_ptr(),
                                outside.data_ptr())
    assert st == 0
    arena.check("depth report kernels")
    return _np(est), _np(table), _np(outside)


def test_kernel_against_the_host_build(cuda, host_report):  # noqa: F811
    pp = DH.branch_post_processor(cuda)
    (vectors, ys, xs, classes, gt_z, valid, targets), planted = RH.report_inputs(pp, cuda)
    est, table, outside = _device_call(cuda, pp, vectors, ys, xs, classes, gt_z, valid, targets)
    st, ref = RH.host_estimates(host_report, vectors, ys, xs, classes, gt_z, valid, pp._image_table(targets, cuda).cpu(), pp.decode_spec())
    assert st == 0
    # the leading columns, the empty rows, `mean` and `oracle` from the device's own four estimates
    RH.check_rows_against_numpy(est, gt_z, valid, classes, planted)
    assert RH.same_bits(est[:, :3], ref[:, :3])
    # the estimates: 1e-4 of the column's largest finite magnitude in the host build (expf / atan2f differ between the builds)
    for m in range(RH.NM - 1):
        got, want = est[:, 3 + m].astype(np.float64), ref[:, 3 + m].astype(np.float64)
        finite = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), finite), m
        err = np.abs(got[finite] - want[finite]).max() / (np.abs(want[finite]).max() + 1e-6)
        print("method %d: %.3e of the column's scale" % (m, err))
        assert err <= 1e-4, (m, err)
    # the `hard` index: the host's choice, found among its four estimates, is the device's choice among its own
    on = RH._flat(valid, np.uint8) != 0
    for s in np.nonzero(on)[0]:
        best = [i for i in range(4) if RH.same_bits(ref[s, 3 + i], ref[s, 3 + RH.HARD])]
        assert best and any(RH.same_bits(est[s, 3 + i], est[s, 3 + RH.HARD]) for i in best), s
    # the tables: bit-equal to the slot-order double sums of the device's own rows, and the counts those of the host build
    RH.check_tables(table, outside, est, RH.EDGES_SMALL, RH.NUM_CLASSES)
    st, host_table, host_outside = RH.host_accumulate(host_report, ref, RH.EDGES_SMALL, RH.NUM_CLASSES)
    assert st == 0
    np.testing.assert_array_equal(outside, host_outside)
    np.testing.assert_array_equal(table[..., 0], host_table[..., 0])
    np.testing.assert_array_equal(table[..., 4], host_table[..., 4])
    assert table[..., 0].sum() > 0 and outside.sum() >= 2


def test_edges_column_is_the_depth_the_decode_kernel_reports(cuda):
    from dcd_amd import ops
    pp = DH.branch_post_processor(cuda)
    vectors, topk, targets = DH.branch_inputs(pp, cuda)
    ys, xs, classes = RH.slots_of(topk)
    table, spec = pp._image_table(targets, cuda), pp.decode_spec()
    rows = _np(ops.decode_detections(vectors, topk, table, spec)[0])
    ones = torch.ones((DH.BRANCH_B, DH.BRANCH_K), device=cuda)
    est = _np(ops.depth_estimates(vectors, ys, xs, classes, 20.0 * ones, ones, table, spec))
    assert est.shape == (N, RH.ROW) and np.isfinite(rows[:, 11]).all()
    assert RH.same_bits(est[:, 3 + RH.EDGES], rows[:, 11])
    # batches of different size through the op: the tables of 32 slots at once, of 2 x 16 and of 32 x 1 have the same bits
    whole = ops.depth_tables(RH.NUM_CLASSES, 3, cuda)
    dev_est = torch.from_numpy(est).to(cuda)
    ops.depth_accumulate(dev_est, RH.EDGES_SMALL, *whole)
    for step in (16, 1):
        parts = ops.depth_tables(RH.NUM_CLASSES, 3, cuda)
        for s in range(0, N, step):
            ops.depth_accumulate(dev_est[s:s + step], RH.EDGES_SMALL, *parts)
        assert RH.same_bits(_np(parts[0]), _np(whole[0])) and RH.same_bits(_np(parts[1]), _np(whole[1])), step
    assert _np(whole[0])[..., 0].sum() > 0


def test_a_broken_slot_touches_nobody_else_and_runs_are_bit_equal(cuda):
    pp = DH.branch_post_processor(cuda)
    (vectors, ys, xs, classes, gt_z, valid, targets), planted = RH.report_inputs(pp, cuda)
    clean = _device_call(cuda, pp, vectors, ys, xs, classes, gt_z, valid, targets)
    again = _device_call(cuda, pp, vectors, ys, xs, classes, gt_z, valid, targets, poison=False)     # zero-filled outputs: the same bits
    for a, b in zip(clean, again):
        assert RH.same_bits(a, b)
    broken = vectors.clone()
    huge, nan = 5, DH.BRANCH_K + 3                                              # one valid slot in each image
    assert huge not in planted["empty"] and nan not in planted["empty"]
    broken[0, 5] = 1e30
    broken[1, 3] = float("nan")
    out = _device_call(cuda, pp, broken, ys, xs, classes, gt_z, valid, targets)
    others = np.ones(N, bool)
    others[[huge, nan]] = False
    assert RH.same_bits(clean[0][others], out[0][others])
    assert not RH.same_bits(clean[0][huge], out[0][huge]) and not RH.same_bits(clean[0][nan], out[0][nan])
    # a NaN vector: every estimate that comes from the four depths is NaN (the edge solver's clamp, fmin / fmax, drops a NaN and
    # leaves 2 - P[2][3] there, as it does in the decode)
    assert not np.isfinite(out[0][nan, 3:3 + RH.EDGES]).any() and np.isnan(out[0][nan, 3 + RH.ORACLE])
    # (the empty slot whose vector is NaN throughout is part of `report_inputs`: its row is zeros in every call)
    assert (out[0][planted["nan_vector"]] == 0).all()


def test_refused_configurations(cuda):
    from dcd_amd import _lib, ops
    pp = DH.branch_post_processor(cuda)
    vectors, topk, targets = DH.branch_inputs(pp, cuda)
    ys, xs, classes = RH.slots_of(topk)
    table, spec = pp._image_table(targets, cuda), pp.decode_spec()
    L = _lib.lib()
    vec = vectors.reshape(-1, vectors.shape[-1]).contiguous()
    gt_z = torch.full((N,), 20.0, device=cuda)
    valid = torch.ones(N, dtype=torch.uint8, device=cuda)
    est = torch.full((N, RH.ROW), -7.0, device=cuda)

    def status(a):
        return L.dcd_depth_estimates(_lib.stream_of(vec), vec.data_ptr(), ys.data_ptr(), xs.data_ptr(), classes.data_ptr(),
                                     gt_z.data_ptr(), valid.data_ptr(), table.data_ptr(), a, est.data_ptr())
    a = ops.decode_args(spec, DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])
    a.K = 129                                                                   # M = 129
    assert status(a) == 1
    assert status(ops.decode_args(dict(spec, nk=129), DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])) == 1
    assert status(ops.decode_args(dict(spec, orientation=ops.DECODE_ORIENTATION["head-axis"]), DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])) == 1
    tab = torch.full((8, 17, RH.NM, RH.STATS), -7.0, dtype=torch.float64, device=cuda)
    out = torch.full((9,), -7, dtype=torch.int64, device=cuda)
    rows = torch.zeros((N, RH.ROW), device=cuda)

    def acc_status(edges, num_classes):
        c_edges = (ctypes.c_float * len(edges))(*edges)
        return L.dcd_depth_accumulate(_lib.stream_of(rows), rows.data_ptr(), N, c_edges, len(edges) - 1, num_classes, tab.data_ptr(),
                                      out.data_ptr())
    assert acc_status([float(i) for i in range(18)], 3) == 1                    # 17 bins
    assert acc_status([0.0, 30.0, 20.0], 3) == 1                                # decreasing
    assert acc_status([0.0, 10.0, 10.0], 3) == 1
    assert acc_status([0.0, 10.0], 9) == 1                                      # 9 classes
    torch.cuda.synchronize()
    assert bool((est == -7.0).all()) and bool((tab == -7.0).all()) and bool((out == -7).all())
    with pytest.raises(_lib.DcdHipError):
        ops.depth_estimates(vectors, ys, xs, classes, gt_z, valid, table, dict(spec, nk=129))
    with pytest.raises(_lib.DcdHipError):
        ops.depth_accumulate(rows, [0.0, 30.0, 20.0], *ops.depth_tables(3, 2, cuda))


def test_heads_at_is_the_sparse_evaluation_path_and_the_dense_map(cuda):
    from dcd_amd.config import get_cfg
    from dcd_amd.data.synthetic import make_batch
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    from dcd_amd.structures.params_3d import stack_field
    cfg = get_cfg(opts=OPTS + ["INPUT.WIDTH_TRAIN", 320, "INPUT.HEIGHT_TRAIN", 96])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    model.eval()
    images, targets = make_batch(2, seed=0, n_objects=3, input_size=(320, 96), device=cuda)
    predictor = model.heads.predictor
    with torch.no_grad():
        feats = model.backbone(images)
        predictor.sparse_eval_heads = True
        try:
            sparse = predictor(feats, targets)
        finally:
            predictor.sparse_eval_heads = False
        assert sparse["reg"] is None
        again = predictor.heads_at(feats, targets, sparse["topk"][1])
        assert again.shape == sparse["reg_pois"].shape and torch.equal(again, sparse["reg_pois"])
        # at the targets' centres: what the dense map holds there, at the bar the batched evaluation is held to against the
        # one-image loop (dense heads) in test_gpu_eval_batched.py: 1e-4 of the column's scale plus 1e-4
        dense = predictor(feats, targets)["reg"]
        centers = stack_field(targets, "target_centers").long()
        lin = centers[:, :, 1] * dense.shape[3] + centers[:, :, 0]
        got = predictor.heads_at(feats, targets, lin)
        want = dense.flatten(2).gather(2, lin.unsqueeze(1).expand(-1, dense.shape[1], -1)).transpose(1, 2)
    assert got.shape == want.shape == (2, lin.shape[1], dense.shape[1])
    g, w = _np(got).reshape(-1, dense.shape[1]).astype(np.float64), _np(want).reshape(-1, dense.shape[1]).astype(np.float64)
    bar = 1e-4 * np.abs(w).max(0) + 1e-4
    print("heads_at against the dense map: worst difference / bar %.3f" % (np.abs(g - w) / bar).max())
    assert (np.abs(g - w) <= bar).all()
    # the preconditions of the sparse evaluation path
    with pytest.raises(NotImplementedError, match="gradients"):
        predictor.heads_at(feats, targets, lin)
    model.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training"):
        predictor.heads_at(feats, targets, lin)


# ---- end to end on the fixture directory -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """The fixture directory of tests/test_gpu_eval_batched.py, an initialised detector and a seeded GMW."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.gmw import GMW
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path_factory.mktemp("depth_report"), [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=OPTS)
    files = KittiFiles(root, "train", cfg, is_train=False)
    assert len(files) == 4
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    torch.manual_seed(0)
    gmw = GMW().to(cuda).eval()
    pipe = DeviceInputPipeline(cfg, cuda, is_train=False)
    labelled = 0
    for i in range(len(files)):                                                  # the split's objects, counted from its targets
        _, targets = pipe([files.frame(i)], [files.sample(i)], img_ids=[files.img_id(i)])
        labelled += int(targets[0].get_field("reg_mask").sum())
    assert labelled > 0
    return dict(root=root, cfg=cfg, files=files, model=model, gmw=gmw, pipe=pipe, labelled=labelled)


ARRAYS = ("mae", "bias", "rmse", "count", "nonfinite", "outside")


def _largest_differences(a, b):
    """For the record: how far two passes' results are apart, relative to the larger magnitude, per array."""
    out = {}
    for k in ("mae", "bias", "rmse", "est"):
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        both = np.isfinite(x) & np.isfinite(y)
        out[k] = float((np.abs(x - y)[both] / np.maximum(np.maximum(np.abs(x), np.abs(y))[both], 1e-30)).max()) if both.any() else 0.0
    return out


def _replay_backbone(world, monkeypatch):
    """The backbone replaced by a replay of ONE recorded forward per image of the split, so that every later pass sees the same
    feature bits whatever its batch size.  (The backbone's own forward is not bit-reproducible across batch sizes: its kernels
    are chosen by problem size, see DESIGN.md.)"""
    model, files, pipe = world["model"], world["files"], world["pipe"]
    model.eval()
    recorded = []
    with torch.no_grad():
        for i in range(len(files)):
            images, _ = pipe([files.frame(i)], [files.sample(i)], img_ids=[files.img_id(i)])
            recorded.append((images[0].clone(), model.backbone(images).clone()))

    def replay(images):
        out = []
        for b in range(images.shape[0]):
            hit = [feats for image, feats in recorded if torch.equal(image, images[b])]
            assert len(hit) == 1
            out.append(hit[0])
        return torch.cat(out)
    monkeypatch.setattr(model.backbone, "forward", replay)


def test_batch_sizes_1_and_2_give_bit_equal_results(world):
    """The whole pass at batch 1 and at batch 2, bit for bit.  It holds because the pass runs the backbone one image at a time
    (`backbone_batch=1`, the default): with one backbone call per batch the estimates were measured 6.7e-7 apart (relative) and
    mae / bias / rmse 4.0e-7 -- the backbone's kernels are chosen by problem size, and at batch 2 its `base.level5` is not
    reproducible from run to run at all.  Everything after the backbone does not depend on the batch size: the next
    test."""
    from dcd_amd.engine.depth_report import depth_report
    text1, one = depth_report(world["model"], world["files"], world["pipe"], batch_size=1, per_object=True)
    text2, two = depth_report(world["model"], world["files"], world["pipe"], batch_size=2, per_object=True)
    print("batch 1 against batch 2, largest relative differences: %s" % _largest_differences(one, two))
    for k in ("count", "nonfinite", "outside"):
        assert RH.same_bits(one[k], two[k]), k
    assert one["img_ids"] == two["img_ids"]
    for k in ARRAYS:
        assert RH.same_bits(one[k], two[k]), k
    assert text1 == text2 and RH.same_bits(one["est"], two["est"])


def test_on_the_same_features_the_batch_size_does_not_matter(world, monkeypatch):
    from dcd_amd.engine.depth_report import depth_report
    _replay_backbone(world, monkeypatch)
    results = [depth_report(world["model"], world["files"], world["pipe"], batch_size=b, per_object=True) for b in (1, 2, 3, 8)]
    (text1, one) = results[0]
    for text, other in results[1:]:
        for k in ARRAYS + ("est",):
            assert RH.same_bits(one[k], other[k]), k
        assert text == text1 and other["img_ids"] == one["img_ids"]
    assert one["count"][:, -1, RH.EDGES].sum() > 0


def test_backbone_batch_decides_the_backbone_calls_and_little_else(world):
    from dcd_amd.engine.depth_report import depth_report
    seen = []
    hook = world["model"].backbone.register_forward_hook(lambda m, inp, out: seen.append(int(inp[0].shape[0])))
    try:
        _, one = depth_report(world["model"], world["files"], world["pipe"], batch_size=3)
        per_image, seen[:] = list(seen), []
        _, whole = depth_report(world["model"], world["files"], world["pipe"], batch_size=3, backbone_batch=None)
    finally:
        hook.remove()
    assert per_image == [1, 1, 1, 1] and seen == [3, 1]
    for k in ("count", "nonfinite", "outside"):
        assert RH.same_bits(one[k], whole[k]), k
    # one backbone call per batch: the same report up to the backbone's own dependence on its batch size (measured: 4e-7 of an
    # error; the bar is the 1e-4 of the decode's header family, on the scale of the largest error)
    finite = np.isfinite(one["mae"])
    assert np.array_equal(finite, np.isfinite(whole["mae"]))
    assert np.abs(one["mae"][finite] - whole["mae"][finite]).max() <= 1e-4 * np.abs(one["mae"][finite]).max()
    with pytest.raises(ValueError):
        depth_report(world["model"], world["files"], world["pipe"], backbone_batch=0)


def test_report_reads_nothing_in_the_loop_and_books_every_object(world, monkeypatch):
    from dcd_amd import ops
    from dcd_amd.engine import depth_report as DR
    DR.depth_report(world["model"], world["files"], world["pipe"], batch_size=2)       # warms every cache the loop body fills once
    inner = DR.report_batch
    calls = []

    def guarded(*a, **k):
        """The loop body under the synchronisation check."""
        torch.cuda.set_sync_debug_mode("error")
        try:
            calls.append(1)
            return inner(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(DR, "report_batch", guarded)
    text1, one = DR.depth_report(world["model"], world["files"], world["pipe"], batch_size=2, per_object=True)
    monkeypatch.undo()
    assert len(calls) == 2
    assert one["methods"] == list(ops.DEPTH_METHODS) and one["classes"] == ["Car", "Pedestrian", "Cyclist"]
    held = [one["classes"].index(c) for c in world["files"].classes]             # DATASETS.DETECT_CLASSES: what the targets hold
    assert all(int(one["count"][c].sum() + one["nonfinite"][c].sum() + one["outside"][c]) == 0 for c in range(3) if c not in held)
    n_bins = len(DR.DEFAULT_EDGES) - 1
    assert one["mae"].shape == (len(one["classes"]), n_bins + 1, RH.NM) and one["edges"] == [float(e) for e in DR.DEFAULT_EDGES]
    # every labelled object once: in a bin (a finite or a non-finite estimate, per method) or outside
    for m in range(RH.NM):
        assert int(one["count"][:, -1, m].sum() + one["nonfinite"][:, -1, m].sum() + one["outside"].sum()) == world["labelled"], m
    assert int(one["est"][:, 0].sum()) == world["labelled"] and one["est"].shape == (4 * world["cfg"].DATASETS.MAX_OBJECTS, RH.ROW)
    assert (one["count"][:, :-1].sum(1) == one["count"][:, -1]).all()
    assert one["count"][:, -1, RH.GMW].sum() == 0 and np.isnan(one["mae"][:, :, RH.GMW]).all()       # no GMW: the column is NaN
    assert one["count"][:, -1, RH.EDGES].sum() > 0 and np.isfinite(one["mae"][one["count"] > 0]).all()
    # the tables are the slot-order double sums of the rows the pass returns
    want, want_out = RH.numpy_tables(one["est"], DR.DEFAULT_EDGES, len(one["classes"]))
    np.testing.assert_array_equal(one["outside"], want_out)
    np.testing.assert_array_equal(one["count"][:, :-1], want[..., 0].astype(np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert RH.same_bits(one["mae"][:, :-1], want[..., 1] / want[..., 0])
    assert "direct" in text1 and "oracle" in text1 and all(c in text1 for c in world["files"].classes)
    print(text1)


def test_gmw_column_on_the_same_features(world, monkeypatch):
    """The comparison of the next test with the backbone replayed: filling the tenth column changes no bit of the other nine."""
    from dcd_amd.engine.depth_report import depth_report
    _replay_backbone(world, monkeypatch)
    _, plain = depth_report(world["model"], world["files"], world["pipe"], batch_size=2, per_object=True)
    _, with_gmw = depth_report(world["model"], world["files"], world["pipe"], batch_size=3, gmw=world["gmw"], gmw_batch=48, per_object=True)
    on = plain["est"][:, 0] != 0
    assert np.isfinite(with_gmw["est"][on, 3 + RH.GMW]).all() and (with_gmw["est"][~on] == 0).all()
    assert RH.same_bits(with_gmw["est"][:, :3 + RH.GMW], plain["est"][:, :3 + RH.GMW])
    for k in ("mae", "bias", "rmse", "count", "nonfinite"):
        assert RH.same_bits(with_gmw[k][:, :, :RH.GMW], plain[k][:, :, :RH.GMW]), k
    assert RH.same_bits(with_gmw["outside"], plain["outside"])


def test_gmw_column(world):
    """A pass with `gmw=` against a pass without: the tenth column finite on every labelled slot, the other nine unchanged bit
    for bit (two passes are two forwards of the backbone: reproducible because it runs one image at a time, see
    test_batch_sizes_1_and_2_give_bit_equal_results)."""
    from dcd_amd.engine.depth_report import depth_report
    world["model"].train()
    _, plain = depth_report(world["model"], world["files"], world["pipe"], batch_size=2, per_object=True)
    _, with_gmw = depth_report(world["model"], world["files"], world["pipe"], batch_size=2, gmw=world["gmw"], gmw_batch=48, per_object=True)
    print("with gmw= against without, largest relative differences: %s" % _largest_differences(plain, with_gmw))
    assert world["model"].training is True and world["gmw"].training is False    # both modes restored
    world["model"].eval()
    on = plain["est"][:, 0] != 0
    assert on.sum() == world["labelled"]
    assert np.isfinite(with_gmw["est"][on, 3 + RH.GMW]).all() and np.isnan(plain["est"][on, 3 + RH.GMW]).all()
    assert RH.same_bits(with_gmw["est"][:, :3 + RH.GMW], plain["est"][:, :3 + RH.GMW])
    assert (with_gmw["est"][~on] == 0).all()
    for k in ("mae", "bias", "rmse", "count", "nonfinite"):
        assert RH.same_bits(with_gmw[k][:, :, :RH.GMW], plain[k][:, :, :RH.GMW]), k
    assert with_gmw["count"][:, -1, RH.GMW].sum() + with_gmw["outside"].sum() == world["labelled"]
    # the refinement partition does not matter to a slot's depth beyond the extractors' batch behaviour: every slot in one group
    _, whole = depth_report(world["model"], world["files"], world["pipe"], batch_size=2, gmw=world["gmw"], gmw_batch=256, per_object=True)
    assert np.isfinite(whole["est"][on, 3 + RH.GMW]).all()


def test_a_split_without_labels_is_refused(world, tmp_path):
    import shutil
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.depth_report import depth_report
    root = str(tmp_path / "testing")
    for d in ("ImageSets", "calib", "image_2"):
        shutil.copytree(os.path.join(world["root"], d), os.path.join(root, d))
    shutil.copy(os.path.join(root, "ImageSets", "train.txt"), os.path.join(root, "ImageSets", "test.txt"))
    files = KittiFiles(root, "test", world["cfg"], is_train=False)
    assert not files.has_labels
    with pytest.raises(ValueError, match="label"):
        depth_report(world["model"], files, world["pipe"], batch_size=2)
    with pytest.raises(ValueError, match="edges"):
        depth_report(world["model"], world["files"], world["pipe"], edges=(0, 20, 10))


def test_command_line_prints_the_table(world, tmp_path):
    from dcd_amd.engine.train import save_checkpoint
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    optimizer = build_optimizer(world["model"], world["cfg"])
    scheduler, _ = build_scheduler(optimizer, world["cfg"])
    ckpt = save_checkpoint(str(tmp_path / "ckpt"), "model_final", world["model"], optimizer, scheduler, {"iteration": 1})
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "dcd_amd.engine.depth_report", "--root", world["root"], "--split", "train", "--ckpt", ckpt,
           "--output-dir", out, "--batch", "3", "--edges", "0", "20", "40", "80"] + [str(v) for v in OPTS]
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "0-20" in done.stdout and "oracle" in done.stdout and "RMSE" in done.stdout
    back = json.load(open(os.path.join(out, "depth_report.json")))
    assert back["edges"] == [0.0, 20.0, 40.0, 80.0] and np.asarray(back["count"]).shape == (3, 4, RH.NM)
    _, here = __import__("dcd_amd.engine.depth_report", fromlist=["depth_report"]).depth_report(
        world["model"], world["files"], world["pipe"], batch_size=1, edges=(0, 20, 40, 80))
    assert np.array_equal(np.asarray(back["count"]), here["count"]) and open(os.path.join(out, "depth_report.txt")).read() in done.stdout
