"""`dcd_dis_iou_estimates` / `dcd_dis_iou_accumulate` (csrc/dis_iou.hip) on the device -- against the host build of the same header
and the float64 restatement (tests/dis_iou_refs.py), against the decode and the depth report's kernels whose bits `full` and
`depth:<m>` carry, isolation, run-to-run bits, guard bands, edge shapes -- and `engine.dis_iou_report.dis_iou_report` end to end on
the four-image fixture directory.  Kernel shapes: 24 x 80 maps, 2 images, 16 slots each, 73 key points (the candidates of
test_decode_host on which every clamp of the decode occurs), labels seeded around the predictions (test_dis_iou_host.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dis_iou_refs as R  # noqa: E402
import test_decode_host as DH  # noqa: E402
import test_dis_iou_host as H  # noqa: E402
from arena import Arena  # noqa: E402
from test_dis_iou_host import host_dis  # noqa: E402,F401  (the fixture: the host build of the header)
from test_gpu_depth_report import OPTS, _replay_backbone, world  # noqa: E402,F401  (the fixture directory, a detector, a seeded GMW)
from test_depth_report_host import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = H.N


def _np(t):
    return t.detach().cpu().numpy()


def _device_call(cuda, inp, edges=H.EDGES_SMALL, thr=None, poison=True, gmw=True, want_boxes=True, vectors=None, spec=None):
    """Both entry points on buffers of one `Arena`, poisoned and guarded: (dis, boxes or None, table, outside) as numpy arrays
    after the guards, the inputs and the "every output word written" rule were checked."""
    from dcd_amd import _lib, ops
    thr = H.thresholds() if thr is None else thr
    arena = Arena(cuda, poison=poison)
    vectors = inp["vectors"] if vectors is None else vectors
    B, M, C = vectors.shape
    f = lambda t, name: arena.place(t.detach().cpu().float().reshape(-1), name)  # noqa: E731
    vec = arena.place(vectors.detach().cpu().float().reshape(B * M, C), "vectors")
    ys, xs, classes, gt = f(inp["ys"], "ys"), f(inp["xs"], "xs"), f(inp["classes"], "classes"), f(inp["gt"], "gt")
    valid = arena.place(inp["valid"].detach().cpu().to(torch.uint8).reshape(-1), "valid")
    table_in = arena.place(inp["table"].cpu(), "image_table")
    gmw_z = f(inp["gmw_z"], "gmw_z") if gmw else None
    dis = arena.out((B * M, R.ROW), "dis")
    boxes = arena.out((B * M, R.NBOX, R.BOX), "boxes") if want_boxes else None
    n_bins, num_classes = len(edges) - 1, thr.shape[0]
    table = arena.place(torch.zeros((num_classes, n_bins, R.NV, R.NMETRIC, R.STATS), dtype=torch.float64), "table", inplace=True)
    outside = arena.place(torch.zeros(num_classes, dtype=torch.int64), "outside", inplace=True)
    a = ops.decode_args(spec or inp["spec"], B, M, C)
    L = _lib.lib()
    st = L.dcd_dis_iou_estimates(_lib.stream_of(vec), vec.data_ptr(), ys.data_ptr(), xs.data_ptr(), classes.data_ptr(), gt.data_ptr(),
                                 valid.data_ptr(), table_in.data_ptr(), _lib.ptr(gmw_z), a, dis.data_ptr(), _lib.ptr(boxes))
    assert st == 0
    c_edges = (ctypes.c_float * len(edges))(*edges)
    flat = [float(t) for t in np.asarray(thr).reshape(-1)]
    st = L.dcd_dis_iou_accumulate(_lib.stream_of(vec), dis.data_ptr(), B * M, c_edges, n_bins, num_classes,
                                  (ctypes.c_double * len(flat))(*flat), table.data_ptr(), outside.data_ptr())
    assert st == 0
    arena.check("dis_iou kernels")
    return _np(dis), (None if boxes is None else _np(boxes)), _np(table), _np(outside)


def test_kernel_against_the_host_build_and_the_restatement(cuda, host_dis):  # noqa: F811
    """Boxes per column (h w l x y z ry) as a fraction of the column's largest finite magnitude in the restatement: the bar is
    4 x the host build's own distance (5.72e-08 6.97e-08 3.28e-08 1.31e-07 8.80e-08 8.76e-08 1.46e-07, test_dis_iou_host.py); the
    device's distance is printed (measured on an MI355X: 5.72e-08 6.97e-08 3.28e-08 1.00e-07 9.16e-08 1.06e-07 1.46e-07; overlaps
    2.89e-07 from the exact clip of the device's own boxes, bar 1e-6)."""
    pp = DH.branch_post_processor(cuda)
    inp = H.report_inputs(pp, cuda)
    thr = H.thresholds()
    dis, boxes, table, outside = _device_call(cuda, inp)
    st, ref, ref_boxes = H.host_estimates(host_dis, inp)
    assert st == 0
    on = H._flat(inp["valid"], np.uint8) != 0
    assert same_bits(dis[:, :3], ref[:, :3]) and same_bits(dis[~on], np.zeros_like(dis[~on])) and same_bits(boxes[~on], np.zeros_like(boxes[~on]))
    assert same_bits(boxes[:, 0], ref_boxes[:, 0])                                # the label's box: no libm in it
    want_boxes, want_rows, _ = H.restatement(inp)
    host = H.column_distance(ref_boxes, want_boxes, on)
    device = H.column_distance(boxes, want_boxes, on)
    print("the host build from the restatement, per column: %s" % np.array2string(host, precision=2))
    print("the device from the restatement:                 %s" % np.array2string(device, precision=2))
    assert (device <= 4 * host).all(), (device, host)
    assert np.array_equal(np.isfinite(dis), np.isfinite(ref)) and np.array_equal(np.isfinite(boxes), np.isfinite(ref_boxes))
    H.check_overlaps_against_own_boxes(dis, boxes, inp["classes"], inp["valid"], "device")
    H.check_hit_decisions(dis, want_rows, inp["classes"], inp["valid"], thr, "device")
    # the tables: the slot-order double sums of the device's own rows, and the host build's counts
    H.check_tables(table, outside, dis, H.EDGES_SMALL, thr, H.NUM_CLASSES)
    st, host_table, host_outside = H.host_accumulate(host_dis, ref, H.EDGES_SMALL, thr, H.NUM_CLASSES)
    assert st == 0
    np.testing.assert_array_equal(outside, host_outside)
    for stat in (0, 5):
        np.testing.assert_array_equal(table[..., stat], host_table[..., stat])
    assert table[..., 0].sum() > 0 and table[..., 3].sum() > 0
    # boxes = null: the same rows, and the arena's guards say nothing else was written
    no_boxes = _device_call(cuda, inp, want_boxes=False)
    assert no_boxes[1] is None and same_bits(no_boxes[0], dis) and same_bits(no_boxes[2], table)


def test_full_is_the_decodes_row_and_the_depths_are_the_depth_reports(cuda):
    from dcd_amd import ops
    pp = DH.branch_post_processor(cuda)
    inp = H.report_inputs(pp, cuda)
    on = H._flat(inp["valid"], np.uint8) != 0
    B, M = DH.BRANCH_B, DH.BRANCH_K
    rows = _np(ops.decode_detections(inp["clean"], inp["topk"], inp["table"], inp["spec"])[0])
    shaped = lambda t: t.reshape(B, M)  # noqa: E731
    dis, boxes = ops.dis_iou_estimates(inp["vectors"], inp["ys"], inp["xs"], inp["classes"], inp["gt"].reshape(B, M, 9), shaped(inp["valid"]),
                                       inp["table"], inp["spec"], gmw_z=shaped(inp["gmw_z"]), want_boxes=True)
    dis, boxes = _np(dis), _np(boxes)
    assert dis.shape == (N, ops.DIS_ROW) and boxes.shape == (N, 1 + len(ops.DIS_VARIANTS), ops.DIS_BOX)
    assert ops.DIS_VARIANTS == R.VARIANTS and ops.DIS_ROW == R.ROW and ops.DIS_STATS == R.STATS and ops.DIS_METRICS == ("bev", "3d")
    assert np.isfinite(rows[on, 6:13]).all() and same_bits(boxes[on, 1 + R.FULL], rows[on, 6:13])
    est = _np(ops.depth_estimates(inp["vectors"], inp["ys"], inp["xs"], inp["classes"], inp["gt"][:, 4], inp["valid"], inp["table"], inp["spec"]))
    z = boxes[:, 1 + R.DEPTH0:1 + R.DEPTH0 + 10, 5]
    assert same_bits(z[on, :R.GMW], est[on, 3:3 + R.GMW]) and same_bits(z[on, R.GMW], H._flat(inp["gmw_z"])[on])
    plain = _np(ops.dis_iou_estimates(inp["vectors"], inp["ys"], inp["xs"], inp["classes"], inp["gt"], inp["valid"], inp["table"], inp["spec"]))
    gm = [3 + R.NV - 1, 3 + 2 * R.NV - 1]
    keep = [c for c in range(R.ROW) if c not in gm]
    assert np.isnan(plain[on][:, gm]).all() and same_bits(plain[:, keep], dis[:, keep])
    # the op's tables: 32 slots at once, 2 x 16 and 32 x 1 have the same bits
    thr = H.thresholds()
    dev = torch.from_numpy(dis).to(cuda)
    whole = ops.dis_iou_tables(H.NUM_CLASSES, 3, cuda)
    ops.dis_iou_accumulate(dev, H.EDGES_SMALL, thr, *whole)
    for step in (16, 1):
        parts = ops.dis_iou_tables(H.NUM_CLASSES, 3, cuda)
        for s in range(0, N, step):
            ops.dis_iou_accumulate(dev[s:s + step], H.EDGES_SMALL, thr, *parts)
        assert same_bits(_np(parts[0]), _np(whole[0])) and same_bits(_np(parts[1]), _np(whole[1])), step
    H.check_tables(_np(whole[0]), _np(whole[1]), dis, H.EDGES_SMALL, thr, H.NUM_CLASSES)


def test_a_broken_slot_touches_nobody_else_and_runs_are_bit_equal(cuda):
    pp = DH.branch_post_processor(cuda)
    inp = H.report_inputs(pp, cuda)
    clean = _device_call(cuda, inp)
    again = _device_call(cuda, inp)
    zeroed = _device_call(cuda, inp, poison=False)                                # zero-filled outputs: the same bits
    for a, b, c in zip(clean, again, zeroed):
        assert same_bits(a, b) and same_bits(a, c)
    broken = inp["vectors"].clone()
    slot = DH.BRANCH_K + 3
    assert slot not in H.EMPTY
    broken.view(N, -1)[slot] = float("nan")
    out = _device_call(cuda, inp, vectors=broken)
    others = np.arange(N) != slot
    assert same_bits(clean[0][others], out[0][others]) and same_bits(clean[1][others], out[1][others])
    # a NaN vector: every variant that reads a head is NaN in both metrics (the all-pairs depth stays finite -- the solver's clamp
    # drops a NaN -- but `depth:edges` sits at the label's offset, which no head enters, so it alone stays finite with `depth:gmw`)
    finite = np.isfinite(out[0][slot, 3:].reshape(R.NMETRIC, R.NV))
    assert (finite == finite[0]).all() and set(np.nonzero(finite[0])[0]) == {R.DEPTH0 + R.EDGES, R.DEPTH0 + R.GMW}
    assert (out[0][H.EMPTY[1]] == 0).all()                                        # (the empty slot whose vector is NaN throughout)


@pytest.mark.parametrize("M,nk", [(1, 73), (128, 73), (128, 2)])
def test_edge_shapes(cuda, host_dis, M, nk):  # noqa: F811
    """1 and 128 slots per image, 2 key points: device against host build and the exact clip, on seeded vectors and labels."""
    pp = DH.branch_post_processor(cuda)
    base = H.report_inputs(pp, cuda)
    spec = dict(base["spec"], nk=nk)
    B, C = 2, base["vectors"].shape[2]
    rng = np.random.RandomState(M + nk)
    scale = base["clean"].std(dim=(0, 1)).cpu().numpy()
    vectors = torch.from_numpy((rng.normal(0, 1, (B, M, C)) * scale).astype(np.float32))
    ys, xs, classes = (torch.from_numpy(rng.randint(0, hi, (B, M)).astype(np.float32)) for hi in (24, 80, 3))
    table = base["table"].cpu()
    gt, gmw_z = R.seeded_labels(spec, vectors.numpy(), ys.numpy(), xs.numpy(), classes.numpy(), table.numpy(), 3)
    valid = (rng.rand(B * M) < 0.9).astype(np.uint8)
    valid[0] = 1
    inp = dict(vectors=vectors, ys=ys, xs=xs, classes=classes, gt=torch.from_numpy(gt), gmw_z=torch.from_numpy(gmw_z),
               valid=torch.from_numpy(valid), table=table, spec=spec)
    dis, boxes, table_out, outside = _device_call(cuda, inp, spec=spec)
    st, ref, ref_boxes = H.host_estimates(host_dis, inp, spec=spec)
    assert st == 0 and same_bits(dis[:, :3], ref[:, :3]) and same_bits(dis[valid == 0], ref[valid == 0])
    assert np.array_equal(np.isfinite(dis), np.isfinite(ref)) and np.array_equal(np.isfinite(boxes), np.isfinite(ref_boxes))
    want_boxes, _ = R.boxes_of(spec, vectors.numpy(), ys.numpy(), xs.numpy(), classes.numpy(), gt, valid, table.numpy(), gmw_z)
    on = valid != 0
    host, device = H.column_distance(ref_boxes, want_boxes, on), H.column_distance(boxes, want_boxes, on)
    print("M = %d, nk = %d: host %s, device %s" % (M, nk, np.array2string(host, precision=2), np.array2string(device, precision=2)))
    assert (device <= 4 * host).all(), (device, host)
    some = np.nonzero(on)[0][::max(1, on.sum() // 16)]                            # the exact clip in Python: on sixteen slots or so
    H.check_overlaps_against_own_boxes(dis[some], boxes[some], classes.reshape(-1)[some], valid[some], "device")
    H.check_tables(table_out, outside, dis, H.EDGES_SMALL, H.thresholds(), H.NUM_CLASSES)


def test_empty_batch_bins_and_gmw_null(cuda):
    pp = DH.branch_post_processor(cuda)
    inp = H.report_inputs(pp, cuda)
    nothing = dict(inp, valid=torch.zeros(N, dtype=torch.uint8))
    dis, boxes, table, outside = _device_call(cuda, nothing)
    assert not dis.any() and not boxes.any() and not table.any() and not outside.any()
    thr = H.thresholds()
    for edges in ((0.0, 100.0), tuple(float(e) for e in np.linspace(0, 80, 17))):
        dis, _, table, outside = _device_call(cuda, inp, edges=edges)
        assert table.shape[1] == len(edges) - 1
        H.check_tables(table, outside, dis, edges, thr, H.NUM_CLASSES)
        assert table[..., 0].sum() > 0
    with_gmw, without = _device_call(cuda, inp), _device_call(cuda, inp, gmw=False)
    on = H._flat(inp["valid"], np.uint8) != 0
    gm = [3 + R.NV - 1, 3 + 2 * R.NV - 1]
    keep = [c for c in range(R.ROW) if c not in gm]
    assert same_bits(with_gmw[0][:, keep], without[0][:, keep]) and np.isnan(without[0][on][:, gm]).all() and np.isfinite(with_gmw[0][on][:, gm]).all()
    assert without[2][..., R.NV - 1, :, 0].sum() == 0 and without[2][..., R.NV - 1, :, 5].sum() > 0


def test_refused_configurations(cuda):
    from dcd_amd import _lib, ops
    pp = DH.branch_post_processor(cuda)
    inp = H.report_inputs(pp, cuda)
    L = _lib.lib()
    B, M, C = inp["vectors"].shape
    vec = inp["clean"].reshape(N, C).contiguous()
    ys, xs, classes, gt = (inp[k].float().reshape(-1).contiguous() for k in ("ys", "xs", "classes", "gt"))
    valid = inp["valid"].to(torch.uint8)
    dis = torch.full((N, R.ROW), -7.0, device=cuda)
    boxes = torch.full((N, R.NBOX, R.BOX), -7.0, device=cuda)

    def status(a, null=None):
        ptrs = [vec.data_ptr(), ys.data_ptr(), xs.data_ptr(), classes.data_ptr(), gt.data_ptr(), valid.data_ptr(), inp["table"].data_ptr()]
        if null is not None:
            ptrs[null] = None
        return L.dcd_dis_iou_estimates(_lib.stream_of(vec), *ptrs, None, a, dis.data_ptr(), boxes.data_ptr())
    good = ops.decode_args(inp["spec"], B, M, C)
    for null in range(7):
        assert status(good, null) == 1
    a = ops.decode_args(inp["spec"], B, M, C)
    a.K = 129
    assert status(a) == 1
    for nk in (1, 129):
        assert status(ops.decode_args(dict(inp["spec"], nk=nk), B, M, C)) == 1
    tab = torch.full((8, 17, R.NV, R.NMETRIC, R.STATS), -7.0, dtype=torch.float64, device=cuda)
    out = torch.full((9,), -7, dtype=torch.int64, device=cuda)
    rows = torch.zeros((N, R.ROW), device=cuda)

    def acc_status(edges, num_classes, thr):
        c_edges = (ctypes.c_float * len(edges))(*edges)
        flat = [float(t) for t in np.asarray(thr).reshape(-1)]
        return L.dcd_dis_iou_accumulate(_lib.stream_of(rows), rows.data_ptr(), N, c_edges, len(edges) - 1, num_classes,
                                        (ctypes.c_double * len(flat))(*flat), tab.data_ptr(), out.data_ptr())
    thr = H.thresholds()
    bad = thr.copy()
    bad[2, 0, 1] = 1.5
    assert acc_status([0.0], 3, thr) == 1                                        # 0 bins
    assert acc_status([float(i) for i in range(18)], 3, thr) == 1                # 17 bins
    assert acc_status([0.0, 30.0, 20.0], 3, thr) == 1 and acc_status([0.0, 10.0, 10.0], 3, thr) == 1
    assert acc_status([0.0, 10.0], 9, np.full((9, 2, 2), 0.5)) == 1              # 9 classes
    assert acc_status([0.0, 10.0], 3, bad) == 1                                  # a threshold of 1.5
    torch.cuda.synchronize()
    assert bool((dis == -7.0).all()) and bool((boxes == -7.0).all()) and bool((tab == -7.0).all()) and bool((out == -7).all())
    with pytest.raises(_lib.DcdHipError):
        ops.dis_iou_estimates(inp["clean"], inp["ys"], inp["xs"], inp["classes"], inp["gt"], inp["valid"], inp["table"], dict(inp["spec"], nk=129))
    with pytest.raises(_lib.DcdHipError):
        ops.dis_iou_accumulate(rows, [0.0, 10.0], bad, *ops.dis_iou_tables(3, 1, cuda))
    with pytest.raises(ValueError):
        ops.dis_iou_estimates(inp["clean"], inp["ys"], inp["xs"], inp["classes"], inp["gt"][:, :8], inp["valid"], inp["table"], inp["spec"])
    with pytest.raises(ValueError):
        ops.dis_iou_accumulate(rows, [0.0, 10.0], thr[:2], *ops.dis_iou_tables(3, 1, cuda))


# ---- end to end on the fixture directory -------------------------------------------------------------------------------------
ARRAYS = ("mean_iou", "hit_rate", "hit_rate_loose", "count", "nonfinite", "outside")


def test_report_batch_sizes_the_hand_loop_and_per_object_rows(world, monkeypatch):  # noqa: F811
    from dcd_amd import ops
    from dcd_amd.engine import dis_iou_report as DI
    from dcd_amd.structures.params_3d import stack_field
    model, files, pipe = world["model"], world["files"], world["pipe"]
    text1, one = DI.dis_iou_report(model, files, pipe, batch_size=1, per_object=True)
    inner, calls = DI.report_batch, []

    def guarded(*a, **k):
        """The loop body under the synchronisation check: nothing is read back."""
        torch.cuda.set_sync_debug_mode("error")
        try:
            calls.append(1)
            return inner(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(DI, "report_batch", guarded)
    results = [DI.dis_iou_report(model, files, pipe, batch_size=b, per_object=True) for b in (2, 4)]
    monkeypatch.undo()
    assert len(calls) == 3
    for text, other in results:
        for k in ARRAYS + ("dis",):
            assert same_bits(one[k], other[k]), k
        assert text == text1 and other["img_ids"] == one["img_ids"]
    slots = world["cfg"].DATASETS.MAX_OBJECTS
    assert one["dis"].shape == (4 * slots, ops.DIS_ROW) and int(one["dis"][:, 0].sum()) == world["labelled"]
    assert one["img_ids"] == [files.img_id(i) for i in range(4) for _ in range(slots)]
    assert one["variants"] == list(ops.DIS_VARIANTS) and one["metrics"] == ["bev", "3d"] and one["classes"] == ["Car", "Pedestrian", "Cyclist"]
    n_bins = len(DI.DEFAULT_EDGES) - 1
    assert one["mean_iou"].shape == (3, n_bins + 1, R.NV, R.NMETRIC) and same_bits(one["thresholds"], H.thresholds())
    for v in range(R.NV):                                                        # every labelled object once per variant and metric
        for k in range(R.NMETRIC):
            assert int(one["count"][:, -1, v, k].sum() + one["nonfinite"][:, -1, v, k].sum() + one["outside"].sum()) == world["labelled"]
    assert one["count"][:, -1, R.FULL].sum() > 0 and one["count"][:, -1, R.NV - 1].sum() == 0        # no GMW: the variant is NaN
    assert "depth:oracle" in text1 and "orient" in text1 and all(c in text1 for c in files.classes)
    print(text1)
    # the loop spelled out by hand with the ops, one image at a time
    spec = model.heads.post_processor.decode_spec()
    table, outside = ops.dis_iou_tables(3, n_bins, pipe.device)
    model.eval()
    with torch.no_grad():
        for i in range(len(files)):
            images, targets = pipe([files.frame(i)], [files.sample(i)], img_ids=[files.img_id(i)])
            feats = model.backbone(images)
            centers = stack_field(targets, "target_centers")
            xs, ys = centers[:, :, 0], centers[:, :, 1]
            lin = ys.long() * feats.shape[3] + xs.long()
            vectors = model.heads.predictor.heads_at(feats, targets, lin)
            gt = torch.cat((stack_field(targets, "offset_3D"), stack_field(targets, "locations"), stack_field(targets, "dimensions"),
                            stack_field(targets, "rotys").unsqueeze(-1)), dim=2)
            dis = ops.dis_iou_estimates(vectors, ys, xs, stack_field(targets, "cls_ids"), gt, stack_field(targets, "reg_mask"),
                                        model.heads.post_processor._image_table(targets, pipe.device), spec)
            assert same_bits(_np(dis), one["dis"][i * slots:(i + 1) * slots])
            ops.dis_iou_accumulate(dis, DI.DEFAULT_EDGES, H.thresholds(), table, outside)
    by_hand = DI.summarise(_np(table), _np(outside), DI.DEFAULT_EDGES, one["classes"], H.thresholds())
    for k in ARRAYS:
        assert same_bits(by_hand[k], one[k]), k
    want, want_out = R.tables_of(one["dis"], DI.DEFAULT_EDGES, H.thresholds(), 3)
    assert same_bits(_np(table), want) and np.array_equal(_np(outside), want_out)


def test_gmw_fills_its_variant_and_moves_nothing_else(world):  # noqa: F811
    from dcd_amd.engine.dis_iou_report import dis_iou_report
    _, plain = dis_iou_report(world["model"], world["files"], world["pipe"], batch_size=2, per_object=True)
    _, with_gmw = dis_iou_report(world["model"], world["files"], world["pipe"], batch_size=2, gmw=world["gmw"], gmw_batch=48, per_object=True)
    on = plain["dis"][:, 0] != 0
    gm = [3 + R.NV - 1, 3 + 2 * R.NV - 1]
    keep = [c for c in range(R.ROW) if c not in gm]
    assert on.sum() == world["labelled"] and world["gmw"].training is False
    assert np.isnan(plain["dis"][on][:, gm]).all() and np.isfinite(with_gmw["dis"][on][:, gm]).all() and (with_gmw["dis"][~on] == 0).all()
    assert same_bits(with_gmw["dis"][:, keep], plain["dis"][:, keep])
    for k in ("mean_iou", "hit_rate", "hit_rate_loose", "count", "nonfinite"):
        assert same_bits(with_gmw[k][:, :, :R.NV - 1], plain[k][:, :, :R.NV - 1]), k
    assert same_bits(with_gmw["outside"], plain["outside"])
    assert with_gmw["count"][:, -1, R.NV - 1, 0].sum() + with_gmw["outside"].sum() == world["labelled"]


def test_refusals_and_the_command_line(world, tmp_path):  # noqa: F811
    import shutil
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.dis_iou_report import dis_iou_report
    from dcd_amd.engine.train import save_checkpoint
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    root = str(tmp_path / "testing")
    for d in ("ImageSets", "calib", "image_2"):
        shutil.copytree(os.path.join(world["root"], d), os.path.join(root, d))
    shutil.copy(os.path.join(root, "ImageSets", "train.txt"), os.path.join(root, "ImageSets", "test.txt"))
    files = KittiFiles(root, "test", world["cfg"], is_train=False)
    assert not files.has_labels
    with pytest.raises(ValueError, match="label"):
        dis_iou_report(world["model"], files, world["pipe"], batch_size=2)
    with pytest.raises(ValueError, match="is_train"):
        dis_iou_report(world["model"], world["files"], DeviceInputPipeline(world["cfg"], world["pipe"].device, is_train=True), batch_size=2)
    with pytest.raises(ValueError, match="edges"):
        dis_iou_report(world["model"], world["files"], world["pipe"], edges=(0, 20, 10))
    with pytest.raises(ValueError, match="thresholds"):
        dis_iou_report(world["model"], world["files"], world["pipe"], thresholds=np.full((3, 2, 2), 1.5))
    optimizer = build_optimizer(world["model"], world["cfg"])
    scheduler, _ = build_scheduler(optimizer, world["cfg"])
    ckpt = save_checkpoint(str(tmp_path / "ckpt"), "model_final", world["model"], optimizer, scheduler, {"iteration": 1})
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "dcd_amd.engine.dis_iou_report", "--root", world["root"], "--split", "train", "--ckpt", ckpt,
           "--output-dir", out, "--batch", "3", "--edges", "0", "20", "40", "80"] + [str(v) for v in OPTS]
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "0-20" in done.stdout and "depth:oracle" in done.stdout and "mean IoU" in done.stdout
    back = json.load(open(os.path.join(out, "dis_iou_report.json")))
    assert back["edges"] == [0.0, 20.0, 40.0, 80.0] and np.asarray(back["count"]).shape == (3, 4, R.NV, R.NMETRIC)
    _, here = dis_iou_report(world["model"], world["files"], world["pipe"], batch_size=1, edges=(0, 20, 40, 80))
    assert np.array_equal(np.asarray(back["count"]), here["count"]) and open(os.path.join(out, "dis_iou_report.txt")).read() in done.stdout
