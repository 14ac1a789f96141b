"""The disentangled IoU report's arithmetic (csrc/dis_iou_math.h) compiled for the HOST (tests/host/host_dis_iou.cpp: the two
kernels of csrc/dis_iou.hip in plain loops) against the float64 restatement of tests/dis_iou_refs.py, on the candidates of
test_decode_host on which every clamp of the decode occurs (2 images x 16 slots, 73 key points, 24 x 80 maps) with labels seeded
around the predictions.  The GPU build of the same header is checked in test_gpu_dis_iou.py, which takes its helpers from here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dis_iou_refs as R  # noqa: E402
import test_decode_host as DH  # noqa: E402
import test_depth_report_host as RH  # noqa: E402
from test_decode_host import host_decode  # noqa: E402,F401  (the fixture: the host build of the decode, for the bit checks)
from test_depth_report_host import same_bits  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N = DH.BRANCH_B * DH.BRANCH_K
NUM_CLASSES = 3
EDGES_SMALL = (0.0, 10.0, 30.0, 80.0)
LABEL_SEED = 1                        # chosen on the CPU: no decision of the restatement within MARGIN of a threshold (the cap is 2 %)
MARGIN = 1e-4
EMPTY = (2, 17, 30)                   # slots without an object; the vector of slot 17 is NaN throughout and must never be read


def thresholds(num_classes=NUM_CLASSES):
    """(num_classes, 2, 2): per class and metric (bev, 3d) the strict and the loose threshold of `eval.kitti_ap.MIN_OVERLAPS`."""
    from dcd_amd.eval.kitti_ap import MIN_OVERLAPS
    return np.array([[[MIN_OVERLAPS[0, 1 + k, c], MIN_OVERLAPS[1, 1 + k, c]] for k in range(2)] for c in range(num_classes)], np.float64)


@pytest.fixture(scope="module")
def host_dis(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_dis_iou") / "libhost_dis_iou.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_dis_iou.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _flat(t, dtype=np.float32):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a.reshape(-1).astype(dtype))


def report_inputs(pp, device="cpu", seed=LABEL_SEED):
    """dict(vectors (2, 16, C), ys, xs, classes, gt (32, 9), gmw_z (32), valid (32) u8, table (2, 16), spec, targets, topk, clean):
    the branch candidates, the seeded labels, three empty slots, one of them with a NaN vector (`clean`: the vectors without it)."""
    vectors, topk, targets = DH.branch_inputs(pp, device)
    ys, xs, classes = RH.slots_of(topk)
    table = pp._image_table(targets, device)
    spec = pp.decode_spec()
    gt, gmw_z = R.seeded_labels(spec, vectors.cpu().numpy(), ys.cpu().numpy(), xs.cpu().numpy(), classes.cpu().numpy(), table.cpu().numpy(), seed)
    valid = np.ones(N, np.uint8)
    valid[list(EMPTY)] = 0
    broken = vectors.clone()
    broken.view(N, -1)[EMPTY[1]] = float("nan")
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return dict(vectors=broken, clean=vectors, ys=ys, xs=xs, classes=classes, gt=t(gt), gmw_z=t(gmw_z), valid=t(valid), table=table,
                spec=spec, targets=targets, topk=topk)


def restatement(inp, gmw=True):
    """(boxes (32, 16, 7) float64, rows (32, 33) float64 of the exact overlaps of those boxes rounded to float32, decodes)."""
    a = lambda k: inp[k].detach().cpu().numpy()  # noqa: E731
    boxes, decs = R.boxes_of(inp["spec"], a("vectors"), a("ys"), a("xs"), a("classes"), a("gt"), a("valid"), a("table"),
                             a("gmw_z") if gmw else None)
    return boxes, R.rows_of(boxes.astype(np.float32), a("classes"), a("valid")), decs


def host_estimates(lib, inp, gmw=True, want_boxes=True, vectors=None, change_args=None, spec=None, null=()):
    """`ops.dis_iou_estimates` on host arrays through the host build: (status, dis (32, 33), boxes (32, 16, 7)); outputs start as -7."""
    from dcd_amd import ops
    vectors = inp["vectors"] if vectors is None else vectors
    B, M, C = vectors.shape
    vec = np.ascontiguousarray(vectors.detach().cpu().float().numpy().reshape(B * M, C))
    a = ops.decode_args(spec or inp["spec"], B, M, C)
    if change_args is not None:
        change_args(a)
    dis, boxes = np.full((B * M, R.ROW), -7.0, np.float32), np.full((B * M, R.NBOX, R.BOX), -7.0, np.float32)
    arrays = dict(vectors=vec, ys=_flat(inp["ys"]), xs=_flat(inp["xs"]), classes=_flat(inp["classes"]), gt=_flat(inp["gt"]),
                  valid=_flat(inp["valid"], np.uint8), table=_flat(inp["table"]), gmw_z=_flat(inp["gmw_z"]) if gmw else None)
    ptrs = [None if k in null else _p(v) for k, v in arrays.items()]
    st = lib.host_dis_iou_estimates(*ptrs, ctypes.byref(a), None if "dis" in null else _p(dis), _p(boxes) if want_boxes else None)
    return st, dis, boxes


def host_accumulate(lib, dis, edges, thr, num_classes, tables=None):
    """`ops.dis_iou_accumulate` through the host build, onto `tables` = (table, outside) or fresh zeros: (status, table, outside)."""
    n_bins = len(edges) - 1
    table, outside = tables if tables is not None else (np.zeros((num_classes, max(n_bins, 0), R.NV, R.NMETRIC, R.STATS), np.float64),
                                                        np.zeros(num_classes, np.int64))
    dis = np.ascontiguousarray(dis, dtype=np.float32)
    e, t = np.asarray(edges, np.float32), np.ascontiguousarray(thr, dtype=np.float64)
    st = lib.host_dis_iou_accumulate(_p(dis), int(dis.shape[0]), _p(e), n_bins, num_classes, _p(t), _p(table), _p(outside))
    return st, table, outside


def chain_boxes(pp, inp):
    """The sixteen boxes from the existing torch fp32 chain on the CPU -- `PostProcessor.forward_batch` for `full`,
    `anno_encoder.decode_location_flatten`, `decode_dimension`, `decode_axes_orientation` and the depth report's chain estimates for
    the rest -- on the clean vectors: (32, 16, 7) float32, the yardstick of the box comparison."""
    from dcd_amd.structures.params_3d import stack_field
    enc, sl = pp.anno_encoder, pp.key2channel
    vectors, topk, targets = inp["clean"].cpu(), tuple(t.cpu() for t in inp["topk"]), [t.to("cpu") for t in inp["targets"]]
    B, K, C = vectors.shape
    vec = vectors.reshape(B * K, C)
    gt, gmw_z = inp["gt"].cpu(), inp["gmw_z"].cpu()
    image_of = torch.arange(B).repeat_interleave(K)
    calibs, pad = [t.get_field("calib") for t in targets], stack_field(targets, "pad_size")
    ys, xs, classes = RH.slots_of(topk)
    centres = torch.stack((xs.reshape(-1), ys.reshape(-1)), dim=1).float()
    with torch.no_grad():
        rows, _, _ = DH.chain_on_candidates(pp, vectors, topk, targets)
        est, best = RH.chain_estimates(pp, vectors, topk, targets)
        dims = enc.decode_dimension(classes.reshape(-1), vec[:, sl('3d_dim')])             # (l, h, w)
        four = torch.stack([torch.from_numpy(est[m]).float() for m in range(4)], dim=1)
        mean = (((four[:, 0] + four[:, 1]) + four[:, 2]) + four[:, 3]) / 4
        oracle = four.gather(1, (four.double() - gt[:, 4:5].double()).abs().argmin(dim=1, keepdim=True)).squeeze(1)
        methods = [four[:, 0], four[:, 1], four[:, 2], four[:, 3], torch.from_numpy(est[RH.SOFT]).float(),
                   torch.from_numpy(est[RH.HARD]).float(), mean, rows[:, 11], oracle, gmw_z]
        locate = lambda off, depth: enc.decode_location_flatten(centres, off, depth, calibs, pad, image_of)  # noqa: E731
        gl, gh, gw = gt[:, 5], gt[:, 6], gt[:, 7]
        label = torch.stack((gh, gw, gl, gt[:, 2], gt[:, 3] + gh / 2, gt[:, 4], gt[:, 8]), dim=1)
        out = label.unsqueeze(1).repeat(1, R.NBOX, 1)
        out[:, 1 + R.FULL] = rows[:, 6:13]
        at_edge = locate(vec[:, sl('3d_offset')], rows[:, 11])
        out[:, 1 + R.LOCATION, 3:6] = at_edge + torch.stack((0 * gh, gh / 2, 0 * gh), dim=1)
        at_gt = locate(vec[:, sl('3d_offset')], gt[:, 4])
        out[:, 1 + R.OFFSET, 3:6] = at_gt + torch.stack((0 * gh, gh / 2, 0 * gh), dim=1)
        out[:, 1 + R.DIMS, 0], out[:, 1 + R.DIMS, 1], out[:, 1 + R.DIMS, 2] = dims[:, 1], dims[:, 2], dims[:, 0]
        out[:, 1 + R.DIMS, 4] = gt[:, 3] + dims[:, 1] / 2
        ori = torch.cat((vec[:, sl('ori_cls')], vec[:, sl('ori_offset')]), dim=1)
        out[:, 1 + R.ORIENT, 6] = enc.decode_axes_orientation(ori, gt[:, 2:5].contiguous())[0].reshape(-1)
        for m, d in enumerate(methods):
            out[:, 1 + R.DEPTH0 + m, 3:6] = locate(gt[:, 0:2], d) + torch.stack((0 * gh, gh / 2, 0 * gh), dim=1)
    return out.numpy()


def column_distance(got, want, on):
    """Per box column: the largest |got - want| over the valid slots' sixteen boxes, as a fraction of the column's largest finite
    magnitude in `want`; the finite / non-finite pattern must be the same."""
    got, want = np.asarray(got, np.float64)[on], np.asarray(want, np.float64)[on]
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), "the finite / non-finite pattern differs"
    scale = np.where(finite, np.abs(want), 0).max(axis=(0, 1))
    return np.where(finite, np.abs(got - want), 0).max(axis=(0, 1)) / scale


def check_overlaps_against_own_boxes(dis, boxes, classes, valid, what):
    """Every overlap within 1e-6 of the exact float64 clip of the build's OWN boxes; the same non-finite pattern."""
    own = R.rows_of(boxes, _flat(classes), _flat(valid, np.uint8))
    assert np.array_equal(np.isfinite(dis), np.isfinite(own))
    err = np.nanmax(np.abs(dis.astype(np.float64) - own))
    print("%s: overlaps %.2e from the exact clip of its own boxes" % (what, err))
    assert err <= 1e-6, err
    return own


def check_hit_decisions(dis, ref_rows, classes, valid, thr, what):
    """Exactly the restatement's decisions wherever its float64 IoU is more than MARGIN from the threshold; at most 2 % of the
    decisions are left out (asserted on the restatement alone), and every variant has a hit and a miss at some threshold."""
    on = _flat(valid, np.uint8) != 0
    t = thr[_flat(classes).astype(int)][on]                                      # (n, metric, 2)
    want = ref_rows[on, 3:].reshape(-1, R.NMETRIC, R.NV)[..., None]
    got = dis[on, 3:].astype(np.float64).reshape(-1, R.NMETRIC, R.NV)[..., None]
    t = t[:, :, None, :]
    finite = np.broadcast_to(np.isfinite(want), np.broadcast_shapes(want.shape, t.shape))
    judged = finite & (np.abs(want - t) > MARGIN)
    share = 1.0 - judged.sum() / max(finite.sum(), 1)
    print("%s: %.2f %% of the decisions within %g of a threshold" % (what, 100 * share, MARGIN))
    assert share <= 0.02
    hit, miss = (want > t) & finite, ~(want > t) & finite
    assert hit.any(axis=(0, 1, 3)).all() and miss.any(axis=(0, 1, 3)).all(), "a variant without a hit or without a miss"
    assert np.array_equal((got > t)[judged], (want > t)[judged])


def check_tables(table, outside, dis, edges, thr, num_classes):
    want, want_out = R.tables_of(dis, edges, thr, num_classes)
    np.testing.assert_array_equal(outside, want_out)
    for stat in (0, 3, 4, 5):
        np.testing.assert_array_equal(table[..., stat], want[..., stat])
    assert same_bits(table, want), "the sums are not the slot-order double sums"
    return want, want_out


# ------------------------------------------------------------------------------------------------------------------ tests
def test_boxes_against_the_restatement_on_the_chains_scale(cpu_backend, host_dis, host_decode):  # noqa: F811
    """Per box column, as a fraction of the column's largest finite magnitude, on the 29 valid slots' sixteen boxes.  Measured
    (h w l x y z ry): the torch fp32 chain 5.72e-08 6.97e-08 3.28e-08 1.31e-07 8.80e-08 8.76e-08 1.64e-07 from the restatement, the
    host build 5.72e-08 6.97e-08 3.28e-08 1.31e-07 8.80e-08 8.76e-08 1.46e-07; the bar is 4 x the chain's distance per column."""
    pp = DH.branch_post_processor("cpu")
    inp = report_inputs(pp)
    on = _flat(inp["valid"], np.uint8) != 0
    ref_boxes, _, _ = restatement(inp)
    st, dis, boxes = host_estimates(host_dis, inp)
    assert st == 0
    chain = column_distance(chain_boxes(pp, inp), ref_boxes, on)
    host = column_distance(boxes, ref_boxes, on)
    print("the chain from the restatement, per column: %s" % np.array2string(chain, precision=2))
    print("the host build from the restatement:        %s" % np.array2string(host, precision=2))
    assert (chain > 0).all() and (chain < 1e-5).all()
    assert (host <= 4 * chain).all(), (host, chain)
    # leading columns, empty slots
    assert same_bits(dis[~on], np.zeros_like(dis[~on])) and same_bits(boxes[~on], np.zeros_like(boxes[~on]))
    assert same_bits(dis[on, 0], np.ones(on.sum(), np.float32)) and same_bits(dis[on, 1], _flat(inp["classes"])[on])
    assert same_bits(dis[on, 2], _flat(inp["gt"]).reshape(N, 9)[on, 4])
    # `full` is the decode's row and `depth:edges` its depth, bit for bit (the same header functions in the same lane order)
    rows = DH.run_host(host_decode, inp["vectors"], inp["topk"], inp["table"], inp["spec"], records=False)[0]
    assert same_bits(boxes[on, 1 + R.FULL], rows[on, 6:13]) and same_bits(boxes[on, 1 + R.DEPTH0 + R.EDGES, 5], rows[on, 11])
    # boxes = null changes nothing else
    st, no_boxes, untouched = host_estimates(host_dis, inp, want_boxes=False)
    assert st == 0 and same_bits(no_boxes, dis) and (untouched == -7).all()


def test_overlaps_hits_and_nonfinite_rule(cpu_backend, host_dis):
    pp = DH.branch_post_processor("cpu")
    inp = report_inputs(pp)
    _, ref_rows, _ = restatement(inp)
    st, dis, boxes = host_estimates(host_dis, inp)
    assert st == 0
    check_overlaps_against_own_boxes(dis, boxes, inp["classes"], inp["valid"], "host build")
    check_hit_decisions(dis, ref_rows, inp["classes"], inp["valid"], thresholds(), "host build")
    on = _flat(inp["valid"], np.uint8) != 0
    assert np.isfinite(dis[on]).all()
    # without gmw_z the last variant is NaN in both metrics and nothing else moves
    st, plain, plain_boxes = host_estimates(host_dis, inp, gmw=False)
    gm = [3 + R.NV - 1, 3 + 2 * R.NV - 1]
    keep = [c for c in range(R.ROW) if c not in gm]
    assert st == 0 and np.isnan(plain[on][:, gm]).all() and same_bits(plain[:, keep], dis[:, keep])
    assert np.isnan(plain_boxes[on, R.NBOX - 1, 5]).all() and same_bits(plain_boxes[:, :R.NBOX - 1], boxes[:, :R.NBOX - 1])


def test_tables_are_the_slot_order_sums_however_the_slots_are_cut(cpu_backend, host_dis):
    pp = DH.branch_post_processor("cpu")
    inp = report_inputs(pp)
    thr = thresholds()
    st, dis, _ = host_estimates(host_dis, inp, gmw=False)
    assert st == 0
    on = np.nonzero(dis[:, 0])[0]
    # planted depths: on the edge 10 (the upper bin), below the first edge, above the last, and a NaN
    dis = dis.copy()
    planted = dict(on_10=on[0], below=on[1], above=on[2], nan=on[3])
    dis[planted["on_10"], 2], dis[planted["below"], 2], dis[planted["above"], 2], dis[planted["nan"], 2] = 10.0, -1.0, 80.0, np.nan
    st, whole, whole_out = host_accumulate(host_dis, dis, EDGES_SMALL, thr, NUM_CLASSES)
    assert st == 0
    check_tables(whole, whole_out, dis, EDGES_SMALL, thr, NUM_CLASSES)
    for step in (32, 16, 1):
        tables = None
        for s in range(0, N, step):
            st, t, o = host_accumulate(host_dis, dis[s:s + step], EDGES_SMALL, thr, NUM_CLASSES, tables)
            assert st == 0
            tables = (t, o)
        assert same_bits(tables[0], whole) and same_bits(tables[1], whole_out), step
    alone = host_accumulate(host_dis, dis[planted["on_10"]][None], EDGES_SMALL, thr, NUM_CLASSES)
    c = int(dis[planted["on_10"], 1])
    assert alone[1][c, 1, R.FULL, 0, [0, 5]].sum() == 1 and alone[1][c, 0].sum() == 0 and alone[2].sum() == 0, "gt_z = 10 belongs to [10, 30)"
    for key in ("below", "above", "nan"):
        st, t, o = host_accumulate(host_dis, dis[planted[key]][None], EDGES_SMALL, thr, NUM_CLASSES)
        assert st == 0 and not t.any() and o[int(dis[planted[key], 1])] == 1 and o.sum() == 1, key
    # every object once per variant and metric: counted, non-finite, or outside
    assert (whole[..., 0].sum(axis=(0, 1)) + whole[..., 5].sum(axis=(0, 1)) + whole_out.sum() == len(on)).all()
    assert whole[..., R.NV - 1, :, 0].sum() == 0 and whole[..., R.NV - 1, :, 5].sum() == 2 * (len(on) - whole_out.sum())
    assert (whole[..., 3] <= whole[..., 4]).all() and (whole[..., 4] <= whole[..., 0]).all() and whole[..., 3].sum() > 0


def test_a_nan_in_one_head_reaches_the_variants_that_read_it_and_no_other(cpu_backend, host_dis):
    """The edge solver's clamp (fmin / fmax) drops a NaN, as it does in the decode, so the all-pairs depth stays finite whatever
    head is broken: a NaN key point changes bits of `full`, `location` and `depth:edges` and makes nothing non-finite."""
    pp = DH.branch_post_processor("cpu")
    inp = report_inputs(pp)
    sl = pp.key2channel
    st, clean, clean_boxes = host_estimates(host_dis, inp)
    _, _, decs = restatement(inp)
    slot = 6
    assert slot not in EMPTY and st == 0
    D = R.DEPTH0
    hard = lambda which: {D + R.HARD} if decs[slot]["best"] in which else set()  # noqa: E731
    cases = {
        "offset": (sl('3d_offset').start, {R.FULL, R.LOCATION, R.OFFSET}),
        "length": (sl('3d_dim').start, {R.FULL, R.DIMS}),
        "height": (sl('3d_dim').start + 1, {R.FULL, R.DIMS, D + R.KPT_CENTER, D + R.KPT_02, D + R.KPT_13, D + R.SOFT, D + R.MEAN} | hard((1, 2, 3))),
        "orientation offset": (slice(sl('ori_offset').start, sl('ori_offset').stop), {R.FULL, R.ORIENT}),
        "depth": (sl('depth').start, {R.FULL, D + R.DIRECT, D + R.SOFT, D + R.MEAN} | hard((0,))),
        "key point": (sl('extra_kpts_2d').start + 2 * 7 + 1, set()),
    }
    others = np.arange(N) != slot
    for name, (channel, expect) in cases.items():
        broken = inp["vectors"].clone()
        broken.view(N, -1)[slot, channel] = float("nan")
        st, dis, boxes = host_estimates(host_dis, inp, vectors=broken)
        assert st == 0 and same_bits(dis[others], clean[others]) and same_bits(boxes[others], clean_boxes[others]), name
        for k in range(R.NMETRIC):
            bad = set(np.nonzero(~np.isfinite(dis[slot, 3 + k * R.NV:3 + (k + 1) * R.NV]))[0].tolist())
            assert bad == expect, (name, k, sorted(bad), sorted(expect))
        untouched = [3 + k * R.NV + v for k in range(R.NMETRIC) for v in (R.OFFSET, R.DIMS, R.ORIENT, D + R.GMW) if v not in expect]
        assert same_bits(dis[slot, untouched], clean[slot, untouched]), name
    z = (slot, 1 + D + R.EDGES, 5)                                                            # (the last case: the key point)
    assert np.isfinite(boxes[z]) and not same_bits(boxes[z], clean_boxes[z])


def test_host_build_refuses_what_the_entry_points_refuse(cpu_backend, host_dis):
    pp = DH.branch_post_processor("cpu")
    inp = report_inputs(pp)

    def refused(**k):
        st, dis, boxes = host_estimates(host_dis, inp, **k)
        return st == 1 and (dis == -7).all() and (boxes == -7).all()
    for name in ("vectors", "ys", "xs", "classes", "gt", "valid", "table", "dis"):
        assert refused(null=(name,)), name
    assert refused(spec=dict(inp["spec"], nk=1)) and refused(spec=dict(inp["spec"], nk=129))
    assert refused(change_args=lambda a: setattr(a, "K", 129))
    dis = np.zeros((4, R.ROW), np.float32)
    thr = thresholds()
    fresh = lambda: (np.full((8, 17, R.NV, R.NMETRIC, R.STATS), -7.0), np.full(9, -7, np.int64))  # noqa: E731
    bad_thr = thr.copy()
    bad_thr[1, 1, 0] = 1.5
    nine = np.full((9, 2, 2), 0.5)
    for edges, classes_n, t in (((0.0,), 3, thr), (np.arange(18.0), 3, thr), ((0.0, 10.0, 10.0), 3, thr), ((0.0, 30.0, 20.0), 3, thr),
                                ((0.0, 10.0), 9, nine), ((0.0, 10.0), 3, bad_thr), ((0.0, 10.0), 3, -bad_thr)):
        st, table, outside = host_accumulate(host_dis, dis, edges, t, classes_n, fresh())
        assert st == 1 and (table == -7).all() and (outside == -7).all(), (edges, classes_n)
    for null in range(3):
        table, outside = fresh()
        ptrs = [_p(dis), _p(table), _p(outside)]
        ptrs[null] = None
        e = np.asarray((0.0, 10.0), np.float32)
        st = host_dis.host_dis_iou_accumulate(ptrs[0], 4, _p(e), 1, 3, _p(thr), ptrs[1], ptrs[2])
        assert st == 1 and (table == -7).all() and (outside == -7).all()
    st, table, outside = host_accumulate(host_dis, dis, (0.0, 10.0), thr, 3, fresh())
    assert st == 0                                                                            # (the control: the same call, accepted)
