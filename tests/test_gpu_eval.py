"""The KITTI evaluator's kernels (csrc/eval.hip) on the device: closed forms, the reference's stored overlaps and statistics
(tests/golden/make_golden_eval.py), the AP table end to end, and `inference()` from a KITTI directory."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_fixtures as EF  # noqa: E402
from dcd_amd import _lib  # noqa: E402
from dcd_amd.eval import kitti_annos, kitti_ap  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = EF.load("eval_pairs.npz")
SCENE = EF.load("eval_scene.npz")
N_COMB = 54


def anno(boxes3d, boxes2d, names=None, scores=None, alphas=None):
    """One image's annotation from rows (x, y, z, l, h, w, ry) and (x1, y1, x2, y2)."""
    b3, b2 = np.asarray(boxes3d, np.float64).reshape(-1, 7), np.asarray(boxes2d, np.float64).reshape(-1, 4)
    n = len(b3)
    a = dict(name=np.array(names if names is not None else ["Car"] * n, dtype="<U16"), truncated=np.zeros(n),
             occluded=np.zeros(n, np.int64), alpha=np.asarray(alphas if alphas is not None else np.zeros(n), np.float64),
             bbox=b2, dimensions=b3[:, 3:6], location=b3[:, 0:3], rotation_y=b3[:, 6])
    if scores is not None:
        a["score"] = np.asarray(scores, np.float64)
    return a


def loaded(cuda, gts, dts, classes=(0,)):
    flags = kitti_ap.ignore_flags(gts, dts, list(classes))
    ev = kitti_ap.KittiEvaluator(cuda)
    ev.load(kitti_ap.pack(gts, dts, flags["dontcare"]), flags)
    return ev, flags


def pair_overlaps(cuda, gt3, gt2, dt3, dt2):
    """(3,) overlaps of one detection with one ground-truth box, through dcd_eval_overlaps."""
    ev, _ = loaded(cuda, [anno([gt3], [gt2])], [anno([dt3], [dt2], scores=[0.5])])
    return ev.overlaps().cpu().numpy()[:, 0]


# ---- overlaps: closed forms ------------------------------------------------------------------------------------------
FOOT = (1.0, 2.0, 20.0, 4.0, 2.0, 2.0, 0.0)          # x y z l h w ry: x in [-1, 3], y in [0, 2], z in [19, 21]
BOX2 = (10.0, 20.0, 50.0, 40.0)


def moved(box, **kw):
    keys = ("x", "y", "z", "l", "h", "w", "ry")
    return tuple(kw.get(k, v) for k, v in zip(keys, box))


def test_identical_boxes_overlap_fully(cuda):
    for ry in (0.0, 0.3, -2.1):
        b = moved(FOOT, ry=ry)
        np.testing.assert_allclose(pair_overlaps(cuda, b, BOX2, b, BOX2), 1.0, atol=1e-6, rtol=0)


def test_disjoint_boxes_and_boxes_sharing_an_edge_overlap_zero(cuda):
    far = pair_overlaps(cuda, FOOT, BOX2, moved(FOOT, x=30.0, ry=0.7), (200.0, 20.0, 240.0, 40.0))
    assert (far == 0).all()
    # x extents [-1, 3] and [3, 7]: one common edge; the image boxes share the line x = 50
    edge = pair_overlaps(cuda, FOOT, BOX2, moved(FOOT, x=5.0), (50.0, 20.0, 90.0, 40.0))
    assert (edge == 0).all()


def test_box_inside_another_gives_the_ratio(cuda):
    inner = (1.0, 1.5, 20.0, 2.0, 1.0, 1.0, 0.0)        # y in [0.5, 1.5]
    got = pair_overlaps(cuda, FOOT, BOX2, inner, (20.0, 25.0, 40.0, 35.0))
    np.testing.assert_allclose(got, [200.0 / 800.0, 2.0 / 8.0, 2.0 / 16.0], atol=1e-6, rtol=0)
    assert got[0] == 0.25                                # float64 arithmetic on exact values


def test_quarter_turn_of_the_same_footprint_equals_the_axis_aligned_case(cuda):
    shifted = moved(FOOT, x=2.0, z=20.5)
    turned = moved(shifted, l=2.0, w=4.0, ry=math.pi / 2)    # the same rectangle on the ground
    a = pair_overlaps(cuda, FOOT, BOX2, shifted, BOX2)
    b = pair_overlaps(cuda, FOOT, BOX2, turned, BOX2)
    inter = 3.0 * 1.5
    np.testing.assert_allclose(a[1], inter / (16.0 - inter), atol=1e-6, rtol=0)
    np.testing.assert_allclose(b, a, atol=1e-6, rtol=0)
    np.testing.assert_allclose(pair_overlaps(cuda, FOOT, BOX2, moved(FOOT, l=2.0, w=4.0, ry=math.pi / 2), BOX2), 1.0, atol=1e-6,
                               rtol=0)


def test_crossed_bars_and_octagon(cuda):
    bar = (0.0, 2.0, 20.0, 6.0, 2.0, 2.0, 0.0)
    got = pair_overlaps(cuda, bar, BOX2, moved(bar, ry=math.pi / 2), BOX2)
    np.testing.assert_allclose(got[1:], [4.0 / 20.0, 8.0 / (24.0 + 24.0 - 8.0)], atol=1e-6, rtol=0)
    sq = (0.0, 1.0, 20.0, 1.0, 1.0, 1.0, 0.0)
    octagon = 2.0 * (math.sqrt(2.0) - 1.0)               # two unit squares at 45 degrees: 8 vertices, the cap exactly
    got = pair_overlaps(cuda, sq, BOX2, moved(sq, ry=math.pi / 4), BOX2)
    np.testing.assert_allclose(got[1:], [octagon / (2.0 - octagon)] * 2, atol=1e-6, rtol=0)


def test_partial_height_overlap(cuda):
    # y spans [0, 2] and [1, 3]: 1 m in common on the full 4 x 2 footprint -> 8 / (16 + 16 - 8); no common height -> 0
    got = pair_overlaps(cuda, FOOT, BOX2, moved(FOOT, y=3.0), BOX2)
    np.testing.assert_allclose(got[1:], [1.0, 1.0 / 3.0], atol=1e-6, rtol=0)
    assert pair_overlaps(cuda, FOOT, BOX2, moved(FOOT, y=4.5), BOX2)[2] == 0


def test_dontcare_overlap_through_mode_b(cuda):
    """A detection that covers a DontCare box with a quarter of its own area (criterion 0: intersection / detection area) is
    not a false positive while 0.25 > min_overlap -- strictly -- and only for the image-box metric."""
    gts = [anno([(-1000.0, -1000.0, -1000.0, -1.0, -1.0, -1.0, -10.0)], [(0.0, 0.0, 100.0, 100.0)], names=["DontCare"])]
    dts = [anno([FOOT], [(50.0, 50.0, 150.0, 150.0)], scores=[0.9])]
    ev, flags = loaded(cuda, gts, dts)
    assert ev.n_dc == 1 and flags["gt"][0, 0] == -1 and flags["dt"][0, 0] == 0
    comb = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, -1]], np.int32)
    mo = np.array([0.2, 0.25, 0.3, 0.2])
    counts, _ = ev.match_counts(ev.overlaps(), comb, mo, [np.array([0.0])] * 4, 0)
    assert counts[:, 0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0]]


# ---- overlaps against the reference and the exact value --------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs_run(cuda):
    gts, dts = EF.annos(PAIRS, "gt"), EF.annos(PAIRS, "dt")
    ev, flags = loaded(cuda, gts, dts)
    return ev, flags, ev.overlaps().cpu().numpy(), gts, dts


def test_overlaps_against_exact_and_reference(pairs_run):
    """Yardstick: the reference's own distance from the exact float64 intersection on these pairs, E_ref = 1.63e-5 (stored by
    the generator).  BEV: |kernel - exact| <= 4 E_ref; 3-D: |kernel - reference| <= 4 E_ref and |reference - exact| <= E_ref;
    image boxes, float64 arithmetic: 1e-12."""
    ev, _, got, gts, dts = pairs_run
    e_ref = float(PAIRS["E_ref"])
    assert 0 < e_ref < 1e-4
    assert ev.P == 24 * 30 + 130 * 70 and ev.P % 256 != 0
    off = kitti_ap.pack(gts, dts, np.zeros(ev.G, bool))["pair_off"]
    worst, overlapping = np.zeros(4), 0
    for i in (0, 2):
        blk = got[:, off[i]:off[i + 1]].reshape(3, len(dts[i]["name"]), len(gts[i]["name"]))
        worst[0] = max(worst[0], np.abs(blk[0] - PAIRS["ref_0_%d" % i]).max())
        worst[1] = max(worst[1], np.abs(blk[1] - PAIRS["exact_bev_%d" % i]).max())
        worst[2] = max(worst[2], np.abs(blk[2] - PAIRS["ref_2_%d" % i]).max())
        worst[3] = max(worst[3], np.abs(PAIRS["ref_2_%d" % i] - PAIRS["exact_3d_%d" % i]).max())
        # far apart: exactly zero
        d, g = dts[i], gts[i]
        gap = np.hypot(d["location"][:, None, 0] - g["location"][None, :, 0], d["location"][:, None, 2] - g["location"][None, :, 2])
        reach = (np.hypot(d["dimensions"][:, 0], d["dimensions"][:, 2])[:, None]
                 + np.hypot(g["dimensions"][:, 0], g["dimensions"][:, 2])[None]) / 2
        far = (PAIRS["exact_inter_%d" % i] == 0) & (gap > reach)
        assert far.sum() > 100 and (blk[1][far] == 0).all() and (blk[2][far] == 0).all()
        overlapping += int((PAIRS["exact_bev_%d" % i] > 0.3).sum())
    assert overlapping >= 20
    print("max |bbox - ref| %.3g, |bev - exact| %.3g, |3d - ref| %.3g, |ref 3d - exact| %.3g, E_ref %.3g" % (*worst, e_ref))
    assert worst[0] <= 1e-12
    assert worst[1] <= 4 * e_ref
    assert worst[2] <= 4 * e_ref
    assert worst[3] <= e_ref


def test_images_without_pairs_write_nothing(cuda):
    gts, dts = EF.annos(PAIRS, "gt"), EF.annos(PAIRS, "dt")
    ev, _ = loaded(cuda, [gts[1], gts[3], gts[4]], [dts[1], dts[3], dts[4]])
    assert ev.P == 0 and ev.G == 5 and ev.D == 7
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=cuda)
    t = ev.t
    status = ev.lib.dcd_eval_overlaps(_lib.stream_of(out), ev.n_img, _lib.ptr(t["gt_off"]), _lib.ptr(t["dt_off"]),
                                      _lib.ptr(t["pair_off"]), ev.G, ev.D, 0, _lib.ptr(t["gt_box2d"]), _lib.ptr(t["dt_box2d"]),
                                      _lib.ptr(t["gt_box3d"]), _lib.ptr(t["dt_box3d"]), _lib.ptr(out))
    torch.cuda.synchronize()
    assert status == 0 and bool(torch.isnan(out).all())
    # and the statistics of such images: every valid ground-truth box is a miss, every detection a false positive
    comb = np.array([[0, 0, -1]], np.int32)
    scores = ev.match_scores(ev.overlaps(), comb, np.array([0.5]))
    assert scores.shape == (1, 5) and (scores == kitti_ap.NO_DETECTION).all()
    counts, _ = ev.match_counts(ev.overlaps(), comb, np.array([0.5]), [np.array([0.0])], 0)
    flags = kitti_ap.ignore_flags([gts[1], gts[3], gts[4]], [dts[1], dts[3], dts[4]], [0])
    assert counts[0, 0].tolist() == [0, int((flags["dt"][0] == 0).sum()), int((flags["gt"][0] == 0).sum())]


# ---- matching ----------------------------------------------------------------------------------------------------------
def test_big_image_through_both_modes(cuda):
    """130 detections x 70 ground-truth boxes (three lane blocks, competing candidates, DontCare boxes), the reference's
    stored overlaps: class Car, difficulty hard, min overlap 0.5, five thresholds."""
    gts, dts = EF.annos(PAIRS, "gt")[2:3], EF.annos(PAIRS, "dt")[2:3]
    ev, flags = loaded(cuda, gts, dts)
    assert ev.D == 130 and ev.G == 70 and ev.n_dc > 0
    ovl = torch.from_numpy(np.stack([PAIRS["ref_%d_2" % m].ravel() for m in range(3)])).to(cuda)
    comb = np.array([[0, 2, 0], [1, 2, -1], [2, 2, -1]], np.int32)
    mo = np.full(3, 0.5)
    scores = ev.match_scores(ovl, comb, mo)
    thr = PAIRS["big_thresholds"]
    counts, sim = ev.match_counts(ovl, comb, mo, [thr] * 3, 1)
    for m in range(3):
        assert np.array_equal(np.sort(scores[m][scores[m] != kitti_ap.NO_DETECTION]), PAIRS["big_scores_%d" % m])
        want = PAIRS["big_pr_%d" % m]
        assert np.array_equal(counts[m], want[:, :3]), m
    want = np.where(PAIRS["big_pr_0"][:, 3] == -1, 0.0, PAIRS["big_pr_0"][:, 3])
    np.testing.assert_allclose(sim[0], want, rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def scene_annos():
    ids = EF.scene_ids()
    return (kitti_annos.read_annos(os.path.join(EF.SCENE_DIR, "label_2"), ids),
            kitti_annos.read_annos(os.path.join(EF.SCENE_DIR, "pred"), ids))


def test_scene_statistics_from_the_reference_overlaps(cuda, scene_annos):
    gts, dts = scene_annos
    ev, flags = loaded(cuda, gts, dts, (0, 1, 2))
    ovl = torch.from_numpy(EF.reference_overlaps(SCENE, 16)).to(cuda)
    stages = {}
    kitti_ap.pr_tables(ev, ovl, 3, True, kitti_ap.MIN_OVERLAPS[:, :, [0, 1, 2]], flags["num_valid"], stages)
    for n in range(N_COMB):
        assert np.array_equal(np.sort(stages["scores"][n]), SCENE["comb_%d_scores" % n]), n
        assert all(a == b for a, b in zip(stages["thresholds"][n], SCENE["comb_%d_thresholds" % n]))
        pr = SCENE["comb_%d_pr" % n]
        assert np.array_equal(stages["counts"][n, :len(pr)], pr[:, :3]), n
        assert (stages["counts"][n, len(pr):] == 0).all()
        if n < 18:
            np.testing.assert_allclose(stages["similarity"][n, :len(pr)], pr[:, 3], rtol=1e-9, atol=0)


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["R40", "R11"])
def test_official_eval_reproduces_the_reference_table(cuda, scene_annos, metric):
    """Identical text although the BEV overlaps are only within 4 E_ref of the exact value: the generator made sure that
    every overlap of the scene is at least 8 E_ref away from 0.7, 0.5 and 0.25."""
    gts, dts = scene_annos
    runs = []
    for _ in range(2):
        detail, stages = {}, {}
        text, ret = kitti_ap.official_eval(gts, dts, [0, 1, 2], metric=metric, device=cuda, detail=detail, stages=stages)
        runs.append((text, ret, detail, stages))
    text, ret, detail, stages = runs[0]
    assert text == str(SCENE["text_" + metric])
    assert list(ret) == [str(k) for k in SCENE["dict_keys_" + metric]]
    np.testing.assert_allclose(np.array([ret[k] for k in ret]), SCENE["dict_values_" + metric], rtol=1e-9, atol=1e-9)
    for m in range(3):
        for k, name in enumerate(("precision", "recall", "orientation")):
            np.testing.assert_allclose(stages["curves"][m][k], SCENE["%s_%d" % (name, m)], rtol=1e-9, atol=1e-9)
    for k in ("bbox", "aos", "bev", "3d"):
        np.testing.assert_allclose(detail[k], SCENE["detail_" + k], rtol=1e-9, atol=1e-9)
    # run to run: bit-equal, the floating-point similarity sums included
    again = runs[1]
    assert again[0] == text and all(np.array_equal(again[1][k], ret[k], equal_nan=True) for k in ret)
    assert np.array_equal(again[3]["similarity"], stages["similarity"]) and np.array_equal(again[3]["counts"], stages["counts"])
    for k in detail:
        assert np.array_equal(again[2][k], detail[k], equal_nan=True)
    # from the directories
    t2, r2 = kitti_ap.evaluate(os.path.join(EF.SCENE_DIR, "label_2"), os.path.join(EF.SCENE_DIR, "pred"),
                               os.path.join(EF.SCENE_DIR, "val.txt"), current_class=[0, 1, 2], metric=metric, device=cuda)
    assert t2 == text and all(np.array_equal(r2[k], ret[k], equal_nan=True) for k in ret)


def test_inference_from_a_kitti_directory(cuda, tmp_path):
    """The four-image fixture directory -> model in eval mode, one image per call -> result files -> AP dict.  No AP value
    is asserted: a model that is only initialised detects nothing useful."""
    import test_input_host as IH
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path, [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False])
    files = KittiFiles(root, "train", cfg, is_train=False)
    pipe = DeviceInputPipeline(cfg, cuda, is_train=False)
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    out = str(tmp_path / "out")
    result = inference(model, files, pipe, out, metrics=("R40", "R11"))
    ids = [files.img_id(i) for i in range(len(files))]
    assert len(ids) == 4 and sorted(os.listdir(os.path.join(out, "data"))) == [i + ".txt" for i in ids]
    # the files hold the rounded PostProcessor rows
    model.eval()
    dts = kitti_annos.read_annos(os.path.join(out, "data"), ids)
    with torch.no_grad():
        for i, d in enumerate(dts):
            images, targets = pipe([files.frame(i)], [files.sample(i)], img_ids=[ids[i]])
            rows = kitti_annos.rounded_rows(model(images, targets)[0]).astype(np.float64)
            assert len(d["name"]) == len(rows)
            if len(rows):
                assert [kitti_annos.ID_TYPE_CONVERSION[int(c)] for c in rows[:, 0]] == d["name"].tolist()
                got = np.concatenate([d["alpha"][:, None], d["bbox"], d["dimensions"][:, [1, 2, 0]], d["location"],
                                      d["rotation_y"][:, None], d["score"][:, None]], 1)
                np.testing.assert_array_equal(got, rows[:, 1:])
    gts = kitti_annos.read_annos(os.path.join(root, "label_2"), ids)
    assert set(result) == {"R40", "R11"}
    for metric in result:
        _, want = kitti_ap.official_eval(gts, dts, list(files.classes), metric=metric, device=cuda)
        assert list(result[metric]) == list(want)
        assert all(np.array_equal(result[metric][k], want[k], equal_nan=True) for k in want)
