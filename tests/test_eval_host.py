"""Host stages of the KITTI evaluator against fixtures written by the reference's own evaluator
(tests/golden/make_golden_eval.py): file parsing and writing, ignore flags, thresholds, the table stage.  No GPU."""
import os

import numpy as np
import pytest

import eval_fixtures as EF
from dcd_amd.eval import kitti_annos, kitti_ap

SCENE = EF.load("eval_scene.npz")
N_COMB = 54                                  # 3 metrics x 3 classes x 3 difficulties x 2 overlap rows, in that loop order


def test_read_annos_equals_the_reference_parse():
    ids = EF.scene_ids()
    for prefix, folder in (("gt", "label_2"), ("dt", "pred")):
        got = kitti_annos.read_annos(os.path.join(EF.SCENE_DIR, folder), ids)
        want = EF.annos(SCENE, prefix)
        assert len(got) == len(want) == 16
        for a, b in zip(got, want):
            assert set(a) == set(EF.ANNO_KEYS)
            for k in EF.ANNO_KEYS:
                assert np.asarray(a[k]).shape == b[k].shape, k
                assert np.array_equal(np.asarray(a[k]), b[k]), k
    assert any(len(a["name"]) == 0 for a in EF.annos(SCENE, "gt")) and any(len(a["name"]) == 0 for a in EF.annos(SCENE, "dt"))
    missing = kitti_annos.read_annos(os.path.join(EF.SCENE_DIR, "label_2"), ["999999"])[0]     # no such file: empty annotation
    assert len(missing["name"]) == 0 and missing["bbox"].shape == (0, 4) and missing["score"].shape == (0,)


def test_write_detections_reproduces_the_prediction_files(tmp_path):
    empty = 0
    for i, img_id in enumerate(EF.scene_ids()):
        rows = SCENE["rows_%d" % i]
        path = str(tmp_path / (img_id + ".txt"))
        kitti_annos.write_detections(rows, path)
        with open(path, "rb") as f, open(os.path.join(EF.SCENE_DIR, "pred", img_id + ".txt"), "rb") as g:
            got, want = f.read(), g.read()
        assert got == want, img_id
        if len(rows) == 0:
            assert got == b"\n"
            empty += 1
    assert empty >= 1
    import torch
    kitti_annos.write_detections(torch.from_numpy(SCENE["rows_0"]), str(tmp_path / "t.txt"))     # tensors too
    with open(str(tmp_path / "t.txt"), "rb") as f, open(os.path.join(EF.SCENE_DIR, "pred", EF.scene_ids()[0] + ".txt"), "rb") as g:
        assert f.read() == g.read()


def test_ignore_flags_equal_clean_data():
    gt, dt = EF.annos(SCENE, "gt"), EF.annos(SCENE, "dt")
    flags = kitti_ap.ignore_flags(gt, dt, [0, 1, 2])
    packed = kitti_ap.pack(gt, dt, flags["dontcare"])
    seen = set()
    for c in range(3):
        for d in range(3):
            row = c * 3 + d
            assert np.array_equal(flags["gt"][row], SCENE["clean_%d_%d_gt" % (c, d)])
            assert np.array_equal(flags["dt"][row], SCENE["clean_%d_%d_dt" % (c, d)])
            assert flags["num_valid"][row] == SCENE["clean_%d_%d_num_valid" % (c, d)]
            assert np.array_equal(np.diff(packed["dc_off"]), SCENE["clean_%d_%d_dc_count" % (c, d)])
            seen |= set(flags["gt"][row].tolist())
    assert seen == {-1, 0, 1}
    # names straight from memory keep 'DontCare' (files are read through str.capitalize, which hides it: eval.py:66)
    big = EF.load("eval_pairs.npz")
    g, d = EF.annos(big, "gt")[2:3], EF.annos(big, "dt")[2:3]
    f = kitti_ap.ignore_flags(g, d, [0])
    assert np.array_equal(f["gt"][2], big["big_ignored_gt"]) and np.array_equal(f["dt"][2], big["big_ignored_dt"])
    assert f["dontcare"].sum() == (g[0]["name"] == "DontCare").sum() > 0


def test_get_thresholds_equals_the_reference():
    nonempty = 0
    for n in range(N_COMB):
        got = kitti_ap.get_thresholds(SCENE["comb_%d_scores" % n], int(SCENE["comb_%d_num_gt" % n]))
        want = SCENE["comb_%d_thresholds" % n]
        assert len(got) == len(want) and all(a == b for a, b in zip(got, want)), n
        nonempty += len(want) > 1
    assert nonempty >= 10


@pytest.mark.parametrize("metric", ["R40", "R11"])
def test_table_stage_reproduces_curves_and_text(metric):
    pr = [[SCENE["comb_%d_pr" % (m * 18 + i)] for i in range(18)] for m in range(3)]
    detail, curves = {}, []
    text, ret = kitti_ap.result_from_pr(pr, [0, 1, 2], metric, True, detail, curves)
    assert text == str(SCENE["text_" + metric])
    assert list(ret) == [str(k) for k in SCENE["dict_keys_" + metric]]
    assert np.array_equal(np.array([ret[k] for k in ret]), SCENE["dict_values_" + metric], equal_nan=True)
    for m in range(3):
        for k, name in enumerate(("precision", "recall", "orientation")):
            assert np.array_equal(curves[m][k], SCENE["%s_%d" % (name, m)], equal_nan=True), (m, name)
    for k in ("bbox", "aos", "bev", "3d"):
        assert np.array_equal(detail[k], SCENE["detail_" + k], equal_nan=True)


def test_evaluator_has_no_cpu_path():
    from dcd_amd import _lib
    with pytest.raises(_lib.DcdHipError):
        kitti_ap.KittiEvaluator("cpu")
    gt, dt = EF.annos(SCENE, "gt"), EF.annos(SCENE, "dt")
    with pytest.raises(_lib.DcdHipError):
        kitti_ap.official_eval(gt, dt, [0, 1, 2], device="cpu")


def test_host_pipeline_with_emulated_kernels(monkeypatch):
    """The whole of `official_eval` with the device stages replaced by their plain-Python statement (exact overlaps, arg-max
    assignment): identical text.  Pins the packing, the combination tables and the derivation the kernel's comment states."""
    monkeypatch.setattr(kitti_ap, "KittiEvaluator", EF.EmulatedEvaluator)
    gt, dt = EF.annos(SCENE, "gt"), EF.annos(SCENE, "dt")
    stages = {}
    text, ret = kitti_ap.official_eval(gt, dt, ["Car", "Pedestrian", "Cyclist"], metric="R40", device="cpu", stages=stages)
    assert text == str(SCENE["text_R40"])
    for n in range(N_COMB):
        assert np.array_equal(np.sort(stages["scores"][n]), SCENE["comb_%d_scores" % n]), n
        pr = SCENE["comb_%d_pr" % n]
        assert np.array_equal(stages["counts"][n, :len(pr)], pr[:, :3]), n
