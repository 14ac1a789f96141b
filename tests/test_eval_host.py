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


# ---- the tie fixture (tests/golden/make_golden_eval_ties.py): the derivation of csrc/eval.hip's comment, rule by rule ---------
TIES = EF.load("eval_ties.npz")
RAND_PAIRS = [(int(m), float(mo)) for m, mo in TIES["rand_comb"]]


def check_hand_cases(evaluator_cls):
    """Every hand-made case through `evaluator_cls` as the device test runs it; returns the names of the cases whose mode-A
    array or mode-B table differs from the recorded one."""
    cases = EF.ties_cases("hand")
    wrong = set()
    pairs = sorted({(c["metric"], c["min_overlap"]) for c in cases})
    rows = EF.ties_mode_a(evaluator_cls(), lambda o: o, cases, pairs)
    for c, per_comb in zip(cases, rows):
        got = per_comb[pairs.index((c["metric"], c["min_overlap"]))]
        if not np.array_equal(got, c["a"]):
            wrong.add(c["name"])
    for c in cases:
        counts, sim = EF.ties_mode_b(evaluator_cls(), lambda o: o, [c], [(c["metric"], c["min_overlap"])], c["thr"])
        if not np.array_equal(counts[0], c["b"][:, :3]):
            wrong.add(c["name"])
        elif c["metric"] == 0 and not np.allclose(sim[0], c["b"][:, 3], rtol=1e-9, atol=0):
            wrong.add(c["name"])
    return wrong


def test_emulated_evaluator_reproduces_the_tie_fixture():
    """The arg-max form against the reference's scan on every hand-made case and on 200 quantised images x 4 combinations x
    (mode A + 4 thresholds), image by image."""
    assert check_hand_cases(EF.EmulatedEvaluator) == set()
    cases = EF.ties_cases("rand")
    assert len(cases) == 200 and 2 * int(TIES["rand_tied_images"]) > len(cases)
    rows = EF.ties_mode_a(EF.EmulatedEvaluator(), lambda o: o, cases, RAND_PAIRS)
    for c, per_comb in zip(cases, rows):
        for m in range(len(RAND_PAIRS)):
            assert np.array_equal(per_comb[m], c["a"][m]), (c["name"], m)
    for c in cases:
        counts, sim = EF.ties_mode_b(EF.EmulatedEvaluator(), lambda o: o, [c], RAND_PAIRS, TIES["rand_thr"])
        assert np.array_equal(counts, c["b"][..., :3]), c["name"]
        np.testing.assert_allclose(sim, c["b"][[m for m, p in enumerate(RAND_PAIRS) if p[0] == 0], :, 3], rtol=1e-9, atol=0)


class RuleEvaluator(EF.EmulatedEvaluator):
    """The assignment once more with one rule switchable to a plausible wrong one (`rule`; None: all rules right)."""
    rule = None

    def _match(self, i, overlaps, metric, row, min_overlap, thresh, fp_mode, aos):
        p, f, rule = self.p, self.f, self.rule
        g0, g1, d0, d1 = p["gt_off"][i], p["gt_off"][i + 1], p["dt_off"][i], p["dt_off"][i + 1]
        ng, nd = g1 - g0, d1 - d0
        ig, idt, score = f["gt"][row, g0:g1], f["dt"][row, d0:d1], p["dt_score"][d0:d1]
        ov = overlaps[metric, p["pair_off"][i]:p["pair_off"][i] + nd * ng].reshape(nd, ng)
        below = (score <= thresh) if rule == "score_equal_to_thresh_dropped" else (score < thresh)
        live = (idt != -1) & ~(below if fp_mode else np.zeros(nd, bool))
        used = np.zeros(nd, bool)

        def greatest(idx, val, last_of_equals):
            return idx[len(idx) - 1 - np.argmax(val[::-1])] if last_of_equals else idx[np.argmax(val)]
        tp = fn = 0
        sim, matched = 0.0, np.full(ng, -1e7)
        for g in range(ng):
            if ig[g] == -1:
                continue
            over = (ov[:, g] >= min_overlap) if rule == "overlap_equal_to_min_overlap_accepted" else (ov[:, g] > min_overlap)
            cand = np.flatnonzero(live & ~used & over)
            det = -1
            if not fp_mode:
                cand = cand[score[cand] > -1e7]
                if len(cand):
                    det = greatest(cand, score[cand], rule == "highest_index_among_equal_scores")
            else:
                valid, ignored = cand[idt[cand] == 0], cand[idt[cand] == 1]
                if len(valid):
                    det = greatest(valid, ov[valid, g], rule == "highest_index_among_equal_overlaps")
                    if rule == "ignored_pick_kept_against_smaller_valid" and len(ignored) and ignored[0] < valid[0] \
                            and ov[ignored[0], g] >= ov[valid, g].max():
                        det = ignored[0]
                elif len(ignored):
                    det = ignored[np.argmax(ov[ignored, g])] if rule == "best_ignored_instead_of_first" else ignored[0]
            if det < 0:
                fn += int(ig[g] == 0)
                continue
            if not (rule == "ignored_gt_does_not_consume" and ig[g] == 1):
                used[det] = True
            if ig[g] == 1 or idt[det] == 1:
                continue
            tp += 1
            matched[g] = score[det]
            if aos:
                sim += (1.0 + np.cos(p["gt_alpha"][g0 + g] - p["dt_alpha"][d0 + det])) / 2.0
        fp = 0
        if fp_mode:
            dcs = p["dc_box"][p["dc_off"][i]:p["dc_off"][i + 1]]
            for d in np.flatnonzero((idt == 0) & ~used & ~below):
                inside = sum(EF.box_overlap_2d(p["dt_box2d"][d0 + d], q, 0) > min_overlap for q in dcs) if metric == 0 else 0
                fp += 1 - (inside if rule == "dontcare_subtracted_per_box" else min(inside, 1))
        return tp, fp, fn, sim, matched


def rule_evaluator(rule):
    return type("RuleEvaluator_%s" % rule, (RuleEvaluator,), {"rule": rule})


def test_rule_evaluator_with_every_rule_right_reproduces_the_fixture():
    assert check_hand_cases(rule_evaluator(None)) == set()


@pytest.mark.parametrize("rule, caught_by", [
    ("highest_index_among_equal_scores", {"a_equal_scores_adjacent", "a_equal_scores_63_64", "a_equal_scores_same_lane"}),
    ("highest_index_among_equal_overlaps", {"b_equal_overlaps_adjacent", "b_equal_overlaps_63_64", "b_equal_overlaps_same_lane"}),
    ("best_ignored_instead_of_first", {"b_only_ignored_first_wins", "b_only_ignored_first_block1_better_block2_lane0",
                                       "b_only_ignored_first_block0_better_block1_lane0"}),
    ("ignored_pick_kept_against_smaller_valid", {"b_ignored_then_valid_of_smaller_overlap"}),
    ("score_equal_to_thresh_dropped", {"score_equals_thresh"}),
    ("overlap_equal_to_min_overlap_accepted", {"overlap_equals_min_overlap_07", "overlap_equals_min_overlap_05"}),
    ("ignored_gt_does_not_consume", {"ignored_gt_absorbs_the_only_candidate"}),
    ("dontcare_subtracted_per_box", {"dontcare_two_boxes_counted_once"}),
])
def test_the_tie_fixture_catches_each_wrong_rule(rule, caught_by):
    """A wrong rule changes a recorded number of the hand-made cases named for it (and may change others)."""
    wrong = check_hand_cases(rule_evaluator(rule))
    assert caught_by <= wrong, (rule, sorted(wrong))


def test_get_thresholds_on_tied_score_arrays():
    scene = EF.ties_scene()
    tied = 0
    for n in range(N_COMB):
        scores = scene["comb_%d_scores" % n]
        got = kitti_ap.get_thresholds(scores, int(scene["comb_%d_num_gt" % n]))
        want = scene["comb_%d_thresholds" % n]
        assert len(got) == len(want) and all(a == b for a, b in zip(got, want)), n
        tied += len(np.unique(scores)) < len(scores)
    assert tied == int(scene["tied_combinations"]) >= 10


def test_host_pipeline_with_emulated_kernels_on_the_scene_with_duplicate_scores(monkeypatch):
    scene = EF.ties_scene()
    ids = [str(s) for s in scene["ids"]]
    gt = kitti_annos.read_annos(os.path.join(EF.TIES_SCENE_DIR, "label_2"), ids)
    dt = kitti_annos.read_annos(os.path.join(EF.TIES_SCENE_DIR, "pred"), ids)
    assert len(gt) == 8 and int(scene["dup_images"]) >= 3
    dup = sum(len(set(zip(d["name"].tolist(), d["score"].tolist()))) < len(d["name"]) for d in dt)
    assert dup == int(scene["dup_images"])
    monkeypatch.setattr(kitti_ap, "KittiEvaluator", EF.EmulatedEvaluator)
    stages = {}
    text, ret = kitti_ap.official_eval(gt, dt, [0, 1, 2], metric="R40", device="cpu", stages=stages)
    assert text == str(scene["text_R40"])
    for n in range(N_COMB):
        assert np.array_equal(np.sort(stages["scores"][n]), scene["comb_%d_scores" % n]), n
        pr = scene["comb_%d_pr" % n]
        assert np.array_equal(stages["counts"][n, :len(pr)], pr[:, :3]), n
