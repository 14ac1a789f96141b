"""Generates the tie fixture of the KITTI matching kernel (eval_ties.npz, eval_scene_ties/) by RUNNING THE REFERENCE'S OWN
`compute_statistics_jit` and `get_official_eval_result` on the CPU, imported with the stubs of make_golden_eval.py.

Run in the build container only (`python tests/golden/make_golden_eval_ties.py`).  Nothing of the reference is copied; the
files written hold its recorded inputs and outputs only.  eval_pairs.npz and eval_scene.npz are read, never written.

The kernel takes the overlap matrix as an input, so a case needs no geometry: one [nd, ng] overlap matrix, the two flag
vectors, scores, both alpha vectors, the detections' image boxes, the DontCare boxes, the metric, min_overlap and a list of
thresholds.  Recorded per case: mode A (compute_fp = False), the returned score array in ground-truth order, unsorted; mode B
(compute_fp = True), (tp, fp, fn, similarity) per threshold with the reference's similarity -1 stored as 0.  compute_aos is
on for metric 0 and off otherwise, as in eval_class.

  hand_*   named cases, one rule each; every case is built so that the wrong rule changes a recorded NUMBER: a later
           ground-truth box can only be served by the detection the wrong rule would have used up.
  rand_*   N_RANDOM images with quantised values (overlaps k/8, scores k/10, integer image boxes), so that several ties occur
           in one image; every image is recorded under every combination of RAND_COMB and every threshold of RAND_THR.
           "Tie" below: for some ground-truth box with ignored_gt != -1 the greatest score among its candidates
           (ignored_det != -1, overlap > 0.5) is shared by two of them (score tie), resp. the greatest overlap among its
           candidates with ignored_det == 0 is shared by two of them (overlap tie).  Asserted: most images have both.
  scene_*  8 images of synthetic.make_scene with scores quantised to 0.05, written through the reference's own writer,
           evaluated by the reference end to end (what make_golden_eval.py records for eval_scene, under new names).  Re-seeded
           until three images hold a duplicate score among same-class detections and every overlap is 8 E_ref clear of
           0.7 / 0.5 / 0.25.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_eval as MG  # noqa: E402
from dcd_amd.eval import synthetic  # noqa: E402

N_RANDOM = 200
RAND_SEED = 20240
RAND_COMB = ((0, 0.5), (0, 0.25), (1, 0.5), (2, 0.7))          # (metric, min_overlap)
RAND_THR = (0.0, 0.3, 0.5, 0.9)
RAND_ND = (0, 1, 5, 63, 64, 65, 100, 129)
RAND_ND_P = (0.05, 0.05, 0.1, 0.16, 0.16, 0.16, 0.16, 0.16)     # one- and no-detection images cannot hold a tie: keep them few
FAR_BOX = (100.0, 100.0, 110.0, 110.0)                         # a detection box inside no DontCare box of the hand cases


# ---- one case through the reference ----------------------------------------------------------------------------------
def new_case(name, nd, ng, ov, metric=0, mo=0.5, thr=(0.0,), ig=None, idt=None, score=None, dt_box=None, dc=()):
    """`ov`: {(detection, ground truth): overlap}, everything else 0.  Defaults: all flags 0, distinct scores in (0.2, 0.8),
    distinct alphas, every detection box far from every DontCare box."""
    m = np.zeros((nd, ng))
    for (j, i), v in ov.items():
        m[j, i] = v
    j, i = np.arange(nd), np.arange(ng)
    c = dict(name=name, ovl=m, metric=metric, min_overlap=float(mo), thr=np.array(thr, np.float64),
             ign_gt=np.zeros(ng, np.int8), ign_dt=np.zeros(nd, np.int8), score=0.2 + 0.6 * ((j * 37) % 101) / 101.0,
             dt_alpha=(j * 0.37) % 6.0 - 3.0, gt_alpha=(i * 0.91) % 6.0 - 3.0,
             dt_box=np.tile(np.array(FAR_BOX), (nd, 1)), dc_box=np.array(dc, np.float64).reshape(-1, 4))
    for key, val in (("ign_gt", ig), ("ign_dt", idt), ("score", score), ("dt_box", dt_box)):
        for k, v in (val or {}).items():
            c[key][k] = v
    return c


def reference_stats(E, c, metric, mo, thr):
    """(mode A scores in ground-truth order, mode B rows (len(thr), 4)) of compute_statistics_jit."""
    nd, ng = c["ovl"].shape
    gt_data = np.concatenate([np.zeros((ng, 4)), c["gt_alpha"][:, None]], 1)
    dt_data = np.concatenate([c["dt_box"], c["dt_alpha"][:, None], c["score"][:, None]], 1)
    ig, idt = c["ign_gt"].astype(np.int64), c["ign_dt"].astype(np.int64)
    a = E.compute_statistics_jit(c["ovl"], gt_data, dt_data, ig, idt, c["dc_box"], metric, mo, 0.0, False)[4]
    rows = [E.compute_statistics_jit(c["ovl"], gt_data, dt_data, ig, idt, c["dc_box"], metric, mo, t, True, metric == 0)[:4]
            for t in thr]
    b = np.array(rows, np.float64).reshape(len(thr), 4)
    b[:, 3] = np.where(b[:, 3] == -1, 0.0, b[:, 3])
    return np.array(a, np.float64), b


# ---- the hand-made cases ---------------------------------------------------------------------------------------------
def hand_cases():
    up = lambda v: float(np.nextafter(v, np.inf))                                           # noqa: E731
    cases = []
    # equal scores for one box (mode A keeps the lowest j); box 1 can only be served by the higher j.  The higher j has the
    # greater overlap, so mode B takes it for box 0 and box 1 is a miss there.
    for name, nd, lo, hi in (("a_equal_scores_adjacent", 8, 5, 6), ("a_equal_scores_63_64", 70, 63, 64),
                             ("a_equal_scores_same_lane", 70, 3, 67)):
        cases.append(new_case(name, nd, 2, {(lo, 0): 0.6, (hi, 0): 0.9, (hi, 1): 0.9}, score={lo: 0.8, hi: 0.8}))
    # equal overlaps for one box (mode B keeps the lowest j); the higher j has the greater score, so mode A takes it
    for name, nd, lo, hi in (("b_equal_overlaps_adjacent", 8, 5, 6), ("b_equal_overlaps_63_64", 70, 63, 64),
                             ("b_equal_overlaps_same_lane", 70, 3, 67)):
        cases.append(new_case(name, nd, 2, {(lo, 0): 0.75, (hi, 0): 0.75, (hi, 1): 0.75}, score={lo: 0.4, hi: 0.7}))
    cases.append(new_case("b_ignored_then_valid_of_smaller_overlap", 8, 1, {(2, 0): 0.9, (5, 0): 0.6}, idt={2: 1}))
    cases.append(new_case("b_valid_then_ignored_of_larger_overlap", 8, 1, {(2, 0): 0.6, (5, 0): 0.9}, idt={5: 1}))
    # only ignored candidates: the FIRST wins, so the better one is left for box 1 (no miss); the best would leave a miss
    for name, nd, first, better in (("b_only_ignored_first_wins", 8, 1, 4), ("b_only_ignored_first_block1_better_block2_lane0", 130, 66, 128),
                                    ("b_only_ignored_first_block0_better_block1_lane0", 70, 5, 64)):
        cases.append(new_case(name, nd, 2, {(first, 0): 0.6, (better, 0): 0.9, (better, 1): 0.9}, idt={first: 1, better: 1}))
    # mode A takes detection 1 (ignored) by score: no score for box 0, and it is gone for box 1, which then gets detection 4
    cases.append(new_case("a_ignored_detection_by_score", 5, 2, {(1, 0): 0.8, (3, 0): 0.8, (1, 1): 0.8, (4, 1): 0.8},
                          idt={1: 1}, score={1: 0.9, 3: 0.5, 4: 0.4}))
    cases.append(new_case("ignored_gt_absorbs_the_only_candidate", 3, 2, {(0, 0): 0.8, (0, 1): 0.8}, ig={0: 1}))
    cases.append(new_case("score_equals_thresh", 2, 2, {(0, 0): 0.8, (1, 1): 0.8}, score={0: 0.5, 1: 0.3},
                          thr=(0.5, up(0.5), 0.3, up(0.3))))
    cases.append(new_case("overlap_equals_min_overlap_07", 2, 2, {(0, 0): 0.7, (1, 1): up(0.7)}, mo=0.7, metric=2))
    cases.append(new_case("overlap_equals_min_overlap_05", 2, 2, {(0, 0): 0.5, (1, 1): up(0.5)}, mo=0.5, metric=1))
    cases.append(new_case("score_of_minus_1e7", 2, 2, {(0, 0): 0.9, (1, 1): 0.9}, score={0: -1e7, 1: up(-1e7)}, thr=(0.0, -2e7)))
    cases.append(new_case("negative_valid_scores", 3, 2, {(0, 0): 0.8, (1, 0): 0.8, (0, 1): 0.8, (2, 1): 0.6},
                          score={0: -5.0, 1: -3.0, 2: -4.0}, thr=(-10.0, -4.0, 0.0)))
    # DontCare: detection 0 lies inside both DontCare boxes, 1 inside none, 2 (ignored_det == 1) inside both
    dcs = ((0, 0, 30, 30), (5, 5, 25, 25))
    inside = {0: (10, 10, 20, 20), 2: (10, 10, 20, 20)}
    for name, metric in (("dontcare_two_boxes_counted_once", 0), ("dontcare_metric_1_subtracts_nothing", 1),
                         ("dontcare_metric_2_subtracts_nothing", 2)):
        cases.append(new_case(name, 3, 1, {}, metric=metric, idt={2: 1}, dt_box=inside, dc=dcs))
    cases.append(new_case("dontcare_assigned_detection_not_subtracted", 2, 1, {(0, 0): 0.8}, dt_box={0: (10, 10, 20, 20)}, dc=dcs))
    # a match at the last index: box 0 takes it, box 1 has no other candidate -- unless the `assigned` bit got lost
    for n in (1, 63, 64, 65, 127, 128, 129):
        cases.append(new_case("last_index_of_%d" % n, n, 2, {(n - 1, 0): 0.8, (n - 1, 1): 0.8}))
    # 4096: bit 63 of lane 63.  Box 1 falls back to 4031 (lane 63, bit 62), box 2 finds both used, box 3 takes detection 0
    cases.append(new_case("last_index_of_4096", 4096, 4, {(4095, 0): 0.8, (4095, 1): 0.9, (4031, 1): 0.6, (4095, 2): 0.9,
                                                         (4031, 2): 0.8, (0, 3): 0.8}, thr=(0.0, 0.5)))
    cases.append(new_case("no_ground_truth", 5, 0, {}, idt={1: 1, 2: -1}, score={0: 0.1, 1: 0.2, 2: 0.3, 3: 0.4, 4: 0.5},
                          thr=(0.0, 0.35)))
    cases.append(new_case("no_detections", 0, 3, {}, ig={1: 1, 2: -1}))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# ---- the random quantised images ---------------------------------------------------------------------------------------
def random_case(rng, k):
    nd, ng = int(rng.choice(RAND_ND, p=RAND_ND_P)), int(rng.randint(0, 13))
    c = new_case("rand_%d" % k, nd, ng, {})
    c["ovl"] = rng.randint(0, 9, (nd, ng)) / 8.0
    c["score"] = rng.randint(1, 10, nd) / 10.0
    c["ign_gt"], c["ign_dt"] = rng.randint(-1, 2, ng).astype(np.int8), rng.randint(-1, 2, nd).astype(np.int8)
    c["dt_alpha"], c["gt_alpha"] = rng.randint(-12, 13, nd) / 4.0, rng.randint(-12, 13, ng) / 4.0
    xy = rng.randint(0, 13, (nd, 2)).astype(np.float64)
    c["dt_box"] = np.concatenate([xy, xy + 4.0], 1)                          # 4 x 4 boxes, 8 x 8 DontCare boxes: ratios k/16
    XY = rng.randint(0, 9, (int(rng.randint(0, 3)), 2)).astype(np.float64)
    c["dc_box"] = np.concatenate([XY, XY + 8.0], 1)
    return c


def has_ties(c):
    score_tie = overlap_tie = False
    for i in np.flatnonzero(c["ign_gt"] != -1):
        cand = (c["ign_dt"] != -1) & (c["ovl"][:, i] > 0.5)
        if cand.any():
            score_tie |= int((c["score"][cand] == c["score"][cand].max()).sum()) > 1
        cand &= c["ign_dt"] == 0
        if cand.any():
            overlap_tie |= int((c["ovl"][cand, i] == c["ovl"][cand, i].max()).sum()) > 1
    return score_tie and overlap_tie


def store_inputs(out, prefix, cases):
    cat = lambda k, shape=(0,): np.concatenate([c[k].reshape((-1,) + shape[1:]) for c in cases], 0)      # noqa: E731
    out[prefix + "nd"] = np.array([c["ovl"].shape[0] for c in cases], np.int32)
    out[prefix + "ng"] = np.array([c["ovl"].shape[1] for c in cases], np.int32)
    out[prefix + "ndc"] = np.array([len(c["dc_box"]) for c in cases], np.int32)
    out[prefix + "ovl"] = cat("ovl")
    out[prefix + "ign_gt"], out[prefix + "ign_dt"] = cat("ign_gt").astype(np.int8), cat("ign_dt").astype(np.int8)
    for k in ("score", "dt_alpha", "gt_alpha"):
        out[prefix + k] = cat(k).astype(np.float64)
    out[prefix + "dt_box"], out[prefix + "dc_box"] = cat("dt_box", (0, 4)), cat("dc_box", (0, 4))


def make_cases(E, out):
    hand = hand_cases()
    store_inputs(out, "hand_", hand)
    out["hand_name"] = np.array([c["name"] for c in hand])
    out["hand_metric"] = np.array([c["metric"] for c in hand], np.int8)
    out["hand_min_overlap"] = np.array([c["min_overlap"] for c in hand], np.float64)
    out["hand_nthr"] = np.array([len(c["thr"]) for c in hand], np.int32)
    out["hand_thr"] = np.concatenate([c["thr"] for c in hand])
    res = [reference_stats(E, c, c["metric"], c["min_overlap"], c["thr"]) for c in hand]
    out["hand_a_n"] = np.array([len(a) for a, _ in res], np.int32)
    out["hand_a"], out["hand_b"] = np.concatenate([a for a, _ in res]), np.concatenate([b for _, b in res], 0)
    for c, (a, b) in zip(hand, res):
        print("%-52s A %-22s B %s" % (c["name"], np.round(a, 3).tolist(), b[:, :3].astype(int).tolist()))

    rng = np.random.RandomState(RAND_SEED)
    rand = [random_case(rng, k) for k in range(N_RANDOM)]
    tied = sum(has_ties(c) for c in rand)
    assert 2 * tied > N_RANDOM, tied
    store_inputs(out, "rand_", rand)
    out["rand_comb"], out["rand_thr"] = np.array(RAND_COMB, np.float64), np.array(RAND_THR, np.float64)
    out["rand_tied_images"] = np.int64(tied)
    a_n, a_all, b_all = [], [], []
    for c in rand:
        for metric, mo in RAND_COMB:
            a, b = reference_stats(E, c, metric, mo, RAND_THR)
            a_n.append(len(a))
            a_all.append(a)
            b_all.append(b)
    out["rand_a_n"] = np.array(a_n, np.int32).reshape(N_RANDOM, len(RAND_COMB))
    out["rand_a"] = np.concatenate(a_all)
    out["rand_b"] = np.array(b_all, np.float64).reshape(N_RANDOM, len(RAND_COMB), len(RAND_THR), 4)
    print("%d hand-made cases, %d random images, %d of them with a score tie and an overlap tie" % (len(hand), N_RANDOM, tied))


# ---- the scene with duplicate scores -----------------------------------------------------------------------------------
def make_tie_scene(E, K, V, seed, e_ref, folder):
    rng = np.random.RandomState(seed)
    n_img = 8
    gts, dts = synthetic.make_scene(rng, n_img, n_obj=(6, 15), empty_gt=(3,), empty_dt=(6,))
    for d in dts:
        d["score"] = np.round(d["score"] / 0.05) * 0.05
    ids = ["%06d" % (i * 5 + 2) for i in range(n_img)]
    if os.path.isdir(folder):
        shutil.rmtree(folder)
    os.makedirs(os.path.join(folder, "label_2"))
    os.makedirs(os.path.join(folder, "pred"))
    with open(os.path.join(folder, "val.txt"), "w") as f:
        f.write("".join(i + "\n" for i in ids))
    rows = [MG.detection_rows(d) for d in dts]
    for i, g, r in zip(ids, gts, rows):
        with open(os.path.join(folder, "label_2", i + ".txt"), "w") as f:
            f.write(MG.label_lines(g))
        V.generate_kitti_3d_detection(torch.from_numpy(r), os.path.join(folder, "pred", i + ".txt"))
    gts = K.get_label_annos(os.path.join(folder, "label_2"), ids)
    dts = K.get_label_annos(os.path.join(folder, "pred"), ids)
    dup = 0
    for d in dts:
        pairs = list(zip(d["name"].tolist(), d["score"].tolist()))
        dup += len(set(pairs)) < len(pairs)
    if dup < 3:
        return None, "%d images with a duplicate score inside a class" % dup
    ref = MG.reference_overlaps(E, gts, dts)
    flat = np.concatenate([o.ravel() for m in range(3) for o in ref[m]])
    clear = min(np.abs(flat - t).min() for t in (0.7, 0.5, 0.25))
    if clear < 8 * e_ref:
        return None, "clearance %g" % clear

    out = {"ids": np.array(ids), "clearance": np.float64(clear), "dup_images": np.int64(dup)}
    MG.pack(gts, "gt", out)
    MG.pack(dts, "dt", out)
    for m in range(3):
        for i in range(n_img):
            out["ref_%d_%d" % (m, i)] = ref[m][i]
    # what eval_class hands to / gets from get_thresholds and fused_compute_statistics, in call order
    log = []
    get_thresholds, fused = E.get_thresholds, E.fused_compute_statistics

    def rec_thresholds(scores, num_gt, num_sample_pts=41):
        inp = np.sort(np.array(scores, np.float64))
        thr = get_thresholds(scores, num_gt, num_sample_pts)
        log.append([inp, np.int64(num_gt), np.array(thr, np.float64), None])
        return thr

    def rec_fused(overlaps, pr, *a, **k):
        fused(overlaps, pr, *a, **k)
        assert log[-1][3] is None
        log[-1][3] = pr.copy()
    E.get_thresholds, E.fused_compute_statistics = rec_thresholds, rec_fused
    try:
        for metric in ("R40", "R11"):
            del log[:]
            detail = {}
            text, rd = E.get_official_eval_result(gts, dts, [0, 1, 2], PR_detail_dict=detail, metric=metric)
            out["text_" + metric] = np.array(text)
            out["dict_keys_" + metric] = np.array(list(rd.keys()))
            out["dict_values_" + metric] = np.array([rd[k] for k in rd], np.float64)
        assert len(log) == 54
        for n, (scores, num_gt, thr, pr) in enumerate(log):
            out["comb_%d_scores" % n], out["comb_%d_num_gt" % n] = scores, num_gt
            out["comb_%d_thresholds" % n], out["comb_%d_pr" % n] = thr, pr
        for k in ("bbox", "aos", "bev", "3d"):
            out["detail_" + k] = detail[k]
        mo = np.stack([np.array([[0.7, 0.5, 0.5]] * 3), np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])], 0)
        for m in range(3):
            ret = E.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], m, mo, compute_aos=(m == 0))
            for k in ("precision", "recall", "orientation"):
                out["%s_%d" % (k, m)] = ret[k]
    finally:
        E.get_thresholds, E.fused_compute_statistics = get_thresholds, fused
    tied_combs = sum(len(np.unique(s)) < len(s) for s, _, _, _ in log[:54])         # the eval_class calls above log again
    if tied_combs < 10:
        return None, "only %d combinations with tied matched scores" % tied_combs
    out["tied_combinations"] = np.int64(tied_combs)
    return out, "ok"


def main():
    """Writes the fixture; with --check, regenerates it elsewhere and compares with the committed files instead."""
    check = "--check" in sys.argv[1:]
    R, E, K, V = MG.load_reference()
    out = {}
    make_cases(E, out)
    with np.load(os.path.join(HERE, "eval_pairs.npz")) as z:
        e_ref = float(z["E_ref"])
    committed = os.path.join(HERE, "eval_scene_ties")
    folder = tempfile.mkdtemp() if check else committed
    seed = 0
    while True:
        try:
            scene, why = make_tie_scene(E, K, V, seed, e_ref, folder)
        except IndexError:
            scene, why = None, "more than 8 vertices"
        print("eval_scene_ties: seed %d: %s" % (seed, why))
        if scene is not None:
            break
        seed += 1
    scene["seed"] = np.int64(seed)
    out.update({"scene_" + k: v for k, v in scene.items()})
    path = os.path.join(HERE, "eval_ties.npz")
    print(str(scene["text_R40"]))
    print("clearance %.3g = %.1f E_ref, %d images with duplicates, %d of 54 combinations with tied matched scores" % (
        scene["clearance"], scene["clearance"] / e_ref, scene["dup_images"], scene["tied_combinations"]))
    if check:
        with np.load(path) as z:
            assert sorted(z.files) == sorted(out), "key sets differ"
            for k in z.files:
                a, b = z[k], np.asarray(out[k])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        for sub in ("label_2", "pred", "."):
            names = sorted(n for n in os.listdir(os.path.join(committed, sub)) if n.endswith(".txt"))
            assert names == sorted(n for n in os.listdir(os.path.join(folder, sub)) if n.endswith(".txt")), sub
            for n in names:
                with open(os.path.join(committed, sub, n), "rb") as f, open(os.path.join(folder, sub, n), "rb") as g:
                    assert f.read() == g.read(), n
        shutil.rmtree(folder)
        print("the committed fixture is reproduced bit for bit (%d arrays)" % len(out))
        return
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
