"""The assignment kernel of csrc/eval.hip (`eval_match`) where its re-derived form can differ from the reference's scan: equal
scores and equal overlaps inside and across lane blocks, ignored candidates, the strict comparisons, DontCare boxes, the
4096-detection limit and tables that do not fit.  Expected values were recorded from the reference's own
`compute_statistics_jit` by tests/golden/make_golden_eval_ties.py; test_eval_host.py shows that each hand-made case changes a
recorded number under the wrong rule it is named for."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_fixtures as EF  # noqa: E402
from arena import Arena  # noqa: E402
from dcd_amd import _lib  # noqa: E402
from dcd_amd.eval import kitti_annos, kitti_ap  # noqa: E402

pytestmark = pytest.mark.gpu

TIES = EF.load("eval_ties.npz")
RAND_PAIRS = [(int(m), float(mo)) for m, mo in TIES["rand_comb"]]
RAND_THR = TIES["rand_thr"]
AOS_PAIRS = [m for m, p in enumerate(RAND_PAIRS) if p[0] == 0]        # the combinations with a similarity slot, in slot order
N_COMB = 54
BAD_ARG = 1                                                           # DCD_ERR_BAD_ARG


def on(cuda):
    return lambda array: torch.from_numpy(array).to(cuda)


# ---- the hand-made cases -----------------------------------------------------------------------------------------------
def test_hand_cases_mode_a_scores_in_ground_truth_order(cuda):
    """All cases as the images of one load, one combination per (metric, min_overlap) pair that occurs."""
    cases = EF.ties_cases("hand")
    assert len(cases) == 32 and max(c["ovl"].shape[0] for c in cases) == 4096
    pairs = sorted({(c["metric"], c["min_overlap"]) for c in cases})
    rows = EF.ties_mode_a(kitti_ap.KittiEvaluator(cuda), on(cuda), cases, pairs)
    wrong = [c["name"] for c, per_comb in zip(cases, rows)
             if not np.array_equal(per_comb[pairs.index((c["metric"], c["min_overlap"]))], c["a"])]
    assert wrong == []


def test_hand_cases_mode_b_counts_and_similarity(cuda):
    """Each case as a one-image load, so that a failure names the case; twice, for the bit-equal similarity."""
    wrong = []
    for c in EF.ties_cases("hand"):
        runs = [EF.ties_mode_b(kitti_ap.KittiEvaluator(cuda), on(cuda), [c], [(c["metric"], c["min_overlap"])], c["thr"])
                for _ in range(2)]
        counts, sim = runs[0]
        ok = np.array_equal(counts[0], c["b"][:, :3]) and np.array_equal(runs[1][0], counts)
        if c["metric"] == 0:
            ok = ok and np.allclose(sim[0], c["b"][:, 3], rtol=1e-9, atol=0) and np.array_equal(runs[1][1], sim)
        if not ok:
            wrong.append((c["name"], counts[0].tolist(), c["b"][:, :3].astype(int).tolist()))
    assert wrong == []


# ---- the random quantised images -----------------------------------------------------------------------------------------
def check_random_part(cuda, cases):
    ev = kitti_ap.KittiEvaluator(cuda)
    rows = EF.ties_mode_a(ev, on(cuda), cases, RAND_PAIRS)
    for c, per_comb in zip(cases, rows):
        for m in range(len(RAND_PAIRS)):
            assert np.array_equal(per_comb[m], c["a"][m]), (c["name"], RAND_PAIRS[m])
    want = sum(c["b"] for c in cases)                                  # (combinations, thresholds, 4) summed over the images
    runs = [EF.ties_mode_b(ev, on(cuda), cases, RAND_PAIRS, RAND_THR) for _ in range(2)]
    counts, sim = runs[0]
    assert np.array_equal(counts, want[..., :3])
    assert want[..., 0].min() > 0 and want[..., 1].min() > 0 and want[..., 2].min() > 0
    np.testing.assert_allclose(sim, want[AOS_PAIRS, :, 3], rtol=1e-9, atol=0)
    assert np.array_equal(runs[1][0], counts) and np.array_equal(runs[1][1], sim)


def test_random_images_with_ties(cuda):
    cases = EF.ties_cases("rand")
    assert len(cases) == 200 and 2 * int(TIES["rand_tied_images"]) > len(cases)
    check_random_part(cuda, cases)


def test_random_images_in_reversed_order(cuda):
    check_random_part(cuda, EF.ties_cases("rand")[::-1])


# ---- limits: through the raw entry point, outputs between guard words ------------------------------------------------------
def blank_case(nd, ng):
    """nd detections that all overlap every one of ng ground-truth boxes."""
    return dict(name="blank_%d_%d" % (nd, ng), ovl=np.full((nd, ng), 0.9), ign_gt=np.zeros(ng, np.int8), ign_dt=np.zeros(nd, np.int8),
                score=np.linspace(0.2, 0.8, nd), dt_alpha=np.zeros(nd), gt_alpha=np.zeros(ng), dt_box=np.tile([100.0, 100, 110, 110], (nd, 1)),
                dc_box=np.zeros((0, 4)))


class RawMatch:
    """One `dcd_eval_match` call on a loaded evaluator with every output in an Arena.  `tables` replaces offset tables by
    tampered ones, `ints` overrides integer fields of the argument block; `written_*` say which elements the call must write
    (bool arrays; None: all), the rest must keep the poison.  counts start from `counts0` (zeros: the kernel adds to them)."""

    def __init__(self, cuda, cases, comb, mo, n_slots, thr=None, tables=None, ints=None, written_scores=None, written_sim=None,
                 counts0=0):
        packed, flags, ovl = EF.ties_pack(cases)
        self.packed = packed
        ev = kitti_ap.KittiEvaluator(cuda)
        ev.load(packed, flags)
        ovl = torch.from_numpy(ovl).to(cuda)
        mode = 0 if thr is None else 1
        a, keep = ev._args(mode, ovl, comb, mo)
        for k, v in (tables or {}).items():
            keep.append(torch.from_numpy(np.ascontiguousarray(v.astype(packed[k].dtype))).to(cuda))
            setattr(a, k, _lib.ptr(keep[-1]))
        arena = Arena(cuda)
        as_mask = lambda m: None if m is None else torch.from_numpy(np.ascontiguousarray(m))          # noqa: E731
        if mode == 0:
            self.scores = arena.out((len(comb), ev.G), "scores", torch.float64, written=as_mask(written_scores))
            a.scores = Arena.ptr(self.scores)
        else:
            T = len(thr)
            keep += [torch.from_numpy(np.tile(np.asarray(thr, np.float64), (len(comb), 1))).to(cuda),
                     torch.full((len(comb),), T, dtype=torch.int32, device=cuda)]
            self.counts = arena.place(torch.full((len(comb), T, 3), counts0, dtype=torch.int32), "counts", inplace=counts0 == 0)
            self.sim_part = arena.out((len(cases), n_slots, T), "sim_part", torch.float64, written=as_mask(written_sim))
            a.T, a.n_slots = T, n_slots
            a.thresholds, a.n_thresh = _lib.ptr(keep[-2]), _lib.ptr(keep[-1])
            a.counts, a.sim_part = Arena.ptr(self.counts), Arena.ptr(self.sim_part)
        for k, v in (ints or {}).items():
            setattr(a, k, v)
        self.status = ev.lib.dcd_eval_match(_lib.stream_of(ovl), ctypes.byref(a))
        arena.check("dcd_eval_match")
        self.keep = keep


def test_image_with_4097_detections_is_refused(cuda):
    cases = [EF.ties_cases("rand")[0], blank_case(4097, 1)]
    comb, mo, n_slots = EF.ties_comb(RAND_PAIRS)
    nothing = np.zeros((len(comb), sum(c["ovl"].shape[1] for c in cases)), bool)
    run = RawMatch(cuda, cases, comb, mo, n_slots, written_scores=nothing)
    assert run.packed["max_dt"] == 4097 and run.status == BAD_ARG
    run = RawMatch(cuda, cases, comb, mo, n_slots, thr=RAND_THR, written_sim=np.zeros((2, n_slots, len(RAND_THR)), bool),
                   counts0=-77)                                       # Arena.check: the placed counts are unchanged
    assert run.status == BAD_ARG and bool((run.counts == -77).all())


def limit_cases():
    """Eight random-part images; the last one (the victim of a tampered table) has several lane blocks and ground truth."""
    cases = EF.ties_cases("rand")
    victim = next(k for k, c in enumerate(cases) if c["ovl"].shape[0] >= 65 and c["ovl"].shape[1] >= 3 and (c["ign_gt"] == 0).any())
    others = [c for k, c in enumerate(cases) if k != victim and c["ovl"].size][:7]
    return others + [cases[victim]]


@pytest.mark.parametrize("what", ["gt_off_past_G", "dt_off_past_D", "pair_off_past_P", "nd_over_4096"])
def test_only_the_image_whose_tables_do_not_fit_does_nothing(cuda, what):
    """`max_dt` understates the truth, so the launch happens; the wave of the offending image returns before it reads or
    writes anything, every other image gives the recorded results."""
    cases = limit_cases()
    bad = len(cases) - 1
    tables = {}
    if what == "nd_over_4096":
        bad = 4
        cases = cases[:bad] + [blank_case(4097, 2)] + cases[bad:]
    packed = EF.ties_pack(cases)[0]
    G, D, P = int(packed["gt_off"][-1]), int(packed["dt_off"][-1]), int(packed["pair_off"][-1])
    if what == "gt_off_past_G":
        tables["gt_off"] = np.concatenate([packed["gt_off"][:-1], [G + 1]])
    elif what == "dt_off_past_D":
        tables["dt_off"] = np.concatenate([packed["dt_off"][:-1], [D + 1]])
    elif what == "pair_off_past_P":
        tables["pair_off"] = packed["pair_off"].copy()
        tables["pair_off"][bad] += 1                                  # the last block now ends one element past P
    ints = {"max_dt": 129}
    comb, mo, n_slots = EF.ties_comb(RAND_PAIRS)
    good = [k for k in range(len(cases)) if k != bad]
    g_off = packed["gt_off"]
    written = np.ones((len(comb), G), bool)
    written[:, g_off[bad]:g_off[bad + 1]] = False
    assert g_off[bad + 1] > g_off[bad]

    run = RawMatch(cuda, cases, comb, mo, n_slots, tables=tables, ints=ints, written_scores=written)
    assert run.status == 0
    scores = run.scores.cpu().numpy()
    for k in good:
        for m in range(len(comb)):
            row = scores[m, g_off[k]:g_off[k + 1]]
            assert np.array_equal(row[row != kitti_ap.NO_DETECTION], cases[k]["a"][m]), (cases[k]["name"], m)

    written = np.ones((len(cases), n_slots, len(RAND_THR)), bool)
    written[bad] = False
    run = RawMatch(cuda, cases, comb, mo, n_slots, thr=RAND_THR, tables=tables, ints=ints, written_sim=written)
    assert run.status == 0
    want = sum(cases[k]["b"] for k in good)
    assert np.array_equal(run.counts.cpu().numpy(), want[..., :3])
    sim = run.sim_part.cpu().numpy()[good].sum(0)
    np.testing.assert_allclose(sim, want[AOS_PAIRS, :, 3], rtol=1e-9, atol=0)


def test_combination_rows_that_do_not_fit_write_nothing(cuda):
    """Metric 3, a flag row >= n_rows and, in mode B, a similarity slot >= n_slots, among valid combinations."""
    cases = limit_cases()
    packed = EF.ties_pack(cases)[0]
    g_off, G = packed["gt_off"], int(packed["gt_off"][-1])
    comb = np.array([[0, 0, 0], [3, 0, -1], [0, 1, -1], [1, 0, -1], [0, 0, 1]], np.int32)       # one flag row, one slot
    mo = np.full(5, 0.5)
    pair_of = {0: RAND_PAIRS.index((0, 0.5)), 3: RAND_PAIRS.index((1, 0.5)), 4: RAND_PAIRS.index((0, 0.5))}
    written = np.zeros((5, G), bool)
    written[[0, 3, 4]] = True                                          # mode A has no slots: row 4 is valid there
    run = RawMatch(cuda, cases, comb, mo, 1, written_scores=written)
    assert run.status == 0
    scores = run.scores.cpu().numpy()
    for k, c in enumerate(cases):
        for row, m in pair_of.items():
            got = scores[row, g_off[k]:g_off[k + 1]]
            assert np.array_equal(got[got != kitti_ap.NO_DETECTION], c["a"][m]), (c["name"], row)
    run = RawMatch(cuda, cases, comb, mo, 1, thr=RAND_THR)            # slot 0 of every image is written, nothing else exists
    assert run.status == 0
    counts = run.counts.cpu().numpy()
    want = sum(c["b"] for c in cases)
    assert (counts[[1, 2, 4]] == 0).all()
    assert np.array_equal(counts[0], want[pair_of[0], :, :3]) and np.array_equal(counts[3], want[pair_of[3], :, :3])
    np.testing.assert_allclose(run.sim_part.cpu().numpy().sum(0)[0], want[pair_of[0], :, 3], rtol=1e-9, atol=0)


# ---- duplicate scores end to end -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_scene_annos():
    ids = [str(s) for s in EF.ties_scene()["ids"]]
    return (kitti_annos.read_annos(os.path.join(EF.TIES_SCENE_DIR, "label_2"), ids),
            kitti_annos.read_annos(os.path.join(EF.TIES_SCENE_DIR, "pred"), ids))


def test_tie_scene_statistics_from_the_reference_overlaps(cuda, tie_scene_annos):
    scene = EF.ties_scene()
    gts, dts = tie_scene_annos
    assert len(gts) == 8 and int(scene["dup_images"]) >= 3 and int(scene["tied_combinations"]) >= 10
    flags = kitti_ap.ignore_flags(gts, dts, [0, 1, 2])
    ev = kitti_ap.KittiEvaluator(cuda)
    ev.load(kitti_ap.pack(gts, dts, flags["dontcare"]), flags)
    ovl = torch.from_numpy(EF.reference_overlaps(scene, 8)).to(cuda)
    stages = {}
    kitti_ap.pr_tables(ev, ovl, 3, True, kitti_ap.MIN_OVERLAPS[:, :, [0, 1, 2]], flags["num_valid"], stages)
    for n in range(N_COMB):
        assert np.array_equal(np.sort(stages["scores"][n]), scene["comb_%d_scores" % n]), n
        assert all(a == b for a, b in zip(stages["thresholds"][n], scene["comb_%d_thresholds" % n]))
        pr = scene["comb_%d_pr" % n]
        assert np.array_equal(stages["counts"][n, :len(pr)], pr[:, :3]), n
        assert (stages["counts"][n, len(pr):] == 0).all()
        if n < 18:
            np.testing.assert_allclose(stages["similarity"][n, :len(pr)], pr[:, 3], rtol=1e-9, atol=0)


@pytest.mark.parametrize("metric", ["R40", "R11"])
def test_official_eval_reproduces_the_reference_table_of_the_tie_scene(cuda, tie_scene_annos, metric):
    scene = EF.ties_scene()
    gts, dts = tie_scene_annos
    runs = []
    for _ in range(2):
        detail, stages = {}, {}
        text, ret = kitti_ap.official_eval(gts, dts, [0, 1, 2], metric=metric, device=cuda, detail=detail, stages=stages)
        runs.append((text, ret, detail, stages))
    text, ret, detail, stages = runs[0]
    assert text == str(scene["text_" + metric])
    assert list(ret) == [str(k) for k in scene["dict_keys_" + metric]]
    np.testing.assert_allclose(np.array([ret[k] for k in ret]), scene["dict_values_" + metric], rtol=1e-9, atol=1e-9)
    for m in range(3):
        for k, name in enumerate(("precision", "recall", "orientation")):
            np.testing.assert_allclose(stages["curves"][m][k], scene["%s_%d" % (name, m)], rtol=1e-9, atol=1e-9)
    for k in ("bbox", "aos", "bev", "3d"):
        np.testing.assert_allclose(detail[k], scene["detail_" + k], rtol=1e-9, atol=1e-9)
    again = runs[1]
    assert again[0] == text and all(np.array_equal(again[1][k], ret[k], equal_nan=True) for k in ret)
    assert np.array_equal(again[3]["similarity"], stages["similarity"]) and np.array_equal(again[3]["counts"], stages["counts"])
    t2, r2 = kitti_ap.evaluate(os.path.join(EF.TIES_SCENE_DIR, "label_2"), os.path.join(EF.TIES_SCENE_DIR, "pred"),
                               os.path.join(EF.TIES_SCENE_DIR, "val.txt"), current_class=[0, 1, 2], metric=metric, device=cuda)
    assert t2 == text and all(np.array_equal(r2[k], ret[k], equal_nan=True) for k in ret)
