"""Shared by test_eval_host.py, test_gpu_eval.py and test_gpu_eval_ties.py: loaders for the evaluator fixtures of
tests/golden/make_golden_eval.py and make_golden_eval_ties.py, and a numpy stand-in for the device evaluator (test-only: the product has no CPU path)."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENE_DIR = os.path.join(GOLDEN, "eval_scene")
ANNO_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def annos(fix, prefix):
    """The per-image annotation dicts stored under `prefix` ('gt' / 'dt')."""
    off = np.concatenate([[0], np.cumsum(fix[prefix + "_count"])])
    return [{k: fix["%s_%s" % (prefix, k)][off[i]:off[i + 1]] for k in ANNO_KEYS if "%s_%s" % (prefix, k) in fix}
            for i in range(len(off) - 1)]


def scene_ids():
    return [str(s) for s in load("eval_scene.npz")["ids"]]


def reference_overlaps(fix, n_img):
    """(3, P) float64: the reference's stored [dt, gt] matrices in the device layout."""
    return np.stack([np.concatenate([fix["ref_%d_%d" % (m, i)].ravel() for i in range(n_img)]) for m in range(3)])


# ---- numpy stand-in for dcd_amd.eval.kitti_ap.KittiEvaluator ---------------------------------------------------------------
def _corners(r):
    c, s = math.cos(r[4]), math.sin(r[4])
    x, y = r[2] / 2, r[3] / 2
    return [(c * px + s * py + r[0], -s * px + c * py + r[1]) for px, py in ((-x, -y), (-x, y), (x, y), (x, -y))]


def _area2(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))


def clip_area(subj, cl):
    """Exact area of the intersection of two convex polygons (Sutherland-Hodgman, float64)."""
    if _area2(cl) < 0:
        cl = cl[::-1]
    out = subj
    for i in range(len(cl)):
        a, b = cl[i], cl[(i + 1) % len(cl)]
        inp, out = out, []
        if not inp:
            break
        side = [(b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) for p in inp]
        for j in range(len(inp)):
            p, q, sp, sq = inp[j], inp[(j + 1) % len(inp)], side[j], side[(j + 1) % len(inp)]
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return abs(_area2(out)) / 2 if len(out) > 2 else 0.0


def box_overlap_2d(b, q, criterion=-1):
    iw = min(b[2], q[2]) - max(b[0], q[0])
    ih = min(b[3], q[3]) - max(b[1], q[1])
    if not (iw > 0 and ih > 0):
        return 0.0
    area = (b[2] - b[0]) * (b[3] - b[1])
    return iw * ih / (area + (q[2] - q[0]) * (q[3] - q[1]) - iw * ih if criterion == -1 else area)


class EmulatedEvaluator:
    """What csrc/eval.hip computes, in plain Python: exact overlaps and the arg-max form of the assignment."""

    def __init__(self, device=None):
        pass

    def load(self, packed, flags):
        self.p, self.f = packed, flags
        self.n_img = packed["n_img"]

    def overlaps(self):
        p = self.p
        out = np.zeros((3, int(p["pair_off"][-1])))
        for i in range(self.n_img):
            g0, g1, d0, d1 = p["gt_off"][i], p["gt_off"][i + 1], p["dt_off"][i], p["dt_off"][i + 1]
            for d in range(d0, d1):
                D = p["dt_box3d"][d]
                d32 = D[[0, 2, 3, 5, 6]].astype(np.float32).astype(np.float64)
                for g in range(g0, g1):
                    k = p["pair_off"][i] + (d - d0) * (g1 - g0) + (g - g0)
                    G = p["gt_box3d"][g]
                    g32 = G[[0, 2, 3, 5, 6]].astype(np.float32).astype(np.float64)
                    out[0, k] = box_overlap_2d(p["dt_box2d"][d], p["gt_box2d"][g])
                    inter = clip_area(_corners(g32), _corners(d32))
                    out[1, k] = inter / (g32[2] * g32[3] + d32[2] * d32[3] - inter)
                    ih = min(D[1], G[1]) - max(D[1] - D[4], G[1] - G[4])
                    if inter > 0 and ih > 0:
                        out[2, k] = ih * inter / (D[3] * D[4] * D[5] + G[3] * G[4] * G[5] - ih * inter)
        return out

    def _match(self, i, overlaps, metric, row, min_overlap, thresh, fp_mode, aos):
        p, f = self.p, self.f
        g0, g1, d0, d1 = p["gt_off"][i], p["gt_off"][i + 1], p["dt_off"][i], p["dt_off"][i + 1]
        ng, nd = g1 - g0, d1 - d0
        ig, idt = f["gt"][row, g0:g1], f["dt"][row, d0:d1]
        score = p["dt_score"][d0:d1]
        ov = overlaps[metric, p["pair_off"][i]:p["pair_off"][i] + nd * ng].reshape(nd, ng)
        assigned = np.zeros(nd, bool)
        live = (idt != -1) & ~((score < thresh) if fp_mode else np.zeros(nd, bool))
        tp = fn = 0
        sim, matched = 0.0, np.full(ng, -1e7)
        for g in range(ng):
            if ig[g] == -1:
                continue
            cand = np.flatnonzero(live & ~assigned & (ov[:, g] > min_overlap))
            det = -1
            if not fp_mode:
                cand = cand[score[cand] > -1e7]
                if len(cand):
                    det = cand[np.argmax(score[cand])]                 # np.argmax: the first of equals
            else:
                c0 = cand[idt[cand] == 0]
                if len(c0):
                    det = c0[np.argmax(ov[c0, g])]
                elif len(cand):
                    det = cand[0]
            if det < 0:
                fn += int(ig[g] == 0)
                continue
            assigned[det] = True
            if ig[g] == 1 or idt[det] == 1:
                continue
            tp += 1
            matched[g] = score[det]
            if aos:
                sim += (1.0 + math.cos(p["gt_alpha"][g0 + g] - p["dt_alpha"][d0 + det])) / 2.0
        fp = 0
        if fp_mode:
            dcs = p["dc_box"][p["dc_off"][i]:p["dc_off"][i + 1]]
            for d in np.flatnonzero((idt == 0) & ~assigned & ~(score < thresh)):
                inside = metric == 0 and any(box_overlap_2d(p["dt_box2d"][d0 + d], q, 0) > min_overlap for q in dcs)
                fp += int(not inside)
        return tp, fp, fn, sim, matched

    def match_scores(self, overlaps, comb, min_overlap):
        out = np.full((len(comb), int(self.p["gt_off"][-1])), -1e7)
        for c, (metric, row, _) in enumerate(comb):
            for i in range(self.n_img):
                out[c, self.p["gt_off"][i]:self.p["gt_off"][i + 1]] = self._match(i, overlaps, metric, row, min_overlap[c], 0.0,
                                                                                 False, False)[4]
        return out

    def match_counts(self, overlaps, comb, min_overlap, thresholds, n_slots):
        T = max(1, max(len(t) for t in thresholds))
        counts, sim = np.zeros((len(comb), T, 3), np.int64), np.zeros((n_slots, T))
        for c, (metric, row, slot) in enumerate(comb):
            for t, thresh in enumerate(thresholds[c]):
                for i in range(self.n_img):
                    tp, fp, fn, s, _ = self._match(i, overlaps, metric, row, min_overlap[c], thresh, True, slot >= 0)
                    counts[c, t] += (tp, fp, fn)
                    if slot >= 0:
                        sim[slot, t] += s
        return counts, sim


# ---- the tie fixture of tests/golden/make_golden_eval_ties.py ---------------------------------------------------------------
TIES_SCENE_DIR = os.path.join(GOLDEN, "eval_scene_ties")


@functools.lru_cache(maxsize=None)
def ties_cases(part):
    """The cases of part 'hand' or 'rand' as dicts: the inputs (ovl [nd, ng], ign_gt, ign_dt, score, dt_alpha, gt_alpha, dt_box,
    dc_box) and what the reference's compute_statistics_jit returned for them.  hand: name, metric, min_overlap, thr, `a` (the
    mode-A scores in ground-truth order) and `b` (len(thr), 4).  rand: `a` is a list over the combinations of `rand_comb`, `b` is
    (combinations, thresholds, 4)."""
    z = load("eval_ties.npz")
    p = part + "_"
    nd, ng, ndc = (z[p + k].astype(np.int64) for k in ("nd", "ng", "ndc"))
    d0, g0, c0, p0 = (np.concatenate([[0], np.cumsum(v)]) for v in (nd, ng, ndc, nd * ng))
    cases = []
    for k in range(len(nd)):
        c = dict(ovl=z[p + "ovl"][p0[k]:p0[k + 1]].reshape(nd[k], ng[k]), ign_gt=z[p + "ign_gt"][g0[k]:g0[k + 1]],
                 ign_dt=z[p + "ign_dt"][d0[k]:d0[k + 1]], gt_alpha=z[p + "gt_alpha"][g0[k]:g0[k + 1]],
                 dc_box=z[p + "dc_box"][c0[k]:c0[k + 1]])
        for key in ("score", "dt_alpha", "dt_box"):
            c[key] = z[p + key][d0[k]:d0[k + 1]]
        cases.append(c)
    if part == "hand":
        t0, a0 = (np.concatenate([[0], np.cumsum(z[p + k])]) for k in ("nthr", "a_n"))
        for k, c in enumerate(cases):
            c.update(name=str(z["hand_name"][k]), metric=int(z["hand_metric"][k]), min_overlap=float(z["hand_min_overlap"][k]),
                     thr=z["hand_thr"][t0[k]:t0[k + 1]], a=z["hand_a"][a0[k]:a0[k + 1]], b=z["hand_b"][t0[k]:t0[k + 1]])
    else:
        a0 = np.concatenate([[0], np.cumsum(z["rand_a_n"].ravel())]).reshape(-1)
        n_comb = z["rand_comb"].shape[0]
        for k, c in enumerate(cases):
            c.update(name="rand_%d" % k, b=z["rand_b"][k],
                     a=[z["rand_a"][a0[k * n_comb + m]:a0[k * n_comb + m + 1]] for m in range(n_comb)])
    return cases


def ties_comb(pairs):
    """comb (n, 3) int32 and min_overlap (n,) for (metric, min_overlap) pairs: flag row 0, a similarity slot per metric-0 row
    (compute_aos is on for metric 0, as in eval_class).  Returns comb, min_overlap, n_slots."""
    comb, slots = [], 0
    for metric, _ in pairs:
        comb.append((int(metric), 0, slots if int(metric) == 0 else -1))
        slots += int(metric) == 0
    return np.array(comb, np.int32).reshape(-1, 3), np.array([mo for _, mo in pairs], np.float64), slots


def ties_pack(cases):
    """The cases as the images of one evaluator load: (packed, flags, overlaps).  One flag row with the cases' flags
    concatenated; overlaps (3, P) float64 holds every case's matrix under all three metrics."""
    nd = np.array([c["ovl"].shape[0] for c in cases], np.int64)
    ng = np.array([c["ovl"].shape[1] for c in cases], np.int64)
    ndc = np.array([len(c["dc_box"]) for c in cases], np.int64)
    off = lambda v, t: np.concatenate([[0], np.cumsum(v)]).astype(t)                              # noqa: E731
    cat = lambda k, w=None: np.ascontiguousarray(np.concatenate(                                  # noqa: E731
        [np.asarray(c[k], np.float64).reshape((-1,) if w is None else (-1, w)) for c in cases], 0))
    packed = {"n_img": len(cases), "gt_off": off(ng, np.int32), "dt_off": off(nd, np.int32), "dc_off": off(ndc, np.int32),
              "pair_off": off(nd * ng, np.int64), "max_dt": int(nd.max()), "gt_alpha": cat("gt_alpha"), "dt_alpha": cat("dt_alpha"),
              "dt_score": cat("score"), "dt_box2d": cat("dt_box", 4), "dc_box": cat("dc_box", 4)}
    flags = {"gt": np.concatenate([c["ign_gt"] for c in cases]).astype(np.int8)[None],
             "dt": np.concatenate([c["ign_dt"] for c in cases]).astype(np.int8)[None]}
    flat = np.concatenate([c["ovl"].ravel() for c in cases]).astype(np.float64)
    return packed, flags, np.ascontiguousarray(np.stack([flat] * 3))


def ties_mode_a(ev, to_device, cases, pairs):
    """Mode A of all `cases` as one load of evaluator `ev` under every (metric, min_overlap) of `pairs`: per case and pair the
    kernel's row of that image compacted by != NO_DETECTION, i.e. the matched scores in ground-truth order."""
    packed, flags, ovl = ties_pack(cases)
    ev.load(packed, flags)
    comb, mo, _ = ties_comb(pairs)
    scores = np.asarray(ev.match_scores(to_device(ovl), comb, mo))
    off = packed["gt_off"]
    return [[row[off[i]:off[i + 1]][row[off[i]:off[i + 1]] != -1e7] for row in scores] for i in range(len(cases))]


def ties_mode_b(ev, to_device, cases, pairs, thr):
    """Mode B of all `cases` as one load: counts (pairs, thresholds, 3) summed over the cases and the similarity sums
    (metric-0 pairs, thresholds), every pair at the thresholds `thr`."""
    packed, flags, ovl = ties_pack(cases)
    ev.load(packed, flags)
    comb, mo, n_slots = ties_comb(pairs)
    return ev.match_counts(to_device(ovl), comb, mo, [np.asarray(thr, np.float64)] * len(comb), n_slots)


@functools.lru_cache(maxsize=None)
def ties_scene():
    """The end-to-end scene with duplicate scores: the `scene_*` keys of eval_ties.npz without the prefix."""
    return {k[len("scene_"):]: v for k, v in load("eval_ties.npz").items() if k.startswith("scene_")}
