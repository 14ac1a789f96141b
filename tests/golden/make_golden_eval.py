"""Generates the KITTI-AP fixtures (eval_pairs.npz, eval_scene.npz, eval_scene/) by RUNNING THE REFERENCE'S OWN EVALUATOR
(DGDE/data/datasets/evaluation/kitti_object_eval_python, imported from /root/reference) on the CPU.

Run in the build container only (`python tests/golden/make_golden_eval.py`).  Nothing of the reference is copied; the files
written hold data only.  What has to be supplied for its modules to run here:
  * numba and fire are not installed.  `numba.jit` / `numba.cuda.jit` become identity decorators, `numba.cuda.local.array`
    returns a float32 numpy array of the requested shape (so a ninth intersection vertex raises IndexError instead of
    overflowing silently), `fire` and `skimage.io` are empty modules.
  * `rotate_iou_gpu_eval` launches a CUDA kernel.  It alone is replaced, in `rotate_iou` and in `eval`, by a loop that calls
    the reference's own device function per pair on float32 arrays, `devRotateIoUEval(query[k], boxes[n], criterion)` (the
    argument order of rotate_iou.py:295-296), and casts back as rotate_iou.py:333 does.
Everything else of eval.py, evaluate.py and kitti_common.py runs unmodified as plain Python.

The exact rotated intersection (`exact_bev`, `exact_3d`) is this file's own float64 Sutherland-Hodgman clipping on the
float32-rounded inputs; E_ref = max |reference - exact| over every pair and metric of eval_pairs.npz is the yardstick of
tests/test_gpu_eval.py.  The generator re-seeds until: no pair has more than 8 vertices, every reference overlap of the scene
is at least 8 E_ref away from 0.7 / 0.5 / 0.25, no two detections of an image share a score, and some class has a 3-D AP
strictly between 20 and 80.
"""
import math
import os
import shutil
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_EVAL = "/root/reference/DGDE/data/datasets/evaluation"
sys.path.insert(0, ROOT)

from dcd_amd.eval import synthetic  # noqa: E402

ANNO_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


def install_stubs():
    def _jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    class _Local:
        @staticmethod
        def array(shape, dtype=None):
            return np.zeros(shape, np.float32)

    nb = types.ModuleType("numba")
    cuda = types.ModuleType("numba.cuda")
    nb.jit = nb.njit = cuda.jit = _jit
    nb.float32 = np.float32
    cuda.local = cuda.shared = _Local
    nb.cuda = cuda
    sys.modules.update({"numba": nb, "numba.cuda": cuda, "fire": types.ModuleType("fire")})
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    sys.modules.setdefault("skimage", sk)
    sys.modules.setdefault("skimage.io", sk.io)


def load_reference():
    install_stubs()
    sys.path.insert(0, REF_EVAL)
    import kitti_object_eval_python.rotate_iou as R
    import kitti_object_eval_python.kitti_common as K
    import kitti_object_eval_python.evaluate as V

    def rotate_iou(boxes, query_boxes, criterion=-1, device_id=0):
        b32, q32 = boxes.astype(np.float32), query_boxes.astype(np.float32)
        iou = np.zeros((len(b32), len(q32)), np.float32)
        for n in range(len(b32)):
            for k in range(len(q32)):
                iou[n, k] = R.devRotateIoUEval(q32[k], b32[n], criterion)
        return iou.astype(boxes.dtype)

    R.rotate_iou_gpu_eval = rotate_iou
    import kitti_object_eval_python.eval as E
    E.rotate_iou_gpu_eval = rotate_iou
    return R, E, K, V


# ---- exact rotated-rectangle intersection, float64 -------------------------------------------------------------------
def corners64(r):
    c, s = math.cos(r[4]), math.sin(r[4])
    x, y = r[2] / 2, r[3] / 2
    return [(c * px + s * py + r[0], -s * px + c * py + r[1]) for px, py in ((-x, -y), (-x, y), (x, y), (x, -y))]


def area2(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))


def clip_area(subj, cl):
    if area2(cl) < 0:
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
    return abs(area2(out)) / 2 if len(out) > 2 else 0.0


def exact_overlaps(d, g):
    """(bev IoU, 3-D IoU, bev intersection area) [dt, gt] in float64 on the float32-rounded BEV boxes."""
    def bev(a):
        return np.concatenate([a["location"][:, [0, 2]], a["dimensions"][:, [0, 2]], a["rotation_y"][:, None]],
                              1).astype(np.float32).astype(np.float64)
    db, gb = bev(d), bev(g)
    nd, ng = len(db), len(gb)
    inter = np.zeros((nd, ng))
    for i in range(nd):
        ci = corners64(db[i])
        for k in range(ng):
            inter[i, k] = clip_area(corners64(gb[k]), ci)
    a_d, a_g = db[:, 2] * db[:, 3], gb[:, 2] * gb[:, 3]
    iou = inter / (a_d[:, None] + a_g[None] - inter)
    yd, hd, yg, hg = d["location"][:, 1], d["dimensions"][:, 1], g["location"][:, 1], g["dimensions"][:, 1]
    ih = np.minimum(yd[:, None], yg[None]) - np.maximum((yd - hd)[:, None], (yg - hg)[None])
    inc = np.where((inter > 0) & (ih > 0), ih * inter, 0.0)
    vd, vg = d["dimensions"].prod(1), g["dimensions"].prod(1)
    return iou, inc / (vd[:, None] + vg[None] - inc), inter


def reference_overlaps(E, gts, dts):
    """Per image the reference's three [dt, gt] matrices (the call of eval.py:473)."""
    return [E.calculate_iou_partly(dts, gts, m, 100)[0] for m in range(3)]


def pack(annos, prefix, out):
    out[prefix + "_count"] = np.array([len(a["name"]) for a in annos], np.int64)
    for k in ANNO_KEYS:
        if k in annos[0]:
            out["%s_%s" % (prefix, k)] = np.concatenate([np.asarray(a[k]) for a in annos], 0)


def label_lines(g):
    lines = []
    for i in range(len(g["name"])):
        l, h, w = g["dimensions"][i]
        v = [g["truncated"][i], g["alpha"][i], *g["bbox"][i], h, w, l, *g["location"][i], g["rotation_y"][i]]
        lines.append("%s %.2f %d " % (g["name"][i], v[0], g["occluded"][i]) + " ".join("%.2f" % x for x in v[1:]))
    return "".join(s + "\n" for s in lines)


def detection_rows(d):
    cls = np.array([synthetic.NAMES.index(s) for s in d["name"]], np.float64)
    l, h, w = d["dimensions"].T.reshape(3, -1)
    return np.concatenate([cls[:, None], d["alpha"][:, None], d["bbox"], h[:, None], w[:, None], l[:, None], d["location"],
                           d["rotation_y"][:, None], d["score"][:, None]], 1).astype(np.float32)


# ---- eval_pairs.npz --------------------------------------------------------------------------------------------------
def make_pairs(E, seed):
    rng = np.random.RandomState(seed)
    g0, d0 = synthetic.random_boxes(rng, 30), synthetic.random_boxes(rng, 24)
    g0.update(name=np.array(["Car"] * 30, "<U16"), truncated=np.zeros(30), occluded=np.zeros(30, np.int64))
    d0.update(name=np.array(["Car"] * 24, "<U16"), truncated=np.zeros(24), occluded=np.zeros(24, np.int64),
              score=rng.uniform(0.05, 1, 24))
    # 130 x 70: detections are noisy copies of the ground truth (up to four per box) so that the sequential assignment has
    # competing candidates, plus unrelated boxes
    g1 = synthetic.make_gt(rng, 70)
    parts = [synthetic.make_dt(rng, g1, keep_p=0.7, max_fp=0) for _ in range(4)]
    d1 = {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}
    n = len(d1["name"])
    assert n >= 130, n
    sel = rng.permutation(n)[:112]
    d1 = {k: v[sel] for k, v in d1.items()}
    extra = synthetic.random_boxes(rng, 18)
    extra.update(name=np.array(["Car"] * 18, "<U16"), truncated=np.zeros(18), occluded=np.zeros(18, np.int64),
                 score=rng.uniform(0.05, 1, 18))
    d1 = {k: np.concatenate([d1[k], extra[k]], 0) for k in d1}
    e = synthetic.empty_anno
    gts = [g0, e(), g1, synthetic.make_gt(rng, 5), e()]
    dts = [d0, make_nonempty_dt(rng, 7), d1, e(True), e(True)]
    for d in dts:
        assert len(np.unique(d["score"])) == len(d["score"])
    ref = reference_overlaps(E, gts, dts)
    out = {}
    pack(gts, "gt", out)
    pack(dts, "dt", out)
    e_ref = 0.0
    for i, (g, d) in enumerate(zip(gts, dts)):
        ex_bev, ex_3d, ex_inter = exact_overlaps(d, g)
        out["exact_bev_%d" % i], out["exact_3d_%d" % i], out["exact_inter_%d" % i] = ex_bev, ex_3d, ex_inter
        for m in range(3):
            out["ref_%d_%d" % (m, i)] = ref[m][i]
        if ex_bev.size:
            e_ref = max(e_ref, np.abs(ref[1][i] - ex_bev).max(), np.abs(ref[2][i] - ex_3d).max())
    out["E_ref"] = np.float64(e_ref)
    # the 130 x 70 image through compute_statistics_jit: class Car, difficulty hard, min overlap 0.5, five thresholds
    g, d = gts[2], dts[2]
    _, ig, idt, dc = E.clean_data(g, d, 0, 2)
    dc = np.stack(dc, 0).astype(np.float64) if len(dc) else np.zeros((0, 4))
    gt_data = np.concatenate([g["bbox"], g["alpha"][:, None]], 1)
    dt_data = np.concatenate([d["bbox"], d["alpha"][:, None], d["score"][:, None]], 1)
    thr = np.array([0.0, 0.2, 0.45, 0.7, 0.9])
    for m in range(3):
        a = E.compute_statistics_jit(ref[m][2], gt_data, dt_data, np.array(ig), np.array(idt), dc, m, 0.5, 0.0, False)
        out["big_scores_%d" % m] = np.sort(a[4])
        rows = [E.compute_statistics_jit(ref[m][2], gt_data, dt_data, np.array(ig), np.array(idt), dc, m, 0.5, t, True,
                                         m == 0)[:4] for t in thr]
        out["big_pr_%d" % m] = np.array(rows, np.float64)
    out["big_thresholds"] = thr
    out["big_ignored_gt"], out["big_ignored_dt"] = np.array(ig, np.int8), np.array(idt, np.int8)
    assert len(out["big_scores_0"]) > 5 and out["big_pr_0"][0, 0] > 0 and len(dc) > 0
    return out


def make_nonempty_dt(rng, n):
    d = synthetic.random_boxes(rng, n)
    d.update(name=np.array(["Car"] * n, "<U16"), truncated=np.zeros(n), occluded=np.zeros(n, np.int64),
             score=rng.uniform(0.05, 1, n))
    return d


# ---- eval_scene ------------------------------------------------------------------------------------------------------
def make_scene(E, K, V, seed, e_ref, folder):
    rng = np.random.RandomState(seed)
    n_img = 16
    gts, dts = synthetic.make_scene(rng, n_img, empty_gt=(5,), empty_dt=(9,))
    ids = ["%06d" % (i * 3 + 1) for i in range(n_img)]
    if os.path.isdir(folder):
        shutil.rmtree(folder)
    os.makedirs(os.path.join(folder, "label_2"))
    os.makedirs(os.path.join(folder, "pred"))
    with open(os.path.join(folder, "val.txt"), "w") as f:
        f.write("".join(i + "\n" for i in ids))
    rows = [detection_rows(d) for d in dts]
    for i, g, r in zip(ids, gts, rows):
        with open(os.path.join(folder, "label_2", i + ".txt"), "w") as f:
            f.write(label_lines(g))
        V.generate_kitti_3d_detection(torch.from_numpy(r), os.path.join(folder, "pred", i + ".txt"))
    gts = K.get_label_annos(os.path.join(folder, "label_2"), ids)
    dts = K.get_label_annos(os.path.join(folder, "pred"), ids)
    names = set(np.concatenate([g["name"] for g in gts]).tolist())
    if names != {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Dontcare"}:
        return None, "names %s" % sorted(names)
    for d in dts:
        if len(np.unique(d["score"])) != len(d["score"]):
            return None, "duplicate score"
    ref = reference_overlaps(E, gts, dts)
    flat = np.concatenate([o.ravel() for m in range(3) for o in ref[m]])
    clear = min(np.abs(flat - t).min() for t in (0.7, 0.5, 0.25))
    if clear < 8 * e_ref:
        return None, "clearance %g" % clear

    out = {"ids": np.array(ids), "clearance": np.float64(clear)}
    pack(gts, "gt", out)
    pack(dts, "dt", out)
    for i, r in enumerate(rows):
        out["rows_%d" % i] = r
    for m in range(3):
        for i in range(n_img):
            out["ref_%d_%d" % (m, i)] = ref[m][i]
    for c in range(3):
        for dif in range(3):
            flags = [E.clean_data(g, d, c, dif) for g, d in zip(gts, dts)]
            out["clean_%d_%d_num_valid" % (c, dif)] = np.int64(sum(f[0] for f in flags))
            out["clean_%d_%d_gt" % (c, dif)] = np.array(sum((f[1] for f in flags), []), np.int8)
            out["clean_%d_%d_dt" % (c, dif)] = np.array(sum((f[2] for f in flags), []), np.int8)
            out["clean_%d_%d_dc_count" % (c, dif)] = np.array([len(f[3]) for f in flags], np.int64)

    # record what eval_class hands to / gets from get_thresholds and fused_compute_statistics, in call order
    # (metric, class, difficulty, overlap row); 16 images are one part, so there is one fused call per combination
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
        out["min_overlaps"] = mo
        for m in range(3):
            ret = E.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], m, mo, compute_aos=(m == 0))
            for k in ("precision", "recall", "orientation"):
                out["%s_%d" % (k, m)] = ret[k]
    finally:
        E.get_thresholds, E.fused_compute_statistics = get_thresholds, fused
    ap3d = out["dict_values_R40"][[i for i, k in enumerate(out["dict_keys_R40"]) if "_3d_" in k]]
    if not ((ap3d > 20) & (ap3d < 80)).any():
        return None, "3-D APs %s" % np.round(ap3d, 1)
    return out, "ok"


def main():
    R, E, K, V = load_reference()
    seed = 0
    while True:
        try:
            pairs = make_pairs(E, seed)
            break
        except IndexError:
            print("pairs seed %d: more than 8 vertices, re-seeding" % seed)
            seed += 1
    e_ref = float(pairs["E_ref"])
    print("eval_pairs: seed %d, E_ref %.3g" % (seed, e_ref))
    pairs["seed"] = np.int64(seed)
    np.savez_compressed(os.path.join(HERE, "eval_pairs.npz"), **pairs)

    folder = os.path.join(HERE, "eval_scene")
    seed = 0
    while True:
        try:
            scene, why = make_scene(E, K, V, seed, e_ref, folder)
        except IndexError:
            scene, why = None, "more than 8 vertices"
        print("eval_scene: seed %d: %s" % (seed, why))
        if scene is not None:
            break
        seed += 1
    scene["seed"] = np.int64(seed)
    np.savez_compressed(os.path.join(HERE, "eval_scene.npz"), **scene)
    print(str(scene["text_R40"]))
    print("clearance %.3g = %.1f E_ref" % (scene["clearance"], scene["clearance"] / e_ref))


if __name__ == "__main__":
    main()
