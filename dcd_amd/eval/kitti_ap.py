"""KITTI average precision (bbox / BEV / 3-D / AOS, R40 and R11) with the overlaps and the matching on the device.

`official_eval` returns what the reference's `get_official_eval_result` returns (DGDE/data/datasets/evaluation/
kitti_object_eval_python/eval.py:646-728) and `evaluate` mirrors evaluate.py:14-31.  The split of the work:

  host, vectorised numpy   the ignore flags of `clean_data` (eval.py:28-81), which depend on (class, difficulty) only, as
                           int8 (classes x difficulties, boxes) tables; packing all images into concatenated arrays with
                           per-image offset tables
  device, one launch       `dcd_eval_overlaps`: the three overlap metrics of every image's own detection x ground-truth block
  device, one launch       `dcd_eval_match` mode A: per combination (metric, class, difficulty, overlap row) and ground-truth
                           box the score of the detection assigned to it
  host                     `get_thresholds` (eval.py:7-25), a short sequential loop per combination
  device, two launches     `dcd_eval_match` mode B: tp / fp / fn per combination and threshold, AOS similarity per image, then
                           `dcd_eval_sum_similarity` over the image axis in a fixed order
  host                     precision / recall / AOS with the running maximum (eval.py:537-547), mAP, the result text

There is no CPU path: a non-GPU device raises `_lib.DcdHipError`.
"""
import ctypes

import numpy as np

from dcd_amd import _lib
from dcd_amd.eval import kitti_annos

CLASS_NAMES = ("car", "pedestrian", "cyclist", "van", "person_sitting", "truck")        # eval.py:29
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "Truck"}
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
DIFFICULTIES = (0, 1, 2)
N_SAMPLE_PTS = 41
NO_DETECTION = -10000000.0
# [overlap row, metric, class]: eval.py:647-655
MIN_OVERLAPS = np.stack([np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3),
                         np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5],
                                   [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])], axis=0)


# ---- host stages -----------------------------------------------------------------------------------------------------
def _cat(annos, key, width=None):
    shape = (0,) if width is None else (0, width)
    parts = [np.asarray(a[key], np.float64).reshape((-1,) + shape[1:]) for a in annos]
    return np.concatenate(parts, 0) if parts else np.zeros(shape)


def _names(annos):
    return np.array([str(s) for a in annos for s in a["name"]], dtype=str).reshape(-1)


def _offsets(counts, dtype):
    return np.concatenate([[0], np.cumsum(counts)]).astype(dtype)


def ignore_flags(gt_annos, dt_annos, classes, difficulties=DIFFICULTIES):
    """`clean_data` for every (class, difficulty) at once.  Returns a dict: 'gt' (R, G) and 'dt' (R, D) int8 with row
    r = class index * len(difficulties) + difficulty index, 'num_valid' (R,) int64, 'dontcare' (G,) bool."""
    gt_name, dt_name = _names(gt_annos), _names(dt_annos)
    gt_lower, dt_lower = np.char.lower(gt_name) if gt_name.size else gt_name, np.char.lower(dt_name) if dt_name.size else dt_name
    gt_box, dt_box = _cat(gt_annos, "bbox", 4), _cat(dt_annos, "bbox", 4)
    occluded, truncated = _cat(gt_annos, "occluded"), _cat(gt_annos, "truncated")
    gt_height = gt_box[:, 3] - gt_box[:, 1]
    dt_height = np.abs(dt_box[:, 3] - dt_box[:, 1])
    rows_gt, rows_dt = [], []
    for c in classes:
        cur = CLASS_NAMES[c]
        neighbour = {"pedestrian": "person_sitting", "car": "van"}.get(cur)
        valid = np.where(gt_lower == cur, 1, np.where(gt_lower == neighbour, 0, -1)) if neighbour else \
            np.where(gt_lower == cur, 1, -1)
        valid = np.broadcast_to(valid, gt_height.shape)
        for d in difficulties:
            ignore = (occluded > MAX_OCCLUSION[d]) | (truncated > MAX_TRUNCATION[d]) | (gt_height <= MIN_HEIGHT[d])
            rows_gt.append(np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | (ignore & (valid == 1)), 1, -1)))
            rows_dt.append(np.where(dt_height < MIN_HEIGHT[d], 1, np.where(dt_lower == cur, 0, -1)))
    n_rows = len(rows_gt)
    gt = np.array(rows_gt, np.int8).reshape(n_rows, len(gt_height))
    dt = np.array(rows_dt, np.int8).reshape(n_rows, len(dt_height))
    return {"gt": gt, "dt": dt, "num_valid": (gt == 0).sum(1).astype(np.int64),
            "dontcare": (gt_name == "DontCare") if gt_name.size else np.zeros(0, bool)}


def pack(gt_annos, dt_annos, dontcare):
    """All images as concatenated float64 arrays with per-image offset tables (the layout of include/dcd_hip.h)."""
    assert len(gt_annos) == len(dt_annos)
    n_gt = np.array([len(a["name"]) for a in gt_annos], np.int64)
    n_dt = np.array([len(a["name"]) for a in dt_annos], np.int64)
    gt_off = _offsets(n_gt, np.int32)

    def box3d(annos):
        return np.ascontiguousarray(np.concatenate([_cat(annos, "location", 3), _cat(annos, "dimensions", 3),
                                                    _cat(annos, "rotation_y")[:, None]], 1))
    gt_box2d = _cat(gt_annos, "bbox", 4)
    n_dc = np.array([int(dontcare[gt_off[i]:gt_off[i + 1]].sum()) for i in range(len(gt_annos))], np.int64)
    return {"n_img": len(gt_annos), "gt_off": gt_off, "dt_off": _offsets(n_dt, np.int32), "dc_off": _offsets(n_dc, np.int32),
            "pair_off": _offsets(n_gt * n_dt, np.int64), "max_dt": int(n_dt.max()) if len(n_dt) else 0,
            "gt_box2d": gt_box2d, "dt_box2d": _cat(dt_annos, "bbox", 4), "gt_box3d": box3d(gt_annos), "dt_box3d": box3d(dt_annos),
            "gt_alpha": _cat(gt_annos, "alpha"), "dt_alpha": _cat(dt_annos, "alpha"), "dt_score": _cat(dt_annos, "score"),
            "dc_box": np.ascontiguousarray(gt_box2d[dontcare])}


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """eval.py:7-25 with its float arithmetic: Python-float recalls and the accumulated `current_recall`."""
    scores = np.sort(np.asarray(scores, np.float64))[::-1]
    current_recall = 0
    thresholds = []
    n = len(scores)
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def combinations(n_class, compute_aos, min_overlaps, n_diff=len(DIFFICULTIES)):
    """The (metric, class, difficulty, overlap row) loop nest of do_eval / eval_class, in that order.  Returns comb (n, 3)
    int32 [metric, flag row, similarity slot or -1], min_overlap (n,) float64 and the number of slots."""
    comb, mo, slots = [], [], 0
    for metric in range(3):
        for m in range(n_class):
            for l in range(n_diff):
                for k in range(min_overlaps.shape[0]):
                    slot = -1
                    if metric == 0 and compute_aos:
                        slot, slots = slots, slots + 1
                    comb.append((metric, m * n_diff + l, slot))
                    mo.append(min_overlaps[k, metric, m])
    return np.array(comb, np.int32).reshape(-1, 3), np.array(mo, np.float64), slots


def curves_from_pr(pr_tables, n_class, n_overlap, compute_aos, n_diff=len(DIFFICULTIES)):
    """eval.py:537-547 for one metric: `pr_tables` holds the (thresholds, 4) tp fp fn similarity table of every
    (class, difficulty, overlap row) in loop order.  Returns precision, recall, orientation (n_class, n_diff, n_overlap, 41)."""
    shape = [n_class, n_diff, n_overlap, N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    it = iter(pr_tables)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(n_class):
            for l in range(n_diff):
                for k in range(n_overlap):
                    pr = np.asarray(next(it), np.float64).reshape(-1, 4)
                    n = len(pr)
                    recall[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
                    if compute_aos:
                        aos[m, l, k, :n] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
                    for i in range(n):
                        precision[m, l, k, i] = np.max(precision[m, l, k, i:], axis=-1)
                        recall[m, l, k, i] = np.max(recall[m, l, k, i:], axis=-1)
                        if compute_aos:
                            aos[m, l, k, i] = np.max(aos[m, l, k, i:], axis=-1)
    return precision, recall, aos


def get_mAP(prec):                       # eval.py:556-560
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):                   # eval.py:563-568
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def has_alpha(dt_annos):
    """eval.py:678-684: AOS is computed unless the first non-empty detection set carries the -10 placeholder."""
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(anno["alpha"][0] != -10)
    return False


def resolve_classes(classes):
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    if not isinstance(classes, (list, tuple)):
        classes = [classes]
    return [name_to_class[c] if isinstance(c, str) else int(c) for c in classes]


def format_result(classes, min_overlaps, mAPbbox, mAPbev, mAP3d, mAPaos):
    """The text and dict of eval.py:689-728.  min_overlaps is already restricted to `classes`."""
    result, ret = "", {}
    for j, c in enumerate(classes):
        name = CLASS_TO_NAME[c]
        for i in range(min_overlaps.shape[0]):
            result += "{} AP@{:.2f}, {:.2f}, {:.2f}:\n".format(name, *min_overlaps[i, :, j])
            result += f"bbox AP:{mAPbbox[j, 0, i]:.4f}, {mAPbbox[j, 1, i]:.4f}, {mAPbbox[j, 2, i]:.4f}\n"
            result += f"bev  AP:{mAPbev[j, 0, i]:.4f}, {mAPbev[j, 1, i]:.4f}, {mAPbev[j, 2, i]:.4f}\n"
            result += f"3d   AP:{mAP3d[j, 0, i]:.4f}, {mAP3d[j, 1, i]:.4f}, {mAP3d[j, 2, i]:.4f}\n"
            if mAPaos is not None:
                result += f"aos  AP:{mAPaos[j, 0, i]:.2f}, {mAPaos[j, 1, i]:.2f}, {mAPaos[j, 2, i]:.2f}\n"
                if i == 0:
                    for d, level in enumerate(("easy", "moderate", "hard")):
                        ret["%s_aos/%s" % (name, level)] = mAPaos[j, d, 0]
            for d, level in enumerate(("easy", "moderate", "hard")):
                ret["{}_3d_{:.2f}/{}".format(name, min_overlaps[i, 1, j], level)] = mAP3d[j, d, i]
            for d, level in enumerate(("easy", "moderate", "hard")):
                ret["{}_bev_{:.2f}/{}".format(name, min_overlaps[i, 2, j], level)] = mAPbev[j, d, i]
            for d, level in enumerate(("easy", "moderate", "hard")):
                ret["{}_image/{}".format(name, level)] = mAPbbox[j, d, 0]
    return result, ret


def result_from_pr(pr_by_metric, classes, metric="R40", compute_aos=True, detail=None, curves=None):
    """The table stage: per metric the pr tables of every (class, difficulty, overlap row) -> (text, dict)."""
    if metric not in ("R40", "R11"):
        raise ValueError(metric)
    classes = resolve_classes(classes)
    min_overlaps = MIN_OVERLAPS[:, :, classes]
    mAP = get_mAP_R40 if metric == "R40" else get_mAP
    out = [curves_from_pr(pr_by_metric[m], len(classes), min_overlaps.shape[0], compute_aos and m == 0) for m in range(3)]
    if curves is not None:
        curves.extend(out)
    if detail is not None:
        detail["bbox"], detail["bev"], detail["3d"] = out[0][0], out[1][0], out[2][0]
        if compute_aos:
            detail["aos"] = out[0][2]
    return format_result(classes, min_overlaps, mAP(out[0][0]), mAP(out[1][0]), mAP(out[2][0]),
                         mAP(out[0][2]) if compute_aos else None)


# ---- device stages ---------------------------------------------------------------------------------------------------
class KittiEvaluator:
    """Holds one split on the device and runs the kernels of csrc/eval.hip on it."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DcdHipError("the KITTI evaluator runs on the GPU only (got device %s); there is no CPU path" % self.device)
        self.lib = _lib.lib()
        self.t = {}

    def _up(self, array):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def load(self, packed, flags):
        self.n_img, self.max_dt = packed["n_img"], packed["max_dt"]
        if self.n_img == 0:
            raise ValueError("no images to evaluate")
        self.t = {k: self._up(v) for k, v in packed.items() if isinstance(v, np.ndarray)}
        self.t["ign_gt"], self.t["ign_dt"] = self._up(flags["gt"]), self._up(flags["dt"])
        self.n_rows = flags["gt"].shape[0]
        self.G, self.D, self.n_dc = int(packed["gt_off"][-1]), int(packed["dt_off"][-1]), int(packed["dc_off"][-1])
        self.P = int(packed["pair_off"][-1])

    def overlaps(self):
        """(3, P) float64 on the device: bbox, BEV, 3-D overlaps of every image's [dt, gt] block."""
        import torch
        t = self.t
        out = torch.empty((3, self.P), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.dcd_eval_overlaps(_lib.stream_of(out), self.n_img, _lib.ptr(t["gt_off"]), _lib.ptr(t["dt_off"]),
                                              _lib.ptr(t["pair_off"]), self.G, self.D, self.P, _lib.ptr(t["gt_box2d"]),
                                              _lib.ptr(t["dt_box2d"]), _lib.ptr(t["gt_box3d"]), _lib.ptr(t["dt_box3d"]),
                                              _lib.ptr(out)), "dcd_eval_overlaps")
        return out

    def _args(self, mode, overlaps, comb, min_overlap):
        t = self.t
        import torch
        if overlaps.dtype != torch.float64 or tuple(overlaps.shape) != (3, self.P) or not overlaps.is_contiguous():
            raise _lib.DcdHipError("overlaps must be a contiguous (3, %d) float64 tensor" % self.P)
        _lib.require_cuda(overlaps)
        a = _lib.EvalMatchArgs(mode=mode, n_img=self.n_img, n_comb=len(comb), n_rows=self.n_rows, G=self.G, D=self.D,
                               n_dc=self.n_dc, max_dt=self.max_dt, T=0, n_slots=0, P=self.P)
        keep = [self._up(comb.astype(np.int32)), self._up(min_overlap.astype(np.float64))]
        a.comb, a.min_overlap = _lib.ptr(keep[0]), _lib.ptr(keep[1])
        a.overlaps = _lib.ptr(overlaps)
        for k in ("gt_off", "dt_off", "dc_off", "pair_off", "ign_gt", "ign_dt", "dt_score", "gt_alpha", "dt_alpha", "dt_box2d",
                  "dc_box"):
            setattr(a, k, _lib.ptr(t[k]))
        return a, keep

    def match_scores(self, overlaps, comb, min_overlap):
        """Mode A: (n_comb, G) float64 numpy, the score of the detection matched to each ground-truth box or -1e7."""
        import torch
        a, keep = self._args(0, overlaps, comb, min_overlap)
        scores = torch.empty((len(comb), self.G), dtype=torch.float64, device=self.device)
        a.scores = _lib.ptr(scores)
        _lib.check(self.lib.dcd_eval_match(_lib.stream_of(scores), ctypes.byref(a)), "dcd_eval_match")
        return scores.cpu().numpy()

    def match_counts(self, overlaps, comb, min_overlap, thresholds, n_slots):
        """Mode B: thresholds is a list of arrays, one per combination.  Returns counts (n_comb, T, 3) int64 numpy and the
        similarity sums (n_slots, T) float64 numpy."""
        import torch
        a, keep = self._args(1, overlaps, comb, min_overlap)
        T = max(1, max(len(t) for t in thresholds))
        table = np.zeros((len(comb), T), np.float64)
        for i, t in enumerate(thresholds):
            table[i, :len(t)] = t
        keep += [self._up(table), self._up(np.array([len(t) for t in thresholds], np.int32))]
        counts = torch.zeros((len(comb), T, 3), dtype=torch.int32, device=self.device)
        sim_part = torch.empty((self.n_img, n_slots, T), dtype=torch.float64, device=self.device)
        sim = torch.zeros((n_slots, T), dtype=torch.float64, device=self.device)
        a.T, a.n_slots = T, n_slots
        a.thresholds, a.n_thresh, a.counts, a.sim_part = (_lib.ptr(keep[2]), _lib.ptr(keep[3]), _lib.ptr(counts),
                                                          _lib.ptr(sim_part))
        stream = _lib.stream_of(counts)
        _lib.check(self.lib.dcd_eval_match(stream, ctypes.byref(a)), "dcd_eval_match")
        _lib.check(self.lib.dcd_eval_sum_similarity(stream, _lib.ptr(sim_part), self.n_img, n_slots * T, _lib.ptr(sim)),
                   "dcd_eval_sum_similarity")
        return counts.cpu().numpy().astype(np.int64), sim.cpu().numpy()


def pr_tables(evaluator, overlaps, n_class, compute_aos, min_overlaps, num_valid, stages=None):
    """Modes A and B for every combination: per metric the list of (thresholds, 4) tables in loop order."""
    comb, mo, n_slots = combinations(n_class, compute_aos, min_overlaps)
    scores = evaluator.match_scores(overlaps, comb, mo)
    matched = [row[row != NO_DETECTION] for row in scores]
    thresholds = [np.array(get_thresholds(s, num_valid[comb[i, 1]]), np.float64) for i, s in enumerate(matched)]
    counts, sim = evaluator.match_counts(overlaps, comb, mo, thresholds, n_slots)
    if stages is not None:
        stages.update(comb=comb, min_overlap=mo, scores=matched, thresholds=thresholds, counts=counts, similarity=sim)
    by_metric = [[], [], []]
    for i, (metric, _, slot) in enumerate(comb):
        n = len(thresholds[i])
        pr = np.zeros((n, 4))
        pr[:, :3] = counts[i, :n]
        if slot >= 0:
            pr[:, 3] = sim[slot, :n]
        by_metric[metric].append(pr)
    return by_metric


def official_eval(gt_annos, dt_annos, classes, metric="R40", device="cuda:0", detail=None, stages=None):
    """(text, dict) of `get_official_eval_result(gt_annos, dt_annos, classes, PR_detail_dict=detail, metric=metric)`."""
    if metric not in ("R40", "R11"):
        raise ValueError(metric)
    evaluator = KittiEvaluator(device)
    classes = resolve_classes(classes)
    min_overlaps = MIN_OVERLAPS[:, :, classes]
    compute_aos = has_alpha(dt_annos)
    flags = ignore_flags(gt_annos, dt_annos, classes)
    evaluator.load(pack(gt_annos, dt_annos, flags["dontcare"]), flags)
    by_metric = pr_tables(evaluator, evaluator.overlaps(), len(classes), compute_aos, min_overlaps, flags["num_valid"], stages)
    curves = [] if stages is not None else None
    out = result_from_pr(by_metric, classes, metric, compute_aos, detail, curves)
    if stages is not None:
        stages["curves"] = curves
    return out


def evaluate(label_path, result_path, label_split_file, current_class=0, metric="R40", device="cuda:0"):
    """evaluate.py:14-31 without the coco and score-threshold branches."""
    ids = kitti_annos.read_imageset(label_split_file)
    dt_annos = kitti_annos.read_annos(result_path, ids)
    gt_annos = kitti_annos.read_annos(label_path, ids)
    return official_eval(gt_annos, dt_annos, current_class, metric=metric, device=device)
