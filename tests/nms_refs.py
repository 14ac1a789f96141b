"""Float64 restatement of the box NMS on decoded detections (DESIGN.md "Box NMS"; include/dcd_hip.h, dcd_nms_detections), written
from the rules and not from csrc/nms_math.h: numpy only.  TEST INFRASTRUCTURE.

  overlap_matrix    the three overlaps of KITTI's evaluator between the rows of one image, the exact polygon area by
                    Sutherland-Hodgman in float64 (the inputs are the float32 rows; every operation after that is float64)
  nms_image         candidates, visit order, the greedy rule and the output order for one image block
  nms_batch         the same over (B K, .) arrays: what the kernel must return, bit for bit
  build_scene       seeded blocks of clustered boxes under the MARGIN CONDITION: a scene in which some pairwise overlap, in any of
                    the three modes, lies within `MARGIN` of the threshold is drawn again, so that a decision never hangs on the
                    last bits of an overlap and kept sets can be compared exactly; and for every image with two candidates or
                    more the oracle alone must suppress at least a quarter and keep at least a quarter of them in every mode,
                    class-aware and agnostic (an assertion: a kernel that keeps everything, or nothing, cannot pass)

A row's class is the integer part of column 0 (what `write_detections` names it by; the decode leaves the top-K's fraction there).
Row layout (`write_detections`): 0 class | 1 alpha | 2:6 box | 6:9 h w l | 9:12 x y z | 12 ry | 13 score.
"""
import numpy as np

MODES = ("2d", "bev", "3d")
MARGIN = 1e-4


# ---- overlaps -------------------------------------------------------------------------------------------------------------------
def _clip(poly, axis, sign, lim):
    """Convex polygon (list of (x, y)) cut to sign * p[axis] <= lim."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        dp, dq = sign * p[axis], sign * q[axis]
        if dp <= lim:
            out.append(p)
        if (dp <= lim) != (dq <= lim):
            t = (lim - dp) / (dq - dp)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def rotated_intersection(q, b):
    """Area shared by the BEV rectangles of rows q and b: (x, z) centre, l along the box's own x, w along its z, yaw ry in
    KITTI's sense (a corner (px, pz) of the box lies at (cos ry px + sin ry pz, -sin ry px + cos ry pz) from the centre)."""
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    d = np.hypot(b[9] - q[9], b[11] - q[11])
    if d > (np.hypot(q[8], q[7]) + np.hypot(b[8], b[7])) / 2:           # the circumscribed circles are apart: exactly 0
        return 0.0
    cb, sb, cq, sq = np.cos(b[12]), np.sin(b[12]), np.cos(q[12]), np.sin(q[12])
    poly = []
    for px, pz in ((-b[8] / 2, -b[7] / 2), (-b[8] / 2, b[7] / 2), (b[8] / 2, b[7] / 2), (b[8] / 2, -b[7] / 2)):
        wx, wz = b[9] + cb * px + sb * pz - q[9], b[11] - sb * px + cb * pz - q[11]       # the corner, from q's centre
        poly.append((cq * wx - sq * wz, sq * wx + cq * wz))                               # ... in q's own axes
    for axis, lim in ((0, abs(q[8]) / 2), (1, abs(q[7]) / 2)):
        for sign in (1.0, -1.0):
            poly = _clip(poly, axis, sign, lim)
            if len(poly) < 3:
                return 0.0
    x, y = np.array([p[0] for p in poly]), np.array([p[1] for p in poly])
    return abs(float(np.dot(x, np.roll(y, -1)) - np.dot(np.roll(x, -1), y))) / 2


def overlap_2d(q, b):
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    iw = min(b[4], q[4]) - max(b[2], q[2])
    ih = min(b[5], q[5]) - max(b[3], q[3])
    if not (iw > 0 and ih > 0):
        return 0.0
    return iw * ih / ((b[4] - b[2]) * (b[5] - b[3]) + (q[4] - q[2]) * (q[5] - q[3]) - iw * ih)


def overlaps_of_pair(q, b):
    """(2d, bev, 3d) of the kept box q and the visited candidate b."""
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    inter = rotated_intersection(q, b)
    bev = inter / (q[8] * q[7] + b[8] * b[7] - inter)
    ih = min(b[10], q[10]) - max(b[10] - b[6], q[10] - q[6])
    d3 = 0.0
    if inter > 0 and ih > 0:
        d3 = inter * ih / (b[8] * b[6] * b[7] + q[8] * q[6] * q[7] - inter * ih)
    return overlap_2d(q, b), bev, d3


def visit_order(final_scores):
    """Indices in descending score; a tie to the lower index; NaN last (numpy's stable sort puts NaN after every number)."""
    return np.argsort(-np.asarray(final_scores, np.float64), kind="stable")


def overlap_matrix(rows, order=None):
    """(3, n, n) float64, symmetric, zero diagonal: element (i, j) with the one of the two visited first in the kept role."""
    rows = np.asarray(rows)
    n = len(rows)
    order = visit_order(rows[:, 13]) if order is None else order
    out = np.zeros((3, n, n))
    for r in range(n):
        for c in range(r + 1, n):
            i, j = order[r], order[c]
            out[:, i, j] = out[:, j, i] = overlaps_of_pair(rows[i], rows[j])
    return out


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def count_candidates(raw, det_threshold):
    below = ~(np.asarray(raw, np.float32) >= np.float32(det_threshold))     # float32 against the rounded threshold, as the host cuts
    return int(below.argmax()) if below.any() else len(below)


def nms_image(rows, raw, mode, thresh, det_threshold, class_agnostic, matrix=None):
    """One image block (K rows).  Returns dict(n, order, keep (K,) bool: survivors, suppressed (K,) bool, perm (K,): perm[d] =
    the input row that lands at output row d, matrix (3, n, n))."""
    rows, raw = np.asarray(rows), np.asarray(raw)
    K = len(rows)
    n = count_candidates(raw, det_threshold)
    order = visit_order(rows[:n, 13])
    if matrix is None:
        matrix = overlap_matrix(rows[:n], order)
    ovl = matrix[MODES.index(mode)]
    kept = []
    suppressed = np.zeros(K, bool)
    for i in order:
        hit = any(ovl[k, i] > thresh and (class_agnostic or np.trunc(rows[k, 0]) == np.trunc(rows[i, 0])) for k in kept)
        if hit:
            suppressed[i] = True
        else:
            kept.append(i)
    keep = np.zeros(K, bool)
    keep[kept] = True
    idx = np.arange(K)
    perm = np.concatenate([idx[keep], idx[suppressed], idx[n:]])
    return dict(n=n, order=order, keep=keep, suppressed=suppressed, perm=perm, matrix=matrix)


def nms_batch(rows, aux, k2, k3, K, mode, thresh, det_threshold, class_agnostic, matrices=None):
    """What dcd_nms_detections returns for (B K, .) arrays: (rows_out, aux_out, k2_out, k3_out, per-image results)."""
    rows, aux = np.asarray(rows), np.asarray(aux)
    B = len(rows) // K
    outs = [np.empty_like(a) if a is not None else None for a in (rows, aux, k2, k3)]
    results = []
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        res = nms_image(rows[sl], aux[sl, 0], mode, thresh, det_threshold, class_agnostic, None if matrices is None else matrices[b])
        for src, dst in zip((rows, aux, k2, k3), outs):
            if src is not None:
                dst[sl] = src[sl][res["perm"]]
        outs[1][sl][res["suppressed"][res["perm"]], 0] = -np.inf
        results.append(res)
    return outs[0], outs[1], outs[2], outs[3], results


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _draw_rows(rng, n):
    """n rows of clustered boxes: about half are objects of `eval.synthetic.random_boxes`, the rest jittered duplicates of them --
    mostly of the same class, some of another (a Pedestrian / Cyclist pair on one person), some lifted by more than their height
    (stacked: one BEV footprint, no shared volume)."""
    from dcd_amd.eval.synthetic import random_boxes
    n_base = max(1, (n + 1) // 2)
    g = random_boxes(rng, n_base)
    src = np.concatenate([np.arange(n_base), rng.randint(0, n_base, n - n_base)])
    dup = np.arange(n) >= n_base
    cls_base = rng.randint(0, 3, n_base)
    cls = cls_base[src]
    other = dup & (rng.rand(n) < 0.12)
    cls[other] = (cls[other] + 1 + rng.randint(0, 2, int(other.sum()))) % 3
    stacked = dup & ~other & (rng.rand(n) < 0.12)
    jit = lambda s, shape: np.where(dup.reshape((-1,) + (1,) * (len(shape) - 1)), rng.normal(0, s, shape), 0.0)  # noqa: E731
    box = g["bbox"][src] + jit(1.5, (n, 4))
    dims = g["dimensions"][src] + jit(0.03, (n, 3))                     # l h w
    loc = g["location"][src] + jit(0.08, (n, 3))
    loc[stacked, 1] -= dims[stacked, 1] + 0.3
    ry = g["rotation_y"][src] + jit(0.04, (n,))
    rows = np.zeros((n, 14), np.float32)
    rows[:, 0], rows[:, 1] = cls + rng.uniform(0, 0.98, n), g["alpha"][src]   # (the top-K's fraction: the class is the integer part)
    rows[:, 2:6] = box
    rows[:, 6], rows[:, 7], rows[:, 8] = dims[:, 1], dims[:, 2], dims[:, 0]
    rows[:, 9:12], rows[:, 12] = loc, ry
    return rows


def _quarter(n):
    return -(-n // 4)


def build_scene(seed, B, K, counts, nk, thresh=0.5, det_threshold=0.2, confidence=False):
    """counts: candidates of every image.  Returns dict(rows (B K, 14), aux (B K, 4), k2, k3, matrices, K, nk, thresh,
    det_threshold, seed) of float32 arrays.  confidence: the final score is the raw score times a per-row confidence (what
    TEST.UNCERTAINTY_AS_CONFIDENCE makes of it), so that the visit order is not the rank order."""
    assert len(counts) == B and all(0 <= c <= K for c in counts)
    rng = np.random.RandomState(seed)
    for _ in range(20):
        rows = np.zeros((B * K, 14), np.float32)
        aux = np.zeros((B * K, 4), np.float32)
        matrices, ok = [], True
        for b, n in enumerate(counts):
            block = _draw_rows(rng, K)
            block = block[rng.permutation(K)]
            raw = np.concatenate([-np.sort(-rng.uniform(det_threshold + 0.05, 0.95, n)),
                                  -np.sort(-rng.uniform(0.01, det_threshold - 0.02, K - n))]).astype(np.float32)
            conf = rng.uniform(0.3, 1.0, K).astype(np.float32) if confidence else np.ones(K, np.float32)
            block[:, 13] = raw * conf
            rows[b * K:(b + 1) * K] = block
            aux[b * K:(b + 1) * K, 0] = raw
            aux[b * K:(b + 1) * K, 1:] = rng.uniform(0, 1, (K, 3))
            m = overlap_matrix(block[:n])
            ok = ok and not (np.abs(m - thresh) < MARGIN).any()
            matrices.append(m)
        if ok:
            break
    else:
        raise AssertionError("no scene outside the margin in 20 draws (seed %d)" % seed)
    k2 = rng.normal(0, 1, (B * K, nk, 2)).astype(np.float32)
    k3 = rng.normal(0, 1, (B * K, nk, 3)).astype(np.float32)
    scene = dict(rows=rows, aux=aux, k2=k2, k3=k3, matrices=matrices, K=K, nk=nk, thresh=thresh, det_threshold=det_threshold,
                 seed=seed, counts=list(counts))
    for mode in MODES:                                                  # the oracle alone: neither everything nor nothing
        for agnostic in (False, True):
            for b, n in enumerate(counts):
                if n < 2:
                    continue
                r = nms_image(rows[b * K:(b + 1) * K], aux[b * K:(b + 1) * K, 0], mode, thresh, det_threshold, agnostic, matrices[b])
                assert r["suppressed"].sum() >= _quarter(n) and r["keep"].sum() >= _quarter(n), \
                    "seed %d image %d mode %s: %d kept, %d suppressed of %d" % (seed, b, mode, r["keep"].sum(), r["suppressed"].sum(), n)
    return scene
