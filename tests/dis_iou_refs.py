"""Float64 restatement of the disentangled IoU report (DESIGN.md "Disentangled IoU report"; include/dcd_hip.h,
dcd_dis_iou_estimates / dcd_dis_iou_accumulate), written from the rules and the decode's formulas, not from csrc/dis_iou_math.h:
numpy only.  TEST INFRASTRUCTURE.

  decode_slot       the heads of one slot in float64: dimensions, the four depths and sigmas, the fusion, the yaw, the all-pairs
                    edge depth, the ten depth methods
  slot_boxes        the sixteen boxes (the label's, then the fifteen variants') as (16, 7) float64: h w l x y z ry, y the bottom
  boxes_of          the same over a batch: (n, 16, 7); an empty slot's boxes are zeros
  exact_overlaps    BEV and 3-D overlap of a box with the label by the exact rotated clip of tests/nms_refs.py, in float64 on the
                    float32 box numbers; NaN for a box with a non-finite number
  rows_of           (n, 33) float64 rows [valid, class, gt_z, bev[15], iou3d[15]] from given boxes
  tables_of         the accumulate: the rows walked in slot order, each booked into its (class, bin) cells in double
  seeded_labels     labels around the predictions: per slot a mix of small and large errors in every component
"""
import numpy as np

import nms_refs

NV, NMETRIC, STATS, GT, BOX, NBOX = 15, 2, 6, 9, 7, 16
ROW = 3 + NMETRIC * NV
VARIANTS = ("full", "location", "offset", "dims", "orient", "depth:direct", "depth:kpt_center", "depth:kpt_02", "depth:kpt_13",
            "depth:soft", "depth:hard", "depth:mean", "depth:edges", "depth:oracle", "depth:gmw")
FULL, LOCATION, OFFSET, DIMS, ORIENT, DEPTH0 = 0, 1, 2, 3, 4, 5
DIRECT, KPT_CENTER, KPT_02, KPT_13, SOFT, HARD, MEAN, EDGES, ORACLE, GMW = range(10)
PI = np.pi


def _wrap(a):
    a = a - 2 * PI if a > PI else a
    return a + 2 * PI if a < -PI else a


def _clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)      # a NaN passes, as torch.clamp


def _location(spec, tab, x, y, off, depth):
    """(centre + offset) * down_ratio - pad, back-projected at `depth` with the image's P."""
    P = tab[4:].reshape(3, 4)
    u = (x + off[0]) * spec["down_ratio"] - tab[0]
    v = (y + off[1]) * spec["down_ratio"] - tab[1]
    return np.array([(u - P[0, 2]) * depth / P[0, 0] + P[0, 3] / -P[0, 0], (v - P[1, 2]) * depth / P[1, 1] + P[1, 3] / -P[1, 1], depth])


def decode_slot(spec, vec, cls, y, x, tab):
    """dict(dims (l h w), depth (4), sigma (4), best, fused, roty, alpha, edge, off) of one slot, float64 throughout."""
    with np.errstate(all="ignore"):
        vec, tab = np.asarray(vec, np.float64), np.asarray(tab, np.float64)
        off = vec[spec["ch_offset"]:spec["ch_offset"] + 2]
        ci = min(max(int(cls), 0), len(spec["dim_mean"]) - 1)
        d = vec[spec["ch_dims"]:spec["ch_dims"] + 3].copy()
        if spec["dim_mode"] == 1:
            d = np.exp(d)
        if spec["dim_mode"] != 0:
            mean, std = np.asarray(spec["dim_mean"][ci], np.float32).astype(np.float64), np.asarray(spec["dim_std"][ci], np.float32).astype(np.float64)
            d = d * std + mean if spec["dim_std_on"] else d * mean
        lo, hi = (float(np.float32(v)) for v in spec["depth_range"])
        raw = vec[spec["ch_depth"]]
        if spec["depth_mode"] == 1:
            z0 = np.exp(raw)
        elif spec["depth_mode"] == 2:
            z0 = raw * float(np.float32(spec["depth_ref"][1])) + float(np.float32(spec["depth_ref"][0]))
        else:
            z0 = 1.0 / (1.0 / (1.0 + np.exp(-raw))) - 1.0
        depth = np.zeros(4)
        depth[0] = _clamp(z0, lo, hi)
        ky = vec[spec["ch_corner"] + 1:spec["ch_corner"] + 20:2]
        fh = tab[4] * d[1]
        eps = float(np.float32(spec["eps"]))
        relu = lambda v: 0.0 if v < 0 else v  # noqa: E731  (a NaN passes, as F.relu)
        five = [fh / (relu(ky[t] - ky[b]) * spec["down_ratio"] + eps) for t, b in ((8, 9), (0, 4), (2, 6), (1, 5), (3, 7))]
        depth[1] = _clamp(five[0], lo, hi)
        depth[2] = _clamp((five[1] + five[2]) / 2, lo, hi)
        depth[3] = _clamp((five[3] + five[4]) / 2, lo, hi)
        sigma = np.exp(np.concatenate(([vec[spec["ch_depth_unc"]]], vec[spec["ch_corner_unc"]:spec["ch_corner_unc"] + 3])))
        w = 1.0 / sigma
        best = 0
        for i in range(4):
            if w[i] > w[best]:
                best = i
        fused = float(np.sum(depth * (w / w.sum())))
        coarse = _location(spec, tab, x, y, off, fused)
        nb = spec["n_bins"]
        c = vec[spec["ch_ori_cls"]:spec["ch_ori_cls"] + 2 * nb].reshape(nb, 2)
        o = vec[spec["ch_ori_off"]:spec["ch_ori_off"] + 2 * nb].reshape(nb, 2)
        p = np.exp(c[:, 1] - c.max(1)) / np.exp(c - c.max(1, keepdims=True)).sum(1)
        b, bp = 0, 0.0
        for i in range(nb):
            if i == 0 or p[i] > bp:
                b, bp = i, p[i]
        ori = np.arctan2(o[b, 0], o[b, 1]) + (0.0, PI / 2, PI, -PI / 2)[b]
        roty, alpha = _wrap(ori + np.arctan2(coarse[0], coarse[2])), _wrap(ori)
        # the all-pairs edge depth: mean over i < j of clamp(|dY + dvC| / max(|dvn|, 1e-10), 2, 80) - P[2][3]
        nk = spec["nk"]
        kv = (vec[spec["ch_kpts2d"] + 1:spec["ch_kpts2d"] + 2 * nk:2] + (y + off[1])) * 4.0 - tab[1]
        k3 = vec[spec["ch_kpts3d"]:spec["ch_kpts3d"] + 3 * nk].reshape(nk, 3)
        vn = (kv - tab[4 + 6]) / tab[4 + 5]
        vC = vn * (k3[:, 0] * np.sin(roty) - k3[:, 2] * np.cos(roty))
        i, j = np.triu_indices(nk, 1)
        hm = (k3[i, 1] - k3[j, 1]) + (vC[i] - vC[j])
        zz = np.abs(hm) / np.fmax(np.abs(vn[i] - vn[j]), 1e-10)
        zz = np.fmin(np.fmax(zz, 2.0), 80.0)                     # fmax / fmin drop a NaN, as the solver's clamp does
        edge = float(np.sum(zz - tab[4 + 11]) / len(i))
    return dict(dims=d, depth=depth, sigma=sigma, best=best, fused=fused, roty=roty, alpha=alpha, edge=edge, off=off)


def depth_methods(dec, gt_z, gmw_z):
    four = dec["depth"]
    pick, nearest = -1, 0.0
    for i in range(4):
        e = abs(four[i] - gt_z)
        if e == e and (pick < 0 or e < nearest):
            pick, nearest = i, e
    return np.array([four[0], four[1], four[2], four[3], dec["fused"], four[dec["best"]], four.sum() / 4.0, dec["edge"],
                     four[max(pick, 0)], gmw_z])


def slot_boxes(spec, vec, cls, y, x, tab, gt, gmw_z=np.nan):
    """(16, 7) float64: the label's box and the fifteen variants' (DESIGN.md's table), and the slot's decode."""
    gt, tab = np.asarray(gt, np.float64), np.asarray(tab, np.float64)
    dec = decode_slot(spec, vec, cls, y, x, tab)
    g_off, g_c, (gl, gh, gw), g_ry = gt[0:2], gt[2:5], gt[5:8], gt[8]
    l, h, w = dec["dims"]
    label = np.array([gh, gw, gl, g_c[0], g_c[1] + gh / 2, g_c[2], g_ry])
    out = np.tile(label, (NBOX, 1))
    with np.errstate(all="ignore"):
        at_edge = _location(spec, tab, x, y, dec["off"], dec["edge"])
        out[1 + FULL] = [h, w, l, at_edge[0], at_edge[1] + h / 2, at_edge[2], dec["roty"]]
        out[1 + LOCATION, 3:6] = [at_edge[0], at_edge[1] + gh / 2, at_edge[2]]
        at_gt = _location(spec, tab, x, y, dec["off"], g_c[2])
        out[1 + OFFSET, 3:6] = [at_gt[0], at_gt[1] + gh / 2, at_gt[2]]
        out[1 + DIMS, 0:3] = [h, w, l]
        out[1 + DIMS, 4] = g_c[1] + h / 2
        out[1 + ORIENT, 6] = _wrap(dec["alpha"] + np.arctan2(g_c[0], g_c[2]))
        for m, d in enumerate(depth_methods(dec, g_c[2], gmw_z)):
            loc = _location(spec, tab, x, y, g_off, d)
            out[1 + DEPTH0 + m, 3:6] = [loc[0], loc[1] + gh / 2, loc[2]]
    return out, dec


def boxes_of(spec, vectors, ys, xs, classes, gt, valid, table, gmw_z=None):
    """(n, 16, 7) float64 for (B, M, C) vectors and per-slot arrays; table (B, 16).  Also the list of per-slot decodes."""
    vectors = np.asarray(vectors, np.float64)
    B, M, C = vectors.shape
    n = B * M
    flat = lambda a: np.asarray(a, np.float64).reshape(n, -1)  # noqa: E731
    vec, ys, xs, classes, valid, gt = vectors.reshape(n, C), flat(ys)[:, 0], flat(xs)[:, 0], flat(classes)[:, 0], flat(valid)[:, 0], flat(gt)
    gz = np.full(n, np.nan) if gmw_z is None else flat(gmw_z)[:, 0]
    out, decs = np.zeros((n, NBOX, BOX)), [None] * n
    for s in range(n):
        if valid[s]:
            out[s], decs[s] = slot_boxes(spec, vec[s], classes[s], ys[s], xs[s], np.asarray(table, np.float64)[s // M], gt[s], gz[s])
    return out, decs


def _row14(box):
    r = np.zeros(14)
    r[6:13] = box
    return r


def exact_overlaps(label_box, box):
    """(bev, 3d) in float64 of the float32 numbers of `box` against those of `label_box` (the frame); (NaN, NaN) when one of the
    box's seven numbers is not finite or an overlap is not."""
    box32, label32 = np.asarray(box, np.float32), np.asarray(label_box, np.float32)
    if not np.isfinite(box32).all():
        return np.nan, np.nan
    with np.errstate(all="ignore"):
        _, bev, d3 = nms_refs.overlaps_of_pair(_row14(label32), _row14(box32))
    return (bev, d3) if np.isfinite(bev) and np.isfinite(d3) else (np.nan, np.nan)


def rows_of(boxes, classes, valid):
    """(n, 33) float64 rows from (n, 16, 7) boxes: the exact overlaps of every variant's box with the slot's label."""
    boxes = np.asarray(boxes)
    n = boxes.shape[0]
    classes, valid = np.asarray(classes, np.float64).reshape(-1), np.asarray(valid).reshape(-1)
    rows = np.zeros((n, ROW))
    for s in range(n):
        if not valid[s]:
            continue
        rows[s, 0], rows[s, 1], rows[s, 2] = 1.0, classes[s], np.float32(boxes[s, 0, 5])
        for v in range(NV):
            rows[s, 3 + v], rows[s, 3 + NV + v] = exact_overlaps(boxes[s, 0], boxes[s, 1 + v])
    return rows


def tables_of(rows, edges, thresholds, num_classes):
    """The restatement of dcd_dis_iou_accumulate on float32 rows: slot order, double sums.  thresholds (num_classes, 2, 2).
    Returns (table (num_classes, n_bins, 15, 2, 6), outside (num_classes))."""
    n_bins = len(edges) - 1
    edges = np.asarray(edges, np.float32)
    thr = np.asarray(thresholds, np.float64).reshape(num_classes, NMETRIC, 2)
    table, outside = np.zeros((num_classes, n_bins, NV, NMETRIC, STATS), np.float64), np.zeros(num_classes, np.int64)
    for row in np.asarray(rows, np.float32):
        if row[0] == 0 or not (0 <= row[1] < num_classes):
            continue
        c, z = int(row[1]), row[2]
        inside = [i for i in range(n_bins) if np.isfinite(z) and edges[i] <= z < edges[i + 1]]
        if not inside:
            outside[c] += 1
            continue
        for v in range(NV):
            for k in range(NMETRIC):
                cell, o = table[c, inside[0], v, k], np.float64(row[3 + k * NV + v])
                if not np.isfinite(o):
                    cell[5] += 1.0
                    continue
                cell[0] += 1.0
                cell[1] += o
                cell[2] += o * o
                cell[3] += 1.0 if o > thr[c, k, 0] else 0.0
                cell[4] += 1.0 if o > thr[c, k, 1] else 0.0
    return table, outside


def seeded_labels(spec, vectors, ys, xs, classes, table, seed):
    """Labels around the predictions, float32 (n, 9), and a GMW depth per slot (n,): every third slot is `good` (every component
    within a small error of the prediction, the label's depth near the edge depth); the others put the label's depth near one of
    the other depth methods in turn and draw each of offset, dimensions and yaw small or large by a coin."""
    vectors = np.asarray(vectors, np.float64)
    B, M, C = vectors.shape
    n = B * M
    rng = np.random.RandomState(seed)
    vec = vectors.reshape(n, C)
    ys, xs, classes = (np.asarray(a, np.float64).reshape(-1) for a in (ys, xs, classes))
    table = np.asarray(table, np.float64)
    gt, gmw_z = np.zeros((n, GT), np.float32), np.zeros(n, np.float32)
    others = (DIRECT, KPT_CENTER, KPT_02, KPT_13, SOFT, HARD, MEAN, ORACLE)
    for s in range(n):
        tab = table[s // M]
        dec = decode_slot(spec, vec[s], classes[s], ys[s], xs[s], tab)
        good = s % 3 == 0
        coin = (lambda: False) if good else (lambda: rng.rand() < 0.5)
        methods = depth_methods(dec, 0.0, np.nan)
        gz = (dec["edge"] if good else methods[others[(s // 3 + s) % len(others)]]) + rng.normal(0, 0.02)
        gz = float(np.clip(gz, 0.5, 99.0))
        off = dec["off"] + (rng.normal(0, 0.01, 2) if not coin() else rng.choice([-1, 1], 2) * rng.uniform(1.0, 3.0, 2))
        dims = dec["dims"] * (np.exp(rng.normal(0, 0.005, 3)) if not coin() else np.exp(rng.choice([-1, 1], 3) * rng.uniform(0.2, 0.5, 3)))
        # the yaw the `orient` variant will form at this label, then the label's own yaw beside it
        centre = _location(spec, tab, xs[s], ys[s], off, gz)
        yaw = _wrap(dec["alpha"] + np.arctan2(centre[0], centre[2])) + (rng.normal(0, 0.01) if not coin() else rng.choice([-1, 1]) * rng.uniform(0.4, 1.2))
        gt[s] = np.concatenate((off, centre, dims, [_wrap(yaw)]))
        gmw_z[s] = gz + (rng.normal(0, 0.02) if s % 2 == 0 else rng.choice([-1, 1]) * rng.uniform(2.0, 6.0))
    return gt, gmw_z
