"""The raster rule of DESIGN.md 6d restated in float64 and Python integers.  TEST INFRASTRUCTURE, numpy only, written from the
rule and not from csrc/render_math.h: the geometry in float64 (the library's is fp32), the raster with Python's unbounded
integers and its own floor division, the painter's order walked serially, later over earlier.

    prims, ends = image_primitives(rows, aux, k2, P, gt, K, h, det_threshold, vis_threshold, keypoints)   one image
    table, counts, ends = batch_table(...)                                                                  the (B, S, 12) layout
    canvas = raster(frames, table, counts, in_h, in_w)                                                      any integer table
"""
import math

import numpy as np

ENTRY = 12
NEAR = 0.125
LIMIT = float(2 ** 24)
GT_COLOR, PRED_COLOR, BOX_COLOR = (244, 96, 108), (25, 202, 173), (0, 255, 0)
KEYPOINT_COLORS = [[128, 64, 128], [244, 35, 232], [70, 70, 70], [102, 102, 156], [190, 153, 153], [153, 153, 153], [250, 170, 30],
                   [220, 220, 0], [107, 142, 35], [255, 0, 0], [0, 0, 142], [0, 0, 70], [152, 251, 152], [0, 130, 180], [220, 20, 60],
                   [0, 60, 100]]
GLYPH_ORDER = "0123456789.CPY?"
FONT = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    ".": (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),
    "C": (".###.", "#...#", "#....", "#....", "#....", "#...#", ".###."),
    "P": ("####.", "#...#", "#...#", "####.", "#....", "#....", "#...."),
    "Y": ("#...#", "#...#", "#...#", ".#.#.", "..#..", "..#..", "..#.."),
    "?": (".###.", "#...#", "....#", "...#.", "..#..", ".....", "..#.."),
}
# the 12 edges as draw_projected_box3d draws them, then the front-face diagonals
BOX_EDGES = [e for k in range(4) for e in ((k, (k + 1) % 4), (k + 4, (k + 1) % 4 + 4), (k, k + 4))] + [(0, 5), (1, 4)]


def slots(M, K, nk):
    return 17 * M + K * (28 + nk)


def corners(h, w, l, loc, ry):
    """box3d_to_corners: (8, 3) float64, `loc` the bottom centre."""
    x = np.array([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2], np.float64)
    y = np.array([0, 0, 0, 0, -h, -h, -h, -h], np.float64)
    z = np.array([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2], np.float64)
    c, s = math.cos(ry), math.sin(ry)
    return np.stack((c * x + s * z + loc[0], y + loc[1], -s * x + c * z + loc[2]), axis=1)


def _pixel(v):
    """Truncation toward zero, or None for a coordinate the rule skips."""
    if not math.isfinite(v) or abs(v) >= LIMIT:
        return None
    return int(v)


def _segment(order, panel, x0, y0, x1, y1, T, rgb):
    ends = (x0, y0, x1, y1)
    px = [_pixel(float(v)) for v in ends]
    if any(p is None for p in px):
        return None, ends
    return dict(panel=panel, kind=0, pts=px, T=T, rgb=tuple(rgb), order=order, glyph=0), ends


def _edge(order, A, B, P, rgb):
    A, B = np.array(A, np.float64), np.array(B, np.float64)
    na, nb = A[2] < NEAR, B[2] < NEAR
    if na and nb:
        return None, (0.0, 0.0, 0.0, 0.0)
    if na or nb:
        inside, outside = (A, B) if na else (B, A)
        t = (NEAR - inside[2]) / (outside[2] - inside[2])
        inside[0] += t * (outside[0] - inside[0])
        inside[1] += t * (outside[1] - inside[1])
        inside[2] = NEAR
    with np.errstate(all="ignore"):
        uv = [((P[0, 0] * q[0] + P[0, 2] * q[2] + P[0, 3]) / (q[2] + P[2, 3]), (P[1, 1] * q[1] + P[1, 2] * q[2] + P[1, 3]) / (q[2] + P[2, 3]))
              for q in (A, B)]
    return _segment(order, 0, uv[0][0], uv[0][1], uv[1][0], uv[1][1], 1, rgb)


def _bev(order, c, h, rgb):
    pts = [((c[i, 0] + 32.0) * h / 64.0, (64.0 - c[i, 2]) * h / 64.0) for i in range(4)]
    out = [_segment(order + i, 1, *pts[i], *pts[(i + 1) % 4], 2, rgb) for i in range(4)]
    out.append(_segment(order + 4, 1, *pts[0], *pts[1], 4, rgb))
    return out


NONE = (None, (0.0, 0.0, 0.0, 0.0))


def image_primitives(rows, aux, k2, P, gt, K, h, det_threshold, vis_threshold, keypoints):
    """One image's slots in the table's order: a list of (primitive dict or None, float ends).  rows (K, 14), aux (K, 4), k2
    (K, nk, 2) or None, P (3, 4), gt = None or (dimensions (M, 3), locations (M, 3), rotys (M), mask (M)), h the frame's height."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    rows, aux = np.asarray(rows, np.float32), np.asarray(aux, np.float32)
    nk = k2.shape[1] if keypoints else 0
    out = []
    M = 0 if gt is None else len(gt[3])
    for m in range(M):                                                     # (a) ground truth, slot order
        dims, locs, rotys, mask = gt
        if not mask[m]:
            out += [NONE] * 17
            continue
        l, hh, w = (float(v) for v in dims[m])
        loc = (float(locs[m][0]), float(locs[m][1]) + hh / 2, float(locs[m][2]))
        c = corners(hh, w, l, loc, float(rotys[m]))
        base = len(out)
        out += [_edge(base + i, c[p], c[q], P, GT_COLOR) for i, (p, q) in enumerate(BOX_EDGES[:12])]
        out += _bev(base + 12, c, float(h), GT_COLOR)
    for j in range(K):                                                     # (b) detections, reverse rank order
        r = K - 1 - j
        row = rows[r]
        per = 28 + nk
        drawn = bool(aux[r, 0] >= np.float32(det_threshold)) and bool(row[13] > np.float32(vis_threshold))
        if not drawn:
            out += [NONE] * per
            continue
        base = len(out)
        x0, y0, x1, y1 = (float(v) for v in row[2:6])
        rect = [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
        out += [_segment(base + i, 0, *rect[i], 1, BOX_COLOR) for i in range(4)]
        c = corners(float(row[6]), float(row[7]), float(row[8]), [float(v) for v in row[9:12]], float(row[12]))
        out += [_edge(base + 4 + i, c[p], c[q], P, PRED_COLOR) for i, (p, q) in enumerate(BOX_EDGES)]
        for k in range(nk):
            u, v = float(k2[r, k, 0]) * P[0, 0] + P[0, 2], float(k2[r, k, 1]) * P[1, 1] + P[1, 2]
            out.append(_segment(base + 18 + k, 0, u, v, u, v, 3, KEYPOINT_COLORS[k % 16]))
        out += _bev(base + 18 + nk, c, float(h), PRED_COLOR)
        score = row[13]                                                    # fp32, as the rule states it
        cents = 0
        if np.isfinite(score) and score >= 0:
            cents = 99 if score >= 1 else min(99, int(np.float32(score * np.float32(100)) + np.float32(0.5)))
        cls = float(row[0])
        letter = "CPY"[int(cls)] if 0 <= cls < 3 else "?"
        text = letter + "0." + "%02d" % cents
        lx, ly = _pixel(x0), _pixel(y0)
        for i, ch in enumerate(text):
            order = base + 23 + nk + i
            if lx is None or ly is None:
                out.append((None, (x0, y0, 0.0, 0.0)))
                continue
            gx, gy = lx + 6 * i, ly - 8
            out.append((dict(panel=0, kind=1, pts=[gx, gy, gx + 4, gy + 6], T=1, rgb=BOX_COLOR, order=order, glyph=GLYPH_ORDER.index(ch)),
                        (x0, y0, 0.0, 0.0)))
    return out


def batch_table(rows, aux, k2, P, gt, K, heights, det_threshold, vis_threshold, keypoints):
    """All images: (table (B, S, 12) int32, counts (B,), ends (B, S, 4) float64).  P: (B, 3, 4); gt: None or the (B, M, ...) tables;
    heights: the frames' heights."""
    B = len(heights)
    per_image = []
    for b in range(B):
        g = None if gt is None else tuple(t[b] for t in gt)
        kk = None if k2 is None else np.asarray(k2).reshape(B, K, -1, 2)[b]
        per_image.append(image_primitives(np.asarray(rows).reshape(B, K, 14)[b], np.asarray(aux).reshape(B, K, 4)[b], kk, P[b], g, K,
                                          heights[b], det_threshold, vis_threshold, keypoints))
    S = len(per_image[0])
    table = np.zeros((B, S, ENTRY), np.int32)
    table[:, :, 1] = -1
    counts = np.zeros(B, np.int32)
    ends = np.zeros((B, S, 4), np.float64)
    for b, prims in enumerate(per_image):
        assert len(prims) == S
        for i, (p, e) in enumerate(prims):
            ends[b, i] = e
            if p is not None:
                table[b, i] = [p["panel"], p["kind"], *p["pts"], p["T"], *p["rgb"], p["order"], p["glyph"]]
                counts[b] = i + 1
    return table, counts, ends


def _floordiv(a, b):
    """floor(a / b) for b > 0, spelled out (Python's // is this already; the check keeps the rule in sight)."""
    q = a // b
    assert q * b <= a < (q + 1) * b
    return q


def segment_pixels(x0, y0, x1, y1, T):
    """Every (x, y) the rule stamps for a segment with integer ends, unclipped, in Python integers."""
    dx, dy = x1 - x0, y1 - y0
    xmajor = abs(dx) >= abs(dy)
    a, b = ((x0, y0), (x1, y1)) if xmajor else ((y0, x0), (y1, x1))
    if b[0] < a[0]:
        a, b = b, a
    D, dm = b[0] - a[0], b[1] - a[1]
    offs = range(-((T - 1) // 2), T // 2 + 1)
    for t in range(D + 1):
        m = a[1] + (_floordiv(2 * t * dm + D, 2 * D) if D else 0)
        for oa in offs:
            for ob in offs:
                yield (a[0] + t + oa, m + ob) if xmajor else (m + ob, a[0] + t + oa)


def _clipped_segment_pixels(x0, y0, x1, y1, T, pw, ph):
    """segment_pixels inside [0, pw) x [0, ph): the major range is cut first so a far end costs nothing; same pixels."""
    dx, dy = x1 - x0, y1 - y0
    xmajor = abs(dx) >= abs(dy)
    a, b = ((x0, y0), (x1, y1)) if xmajor else ((y0, x0), (y1, x1))
    if b[0] < a[0]:
        a, b = b, a
    D, dm = b[0] - a[0], b[1] - a[1]
    lim_major, lim_minor = (pw, ph) if xmajor else (ph, pw)
    lo_o, hi_o = -((T - 1) // 2), T // 2
    t0, t1 = max(0, -hi_o - a[0]), min(D, lim_major - 1 - lo_o - a[0])
    for t in range(t0, t1 + 1):
        m = a[1] + (_floordiv(2 * t * dm + D, 2 * D) if D else 0)
        for oa in range(lo_o, hi_o + 1):
            M = a[0] + t + oa
            if not 0 <= M < lim_major:
                continue
            for ob in range(lo_o, hi_o + 1):
                if 0 <= m + ob < lim_minor:
                    yield (M, m + ob) if xmajor else (m + ob, M)


def entry_ok(e):
    if e[1] not in (0, 1) or e[0] not in (0, 1):
        return False
    if any(abs(int(v)) >= 2 ** 24 for v in e[2:6]) or not 0 <= e[10] < 2 ** 18:
        return False
    return 1 <= e[6] <= 4 if e[1] == 0 else 0 <= e[11] < len(GLYPH_ORDER)


def raster(frames, table, counts, in_h, in_w):
    """Painter's algorithm over an integer table: frames = list of (h, w, 3) uint8 arrays; returns the (B, in_h, in_w + in_h, 3)
    canvas.  Entries are painted in ascending (order, index), later over earlier."""
    B = len(frames)
    canvas = np.zeros((B, in_h, in_w + in_h, 3), np.uint8)
    for b, frame in enumerate(frames):
        h, w = frame.shape[:2]
        canvas[b, :h, :w] = frame
        canvas[b, :h, w:w + h] = 230
        n = min(max(int(counts[b]), 0), table.shape[1])
        todo = sorted((int(table[b, i, 10]), i) for i in range(n) if entry_ok(table[b, i]))
        for _, i in todo:
            e = [int(v) for v in table[b, i]]
            left, pw = (w, h) if e[0] else (0, w)
            rgb = [v & 255 for v in e[7:10]]
            if e[1] == 0:
                pix = _clipped_segment_pixels(e[2], e[3], e[4], e[5], e[6], pw, h)
            else:
                art = FONT[GLYPH_ORDER[e[11]]]
                pix = ((e[2] + gx, e[3] + gy) for gy in range(7) for gx in range(5) if art[gy][gx] == "#")
            for x, y in pix:
                if 0 <= x < pw and 0 <= y < h:
                    canvas[b, y, left + x] = rgb
    return canvas
