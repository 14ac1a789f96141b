"""Float64 restatement of the mirrored-view merge (DESIGN.md "Mirrored-view test-time augmentation"; include/dcd_hip.h,
dcd_tta_merge_detections), written from the rule and not from csrc/tta_math.h: numpy only, the overlaps are tests/nms_refs.py's.
TEST INFRASTRUCTURE.

  unmirror          a row of the mirrored view back in the frame's own coordinates, in float64 (what the fused floats are judged
                    against) or in float32 (the row the rule hands to the overlap: the rule's un-mirroring is plain float32, and
                    the overlap is defined on float32 rows)
  match_matrix      (3, n, K) float64: the three overlaps of every candidate of view A with every un-mirrored row of view M
  merge_image       candidates, visit order, the greedy matching, the fused rows in float64 and the output order of one image
  merge_batch       the same over (2 B K, .) arrays
  build_scene       a seeded pair of views on top of `nms_refs.build_scene` under the MARGIN CONDITIONS: no overlap within
                    `MARGIN` of the match threshold, the overlaps a candidate could choose between at least `MARGIN` apart, and
                    per image with two candidates or more at least a quarter matched and a quarter unmatched in every mode --
                    asserted here, on the CPU, by the oracle alone

What is exact and what is not.  Decisions (n, the matching, src, mate, the order) are compared exactly; so is every float that
the rule only copies.  Scores are exact too: the mean of two float32 numbers and the product of two are exact in float64, so
rounding them once to float32 gives the very bits float32 arithmetic gives, and the oracle orders the output by those float32
raw scores.  The other fused floats are float64 here and are compared per column scale (`fused_distance`); the two angle
columns by their distance on the circle, since a yaw at the wrap may come out as -pi in one precision and pi in the other.
Row layout (`write_detections`): 0 class | 1 alpha | 2:6 box | 6:9 h w l | 9:12 x y z | 12 ry | 13 score; aux: raw score, depth
error, confidence, arg-max."""
import numpy as np

import nms_refs as N

MODES = N.MODES
MARGIN = 1e-4


def wrap(a):
    for _ in range(4):
        if a > np.pi:
            a = a - 2 * np.pi
    for _ in range(4):
        if a < -np.pi:
            a = a + 2 * np.pi
    return a


def _wrap32(a):
    pi = np.float32(np.pi)
    for _ in range(4):
        if a > pi:
            a = np.float32(a - np.float32(2) * pi)
    for _ in range(4):
        if a < -pi:
            a = np.float32(a + np.float32(2) * pi)
    return a


def unmirror(row, width, dtype=np.float64):
    """The inverse of `data/augment.py:flip_sample` on one row."""
    if dtype == np.float32:
        m = np.asarray(row, np.float32)
        out = m.copy()
        edge, pi = np.float32(width - 1), np.float32(np.pi)
        out[2], out[4], out[9] = edge - m[4], edge - m[2], -m[9]
        out[12] = _wrap32(np.float32(-pi - m[12]) if m[12] < 0 else np.float32(pi - m[12]))
        out[1] = _wrap32(np.float32(out[12] - np.arctan2(out[9], out[11])))
        return out
    m = np.asarray(row, np.float64)
    out = m.copy()
    out[2], out[4], out[9] = (width - 1) - m[4], (width - 1) - m[2], -m[9]
    out[12] = wrap(-np.pi - m[12] if m[12] < 0 else np.pi - m[12])
    out[1] = wrap(out[12] - np.arctan2(out[9], out[11]))
    return out


def mirror(row, width):
    """`flip_sample` on one float64 row: what a perfect detector would return for the mirrored frame."""
    return unmirror(row, width)                                         # the flip is its own inverse


def match_matrix(rows_a, rows_m, width, n):
    out = np.zeros((3, n, len(rows_m)))
    un = [unmirror(r, width, np.float32) for r in rows_m]
    for a in range(n):
        for m, b in enumerate(un):
            out[:, a, m] = N.overlaps_of_pair(rows_a[a], b)
    return out


def fuse(a, xa, m, xm):
    """a, xa: view A's row and aux; m, xm: the UN-MIRRORED row of view M and its aux; float64 in, float64 out."""
    sa, sm = a[13], m[13]
    s = sa + sm
    wa = sa / s if (s > 0 and np.isfinite(s)) else 0.5
    wm = 1 - wa
    row, aux = a.copy(), xa.copy()
    row[2:9] = wa * a[2:9] + wm * m[2:9]
    ea, em = xa[1], xm[1]
    if np.isfinite(ea) and ea > 0 and np.isfinite(em) and em > 0:
        ua, um = 1 / ea, 1 / em
    else:
        ua, um = wa, wm
    with np.errstate(all="ignore"):
        z = (ua * a[11] + um * m[11]) / (ua + um)
        row[9] = z * (wa * a[9] / a[11] + wm * m[9] / m[11])
        row[10] = z * (wa * a[10] / a[11] + wm * m[10] / m[11])
        row[11] = z
        d = wrap(m[12] - a[12])
        if abs(d) > np.pi / 2:
            row[12] = m[12] if sm > sa else a[12]
        else:
            row[12] = wrap(a[12] + wm * d)
        row[1] = wrap(row[12] - np.arctan2(row[9], z))
        row[13] = float(np.float32(0.5 * s))
        aux[0] = float(np.float32(0.5 * (xa[0] + xm[0])))
        aux[1] = (ua * ea + um * em) / (ua + um)
    return row, aux


def merge_image(rows_a, aux_a, rows_m, aux_m, width, mode, match_thresh, det_threshold, unmatched_scale, matrix=None):
    """One image.  Returns dict(n, order, mate_of (K,): the M rank matched to every A rank or -1, src (K,): the A rank at every
    output row, mate (K,): mate_of[src], rows (K, 14) / aux (K, 4) float64 in OUTPUT order, matrix (3, n, K))."""
    rows_a, aux_a, rows_m, aux_m = (np.asarray(x, np.float32) for x in (rows_a, aux_a, rows_m, aux_m))
    K = len(rows_a)
    n = N.count_candidates(aux_a[:, 0], det_threshold)
    order = N.visit_order(rows_a[:n, 13])
    if matrix is None:
        matrix = match_matrix(rows_a, rows_m, width, n)
    ovl = matrix[MODES.index(mode)]
    eligible = ~np.isnan(aux_m[:, 0])
    cls_a, cls_m = np.trunc(rows_a[:, 0]), np.trunc(rows_m[:, 0])
    mate_of = np.full(K, -1, np.int64)
    taken = np.zeros(K, bool)
    for a in order:
        best, at = None, -1
        for m in range(K):
            if taken[m] or not eligible[m] or cls_a[a] != cls_m[m] or not ovl[a, m] > match_thresh:
                continue
            if best is None or ovl[a, m] > best:                        # a tie keeps the lower M rank
                best, at = ovl[a, m], m
        if at >= 0:
            mate_of[a], taken[at] = at, True
    rows, aux = rows_a.astype(np.float64), aux_a.astype(np.float64)
    scale = np.float64(np.float32(unmatched_scale))
    for a in range(n):
        if mate_of[a] >= 0:
            m = mate_of[a]
            rows[a], aux[a] = fuse(rows[a], aux[a], unmirror(rows_m[m], width), aux_m[m].astype(np.float64))
        else:
            with np.errstate(all="ignore"):
                rows[a, 13] = np.float32(rows[a, 13] * scale)
                aux[a, 0] = np.float32(aux[a, 0] * scale)
    src = np.argsort(-aux[:, 0], kind="stable")                         # descending, stable on A's rank, NaN last
    return dict(n=n, order=order, mate_of=mate_of, src=src, mate=mate_of[src], rows=rows[src], aux=aux[src], matrix=matrix)


def merge_batch(rows, aux, k2, k3, K, widths, mode, match_thresh, det_threshold, unmatched_scale, matrices=None):
    """What dcd_tta_merge_detections returns for (2 B K, .) arrays: dict(rows (B K, 14) float64, aux (B K, 4) float64, k2, k3
    (the A member's, exact), src, mate (B K,), fused (B K,) bool, images: the per-image results)."""
    rows, aux = np.asarray(rows), np.asarray(aux)
    B = len(rows) // K // 2
    out = dict(rows=np.zeros((B * K, 14)), aux=np.zeros((B * K, 4)), src=np.zeros(B * K, np.int64), mate=np.zeros(B * K, np.int64),
               k2=None if k2 is None else np.empty_like(k2[:B * K]), k3=None if k3 is None else np.empty_like(k3[:B * K]), images=[])
    for b in range(B):
        sa, sm = slice(b * K, (b + 1) * K), slice((B + b) * K, (B + b + 1) * K)
        r = merge_image(rows[sa], aux[sa], rows[sm], aux[sm], int(widths[b]), mode, match_thresh, det_threshold, unmatched_scale,
                        None if matrices is None else matrices[b])
        out["rows"][sa], out["aux"][sa], out["src"][sa], out["mate"][sa] = r["rows"], r["aux"], r["src"], r["mate"]
        if k2 is not None:
            out["k2"][sa], out["k3"][sa] = k2[sa][r["src"]], k3[sa][r["src"]]
        out["images"].append(r)
    out["fused"] = out["mate"] >= 0
    return out


# ---- comparing -----------------------------------------------------------------------------------------------------------------
ANGLE_COLUMNS = (1, 12)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def fused_distance(got_rows, got_aux, want):
    """Largest distance of the fused rows' floats from the float64 oracle, each column over its own scale: the largest magnitude
    the oracle holds in that column among the fused rows (pi for the two angles, which are compared on the circle).  0.0 when no
    row was fused."""
    f = want["fused"]
    if not f.any():
        return 0.0
    worst = 0.0
    for got, ref, angles in ((got_rows, want["rows"], ANGLE_COLUMNS), (got_aux, want["aux"], ())):
        g, w = np.asarray(got, np.float64)[f], ref[f]
        nan = np.isnan(w)                                               # (a NaN score in, a NaN score out: in both or in neither)
        assert np.array_equal(np.isnan(g), nan), "NaNs of the fused rows differ from the oracle's"
        g, w = np.where(nan, 0.0, g), np.where(nan, 0.0, w)
        with np.errstate(invalid="ignore"):                             # (an infinite score in both: the difference is a NaN, caught below)
            d = np.abs(g - w)
        assert not np.isnan(d[np.isfinite(w)]).any()
        d = np.where(np.isfinite(w), d, 0.0)
        w = np.where(np.isfinite(w), w, 0.0)
        scale = np.abs(w).max(0) + 1e-6
        for c in angles:
            d[:, c] = np.abs((g[:, c] - w[:, c] + np.pi) % (2 * np.pi) - np.pi)
            scale[c] = np.pi
        worst = max(worst, float((d / scale).max()))
    return worst


def assert_decisions_and_copies(got, want, K, det_threshold):
    """got: (rows, aux, k2, k3, src, mate) float32 / int arrays.  Everything that is a decision or a copy, exactly."""
    rows, aux, k2, k3, src, mate = got
    assert np.array_equal(src, want["src"]), "src differs"
    assert np.array_equal(mate, want["mate"]), "mate differs"
    f = want["fused"]
    w_rows, w_aux = want["rows"].astype(np.float32), want["aux"].astype(np.float32)
    assert same_bits(rows[~f], w_rows[~f]) and same_bits(aux[~f], w_aux[~f]), "a row without a mate is not a copy"
    assert same_bits(rows[f][:, [0, 13]], w_rows[f][:, [0, 13]]) and same_bits(aux[f][:, [0, 2, 3]], w_aux[f][:, [0, 2, 3]]), \
        "class, scores, confidence or arg-max of a fused row"
    if want["k2"] is not None:
        assert same_bits(k2, want["k2"]) and same_bits(k3, want["k3"]), "key points do not follow their A row"
    for b in range(len(rows) // K):
        blk, ref = aux[b * K:(b + 1) * K, 0], w_aux[b * K:(b + 1) * K, 0]
        assert N.count_candidates(blk, det_threshold) == N.count_candidates(ref, det_threshold)
        rest = blk[N.count_candidates(blk, det_threshold):]
        assert not (rest >= np.float32(det_threshold)).any(), "a row at or above the cut outside the prefix"


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _quarter(n):
    return -(-n // 4)


def _mirrored_view(rng, block, aux_block, width, det_threshold):
    """View M of one image: every row of view A mirrored, most of them jittered as a second look at the same object would be, some
    moved away or given another class (no partner), shuffled, with raw scores of their own in descending order."""
    K = len(block)
    m = np.stack([mirror(r, width) for r in block.astype(np.float64)])
    m[:, 2:6] += rng.normal(0, 0.4, (K, 4))
    m[:, 6:9] += rng.normal(0, 0.01, (K, 3))
    m[:, 9:12] += rng.normal(0, 0.02, (K, 3))
    m[:, 12] += rng.normal(0, 0.02, K)
    gone = rng.rand(K) < 0.4
    m[gone, 9] += rng.choice([-1.0, 1.0], int(gone.sum())) * rng.uniform(15, 30, int(gone.sum()))
    m[gone, 2] += 400
    m[gone, 4] += 400
    other = ~gone & (rng.rand(K) < 0.1)
    m[other, 0] = (np.trunc(m[other, 0]) + 1) % 3 + rng.uniform(0, 0.98, int(other.sum()))
    m = m[rng.permutation(K)].astype(np.float32)
    raw = -np.sort(-rng.uniform(0.02, 0.95, K)).astype(np.float32)
    m[:, 13] = raw * rng.uniform(0.3, 1.0, K).astype(np.float32)
    aux = np.zeros((K, 4), np.float32)
    aux[:, 0] = raw
    aux[:, 1] = rng.uniform(0.05, 2.0, K)
    aux[:, 2:] = rng.uniform(0, 1, (K, 2))
    return m, aux


WIDTHS = (1242, 1241, 1224, 1237)        # even and odd: (W - 1) - x is not W - x


def build_scene(seed, B, K, counts, nk, match_thresh=0.5, det_threshold=0.2, confidence=False):
    """counts: candidates of view A of every image.  Returns dict(rows (2 B K, 14), aux (2 B K, 4), k2 (2 B K, nk, 2), k3, widths
    (B,) int32, matrices [(3, n, K)], K, nk, match_thresh, det_threshold, counts)."""
    s = N.build_scene(seed, B, K, counts, nk, det_threshold=det_threshold, confidence=confidence)
    rng = np.random.RandomState(seed + 7919)
    widths = np.array([WIDTHS[b % len(WIDTHS)] for b in range(B)], np.int32)
    rows, aux = np.concatenate([s["rows"], np.zeros_like(s["rows"])]), np.concatenate([s["aux"], np.zeros_like(s["aux"])])
    aux[:B * K, 1] = aux[:B * K, 1] * 1.95 + 0.05                       # depth errors: positive
    matrices = []
    for b, n in enumerate(counts):
        sa, sm = slice(b * K, (b + 1) * K), slice((B + b) * K, (B + b + 1) * K)
        for _ in range(40):
            rows[sm], aux[sm] = _mirrored_view(rng, rows[sa], aux[sa], int(widths[b]), det_threshold)
            m = match_matrix(rows[sa], rows[sm], int(widths[b]), n)
            ok = not (np.abs(m - match_thresh) < MARGIN).any()
            same = np.trunc(rows[sa][:n, 0])[:, None] == np.trunc(rows[sm][:, 0])[None, :]
            for i in range(3):
                for a in range(n):
                    v = np.sort(m[i, a][same[a] & (m[i, a] > match_thresh)])
                    ok = ok and not (np.diff(v) < MARGIN).any()
            for mode in MODES:
                if n >= 2 and ok:
                    r = merge_image(rows[sa], aux[sa], rows[sm], aux[sm], int(widths[b]), mode, match_thresh, det_threshold, 0.5, m)
                    matched = int((r["mate_of"][:n] >= 0).sum())
                    ok = matched >= _quarter(n) and n - matched >= _quarter(n)
            if ok:
                break
        else:
            raise AssertionError("seed %d image %d: no mirrored view under the margin and quarter conditions in 40 draws" % (seed, b))
        matrices.append(m)
    k2 = rng.normal(0, 1, (2 * B * K, nk, 2)).astype(np.float32)
    k3 = rng.normal(0, 1, (2 * B * K, nk, 3)).astype(np.float32)
    return dict(rows=rows, aux=aux, k2=k2, k3=k3, widths=widths, matrices=matrices, K=K, nk=nk, match_thresh=match_thresh,
                det_threshold=det_threshold, counts=list(counts), seed=seed)
