"""Inputs of the renderer's tests, shared by the host build's (test_render_host.py) and the device's (test_gpu_render.py).
TEST INFRASTRUCTURE, numpy only.

A case is a dict: frames (list of (h, w, 3) uint8), rows (B K, 14), aux (B K, 4), k2 (B K, nk, 2) or None, P (B, 3, 4), gt (None or
dimensions (B, M, 3), locations (B, M, 3), rotys (B, M), mask (B, M) uint8), K, det, vis, keypoints, in_h, in_w.

The hand-made cases are EXACT: yaw 0, dyadic sizes and positions, focal length 512, every corner at a power-of-two depth, so the
fp32 builds and the float64 restatement compute the same numbers and the integer tables can be compared bit for bit."""
import numpy as np

IN_H, IN_W = 80, 200
SIZES = ((197, 77), (150, 33))         # (w, h): odd widths, more than one 32 x 32 tile both ways, ragged 3-byte row ends


def frames_of(sizes, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for w, h in sizes]


def intrinsics(B, f=512.0, cu=96.0, cv=40.0, tx=0.0):
    P = np.zeros((B, 3, 4), np.float32)
    P[:, 0, 0] = P[:, 1, 1] = f
    P[:, 0, 2], P[:, 1, 2], P[:, 2, 2] = cu, cv, 1.0
    P[:, 0, 3] = tx
    return P


def image_table(P, sizes, in_h=IN_H, in_w=IN_W):
    """The decode's (B, 16) table: pad, padded size, P."""
    B = len(sizes)
    tab = np.zeros((B, 16), np.float32)
    tab[:, 2], tab[:, 3] = in_w, in_h
    tab[:, 4:] = np.asarray(P, np.float32).reshape(B, 12)
    return tab


def det(cls=0.0, box=(20, 20, 60, 50), hwl=(2.0, 4.0, 4.0), xyz=(0.0, 1.0, 6.0), ry=0.0, score=0.9):
    """A row; with yaw 0 the corners lie at z = xyz[2] -+ w / 2 (hwl[1]) and x = xyz[0] -+ l / 2."""
    return np.array([cls, 0.0, *box, *hwl, *xyz, ry, score], np.float32)


def block(rows, raws, K):
    """rows of one image -> ((K, 14), (K, 4)), padded with rows under every threshold."""
    rows, raws = list(rows), list(raws)
    while len(rows) < K:
        rows.append(det(score=0.0))
        raws.append(0.0)
    aux = np.zeros((K, 4), np.float32)
    aux[:, 0] = raws
    return np.stack(rows), aux


def gt_tables(objects, M):
    """objects: per image a list of None (an unused slot) or (l, h, w, x, y_centre, z, ry)."""
    B = len(objects)
    dims, locs = np.zeros((B, M, 3), np.float32), np.zeros((B, M, 3), np.float32)
    rotys, mask = np.zeros((B, M), np.float32), np.zeros((B, M), np.uint8)
    for b, objs in enumerate(objects):
        for m, o in enumerate(objs):
            if o is not None:
                dims[b, m], locs[b, m], rotys[b, m], mask[b, m] = o[:3], o[3:6], o[6], 1
    return dims, locs, rotys, mask


def _case(rows, aux, K, sizes=SIZES, k2=None, gt=None, det=0.2, vis=0.25, keypoints=False, P=None, seed=0):
    B = len(sizes)
    return dict(frames=frames_of(sizes, seed), rows=np.concatenate(rows), aux=np.concatenate(aux), k2=k2, P=intrinsics(B) if P is None else P,
                gt=gt, K=K, det=det, vis=vis, keypoints=keypoints, in_h=IN_H, in_w=IN_W)


def case_overlap():
    """Ground truth under detections and rank 0 on top where they overlap; the rows that must not draw: suppressed (-inf), under the
    detection threshold, NaN raw score, final score equal to the visualisation threshold; an empty second image."""
    K = 6
    r0, a0 = block([det(box=(30, 20, 90, 60), xyz=(0.5, 1.0, 6.0), score=0.9),
                    det(box=(40, 24, 100, 64), xyz=(1.0, 1.0, 6.0), score=0.8, cls=1.0),
                    det(box=(10, 10, 50, 40), xyz=(-1.0, 1.0, 3.0), hwl=(1.0, 2.0, 2.0), score=0.7),          # suppressed
                    det(box=(60, 30, 120, 70), xyz=(2.0, 1.0, 6.0), score=0.6),                              # vis: 0.25 is not > 0.25
                    det(box=(5, 5, 190, 70), xyz=(0.0, 1.0, 6.0), score=0.95),                               # raw score under 0.2
                    det(box=(5, 5, 190, 70), xyz=(0.0, 1.0, 6.0), score=0.95)],                              # raw score NaN
                   [0.9, 0.8, -np.inf, 0.6, 0.1, np.nan], K)
    r0[3, 13] = 0.25
    r1, a1 = block([], [], K)
    gt = gt_tables([[(4.0, 2.0, 4.0, 0.75, 0.0, 6.0, 0.0), None, (2.0, 1.0, 2.0, -1.5, 0.5, 3.0, 0.0)], [None, None, None]], 3)
    return _case([r0, r1], [a0, a1], K, gt=gt)


def case_near():
    """A box straddling z = 0.125 (corners at z = 0 and 2), one wholly nearer (dropped), key points (one off the panel), a label cut at
    row 0, the class letters and the score's edge cases (>= 1, negative with a negative threshold)."""
    K, nk = 5, 3
    r0, a0 = block([det(box=(8, 3, 70, 40), hwl=(1.0, 2.0, 1.0), xyz=(0.0, 0.5, 1.0), score=1.5, cls=2.0),      # z in {0, 2}
                    det(box=(100, 20, 160, 60), hwl=(1.0, 0.125, 1.0), xyz=(0.0, 0.5, 0.0), score=0.5, cls=5.0),  # z = -+ 1 / 16
                    det(box=(120, 9, 196, 76), hwl=(2.0, 4.0, 4.0), xyz=(-0.5, 1.0, 6.0), score=-0.5, cls=1.0),
                    det(box=(-4.5, -3.5, 30, 30), hwl=(1.0, 2.0, 2.0), xyz=(8.0, 1.0, 3.0), score=0.004, cls=0.75)],
                   [0.9, 0.8, 0.7, 0.6], K)
    r1, a1 = block([det(box=(100, 2, 149, 32), hwl=(1.0, 2.0, 2.0), xyz=(0.25, 0.5, 3.0), score=0.996)], [0.5], K)
    k2 = np.zeros((2 * K, nk, 2), np.float32)
    k2[:, 0] = (-0.125, -0.0625)
    k2[:, 1] = (0.0625, 0.03125)
    k2[:, 2] = (0.5, -0.25)                                               # u = 352: off both frames
    k2[0, 1] = (np.nan, 0.0)
    return _case([r0, r1], [a0, a1], K, k2=k2, det=0.2, vis=-1.0, keypoints=True)


def case_skips():
    """Coordinates the rule skips: 2^24 exactly, just under it (drawn, clipped), NaN, infinities; NaN dimensions."""
    K = 4
    r0, a0 = block([det(box=(10, 10, 2.0 ** 24, 50), score=0.9),                       # top, right and bottom sides skipped
                    det(box=(20, 20, 16777215.0, 60), score=0.8),                      # drawn: the far end costs nothing
                    det(box=(np.nan, 30, 80, np.inf), score=0.7),
                    det(box=(30, 30, 90, 70), hwl=(np.nan, 4.0, 4.0), score=0.6)], [0.9, 0.8, 0.7, 0.6], K)
    r1, a1 = block([det(box=(-2.0 ** 24, -16777215.0, 40, 20), xyz=(-np.inf, 1.0, 6.0), score=0.9)], [0.9], K)
    return _case([r0, r1], [a0, a1], K)


def case_k1():
    """K = 1 on a single image with no ground-truth tables."""
    r0, a0 = block([det(box=(3, 9, 100, 30), hwl=(1.0, 2.0, 2.0), xyz=(0.0, 0.5, 3.0), score=0.5)], [0.5], 1)
    return _case([r0], [a0], 1, sizes=((150, 33),))


def case_empty():
    """Nothing drawable: the picture is the frame and the empty panel."""
    r, a = block([], [], 3)
    return _case([r, r], [a, a], 3, gt=gt_tables([[None], [None]], 1))


HAND_MADE = {"overlap": case_overlap, "near": case_near, "skips": case_skips, "k1": case_k1, "empty": case_empty}


def seeded_scene(sizes=((197, 77), (150, 33), (200, 80)), in_h=IN_H, in_w=IN_W, K=50, nk=73, n_gt=5, f=180.0, seed=3, P=None):
    """B images, K candidates with nk key points, n_gt ground-truth objects each, depths >= 3 m, any yaw."""
    rng = np.random.RandomState(seed)
    B = len(sizes)
    P = intrinsics(B, f=f, cu=sizes[0][0] / 2.0, cv=sizes[0][1] / 2.0, tx=11.5) if P is None else P
    rows, aux = np.zeros((B * K, 14), np.float32), np.zeros((B * K, 4), np.float32)
    rows[:, 0] = rng.randint(0, 3, B * K) + rng.rand(B * K) * 0.5
    z = rng.uniform(3.0, 45.0, B * K)
    x = rng.uniform(-0.6, 0.6, B * K) * z
    rows[:, 6:9] = rng.uniform(1.2, 4.5, (B * K, 3))
    rows[:, 9], rows[:, 10], rows[:, 11] = x, rng.uniform(1.0, 2.0, B * K), z
    rows[:, 12] = rng.uniform(-np.pi, np.pi, B * K)
    for b, (w, h) in enumerate(sizes):
        s = slice(b * K, (b + 1) * K)
        x0, y0 = rng.uniform(0, w - 20, K), rng.uniform(0, h - 12, K)
        rows[s, 2], rows[s, 3] = x0, y0
        rows[s, 4], rows[s, 5] = np.minimum(x0 + rng.uniform(4, 80, K), w - 1), np.minimum(y0 + rng.uniform(4, 40, K), h - 1)
        raw = np.sort(rng.uniform(0.05, 1.0, K))[::-1]
        aux[s, 0] = raw
        rows[s, 13] = raw * rng.uniform(0.3, 1.0, K)
    k2 = (rng.uniform(-0.5, 0.5, (B * K, nk, 2)) * np.array([1.0, 0.3])).astype(np.float32)
    objs = []
    for b in range(B):
        objs.append([(rng.uniform(3, 4.5), rng.uniform(1.4, 2), rng.uniform(1.5, 2), rng.uniform(-8, 8), rng.uniform(0.5, 1.5),
                      rng.uniform(5.5, 40), rng.uniform(-np.pi, np.pi)) for _ in range(n_gt)] + [None] * 2)
    return dict(frames=frames_of(sizes, seed), rows=rows, aux=aux, k2=k2, P=P, gt=gt_tables(objs, n_gt + 2), K=K, det=0.2, vis=0.25,
                keypoints=True, in_h=in_h, in_w=in_w)


def kitti_scene():
    """Two frames of KITTI's sizes in the 384 x 1280 input, KITTI's P2."""
    P = intrinsics(2, f=721.5377, cu=609.5593, cv=172.854, tx=44.85728)
    P[:, 1, 3], P[:, 2, 3] = 0.2163791, 0.002745884
    return seeded_scene(sizes=((1242, 375), (1224, 370)), in_h=384, in_w=1280, K=50, nk=73, n_gt=5, seed=5, P=P)


SCENES = {"seeded": seeded_scene, "kitti": kitti_scene}
# worst distance of the HOST build's float ends from the float64 restatement, in pixels, as test_render_host.py measures it
# (g++ -O2 -ffp-contract=off, glibc's sinf / cosf); test_gpu_render.py holds the device build to four times these
HOST_ENDS_DISTANCE = {"seeded": 2.7618e-05, "kitti": 1.2316e-04}


# ---- hand-written primitive tables (the raster alone) -------------------------------------------------------------------------
def entry(panel, x0, y0, x1, y1, T=1, rgb=(255, 0, 0), order=0, kind=0, glyph=0):
    return [panel, kind, x0, y0, x1, y1, T, *rgb, order, glyph]


def table_of(per_image, stride=None):
    stride = stride or max(1, max(len(p) for p in per_image))
    table = np.zeros((len(per_image), stride, 12), np.int32)
    table[:, :, 1] = -1
    counts = np.zeros(len(per_image), np.int32)
    for b, prims in enumerate(per_image):
        for i, p in enumerate(prims):
            table[b, i] = p
        counts[b] = len(prims)
    return table, counts


OCTANTS = [(37, 0), (0, 29), (-37, 0), (0, -29), (23, 23), (-23, 23), (23, -23), (-23, -23),          # horizontal, vertical, 45 degrees
           (31, 11), (11, 31), (-11, 31), (-31, 11), (-31, -11), (-11, -31), (11, -31), (31, -11)]      # the eight octants


def table_octants(reverse):
    """Every direction from two centres per panel; `reverse` swaps each segment's ends (the canvases must not change)."""
    prims = []
    for panel, (cx, cy) in ((0, (60, 38)), (0, (150, 40)), (1, (38, 38))):
        for i, (dx, dy) in enumerate(OCTANTS):
            a, b = (cx, cy), (cx + dx, cy + dy)
            if reverse:
                a, b = b, a
            prims.append(entry(panel, *a, *b, T=1, rgb=(10 * i + 5, 255 - 10 * i, 40 * panel), order=len(prims)))
    return table_of([prims, prims])


def table_thickness():
    prims = []
    for T in (1, 2, 3, 4):
        prims.append(entry(0, 10 + 40 * T, 5, 30 + 40 * T, 60, T=T, rgb=(255, 255, T), order=T))              # steep
        prims.append(entry(0, 5, 8 + 15 * T, 120, 12 + 15 * T, T=T, rgb=(T, 0, 255), order=10 + T))          # shallow
        prims.append(entry(1, 6 + 16 * T, 6 + 16 * T, 6 + 16 * T, 6 + 16 * T, T=T, rgb=(0, T, 0), order=20 + T))   # points
        prims.append(entry(0, 196, 20 * T - 10, 196, 20 * T - 10, T=T, rgb=(9, 9, 9), order=30 + T))          # brush cut by the seam
        prims.append(entry(1, 0, 10 * T, 0, 10 * T, T=T, rgb=(8, 8, 8), order=40 + T))                        # and from the other side
    return table_of([prims, prims])


def table_seam():
    """Segments across column w and rows h - 1 / h of both frames, wholly outside, far ends, tile edges, invalid entries, order ties."""
    per_image = []
    for w, h in SIZES:
        prims = [entry(0, w - 20, 10, w + 20, 20, T=3, rgb=(1, 2, 3), order=5),          # an image-panel line never reaches the panel
                 entry(1, -20, 12, 20, 22, T=3, rgb=(3, 2, 1), order=6),                 # and the reverse
                 entry(0, 5, h - 1, w + 5, h - 1, T=1, rgb=(7, 7, 7), order=7),          # the last row
                 entry(0, 5, h, w - 5, h, T=1, rgb=(9, 9, 9), order=8),                  # row h: nothing
                 entry(0, 5, h, w - 5, h, T=4, rgb=(9, 1, 9), order=60),                 # row h, T4: rows h - 1 only
                 entry(1, 3, h - 3, 3, h + 30, T=2, rgb=(1, 9, 9), order=10),
                 entry(0, -500, -300, -20, -10, T=4, rgb=(5, 5, 5), order=11),           # wholly outside
                 entry(1, 400, 400, 900, 500, T=4, rgb=(5, 5, 5), order=12),
                 entry(0, -16777215, -16777215, 16777215, 16777215, T=2, rgb=(200, 0, 200), order=13),   # far ends
                 entry(0, 16777215, -16000000, -16777215, 16000001, T=1, rgb=(0, 200, 200), order=14),
                 entry(0, 2 ** 24, 0, 0, 0, rgb=(255, 255, 255), order=15),              # not a primitive: passed over
                 entry(0, 0, 0, 50, 50, T=5, rgb=(255, 255, 255), order=15),
                 entry(2, 0, 0, 50, 50, rgb=(255, 255, 255), order=15),
                 entry(0, 0, 0, 50, 50, rgb=(255, 255, 255), order=2 ** 18),
                 entry(0, 0, 0, 50, 50, rgb=(255, 255, 255), order=3, kind=7),
                 entry(0, 0, 0, 0, 0, rgb=(255, 255, 255), order=3, kind=1, glyph=15),
                 entry(0, 20, 5, 80, 5, T=4, rgb=(50, 60, 70), order=1),                 # order decides, not table position
                 entry(0, 50, 0, 50, 30, T=4, rgb=(70, 60, 50), order=0),
                 entry(0, 20, 25, 80, 25, T=2, rgb=(1, 1, 1), order=2),                  # a tie: the later entry
                 entry(0, 50, 20, 50, 30, T=2, rgb=(2, 2, 2), order=2)]
        for i in range(15):                                                              # every glyph, one cut by each border
            prims.append(entry(0, -2 + 13 * i, -3 + 5 * i, 0, 0, rgb=(0, 255, 0), order=30 + i, kind=1, glyph=i))
        for t in (31, 32, 63, 64):                                                       # on the 32-pixel tile edges
            prims.append(entry(0, t, 0, t, h + 5, T=1, rgb=(t, 100, 100), order=50))
            prims.append(entry(0, 0, t, w + 5, t, T=2, rgb=(100, t, 100), order=51))
            prims.append(entry(0, t - 2, t - 2, t + 2, t + 2, T=3, rgb=(100, 100, t), order=52))
        per_image.append(prims)
    return table_of(per_image, stride=64)


TABLES = {"octants": lambda: table_octants(False), "thickness": table_thickness, "seam": table_seam}
