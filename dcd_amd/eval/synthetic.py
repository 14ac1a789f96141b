"""Seeded synthetic KITTI annotations for the evaluator's fixtures and timing tool (no dataset, no reference needed).

Annotations are the dicts `kitti_annos.read_annos` returns: name, truncated, occluded, alpha, bbox (x1 y1 x2 y2),
dimensions (l, h, w), location (x, y, z), rotation_y and, for detections, score.  A scene holds all six names the ignore
rules treat specially, every occlusion / truncation level, boxes below the 40 px and 25 px height limits, detections that
are jittered ground truth, and false positives, some of them inside DontCare boxes.
"""
import numpy as np

NAMES = ("Car", "Pedestrian", "Cyclist", "Van", "DontCare", "Person_sitting")
NAME_P = (0.40, 0.15, 0.12, 0.10, 0.15, 0.08)
DT_NAME = {"Car": "Car", "Pedestrian": "Pedestrian", "Cyclist": "Cyclist", "Van": "Car", "Person_sitting": "Pedestrian"}


def empty_anno(with_score=False):
    a = dict(name=np.zeros(0, "<U16"), truncated=np.zeros(0), occluded=np.zeros(0, np.int64), alpha=np.zeros(0),
             bbox=np.zeros((0, 4)), dimensions=np.zeros((0, 3)), location=np.zeros((0, 3)), rotation_y=np.zeros(0))
    if with_score:
        a["score"] = np.zeros(0)
    return a


def random_boxes(rng, n):
    """n boxes with KITTI-range values: x +-15 m, z 5-50 m, l 3-4.5, w 1.5-1.9, h 1.4-1.8, any yaw."""
    loc = np.stack([rng.uniform(-15, 15, n), rng.uniform(1, 2, n), rng.uniform(5, 50, n)], 1)
    dims = np.stack([rng.uniform(3, 4.5, n), rng.uniform(1.4, 1.8, n), rng.uniform(1.5, 1.9, n)], 1)   # l h w
    x0, y0 = rng.uniform(0, 1100, n), rng.uniform(100, 250, n)
    bbox = np.stack([x0, y0, x0 + rng.uniform(20, 200, n), y0 + rng.uniform(15, 120, n)], 1)
    return dict(bbox=bbox, dimensions=dims, location=loc, rotation_y=rng.uniform(-np.pi, np.pi, n),
                alpha=rng.uniform(-3, 3, n))


def make_gt(rng, n):
    g = random_boxes(rng, n)
    g["name"] = np.array(NAMES)[rng.choice(len(NAMES), n, p=NAME_P)].astype("<U16")
    g["truncated"] = rng.choice([0.0, 0.1, 0.2, 0.4, 0.8], n, p=[0.4, 0.2, 0.15, 0.15, 0.1])
    g["occluded"] = rng.choice(4, n, p=[0.45, 0.25, 0.2, 0.1]).astype(np.int64)
    dc = g["name"] == "DontCare"                      # KITTI's DontCare rows carry no 3-D box
    g["dimensions"][dc] = -1.0
    g["location"][dc] = -1000.0
    g["rotation_y"][dc] = -10.0
    g["alpha"][dc] = -10.0
    g["truncated"][dc] = -1.0
    g["occluded"][dc] = -1
    return g


def make_dt(rng, g, keep_p=0.85, max_fp=2, jitter=None):
    """Detections for one image: kept ground-truth boxes with noise, plus false positives."""
    j = dict(bbox=1.0, dimensions=0.05, location=0.10, rotation_y=0.08, alpha=0.2)
    j.update(jitter or {})
    n = len(g["name"])
    keep = (g["name"] != "DontCare") & (rng.rand(n) < keep_p)
    k = int(keep.sum())
    d = {key: g[key][keep] + rng.normal(0, j[key], g[key][keep].shape) for key in j}
    d["name"] = np.array([DT_NAME[s] for s in g["name"][keep]], "<U16")
    n_fp = int(rng.randint(0, max_fp + 1))
    if n_fp:
        f = random_boxes(rng, n_fp)
        dcs = g["bbox"][g["name"] == "DontCare"]
        for i in range(n_fp):
            if len(dcs) and rng.rand() < 0.6:         # a false positive that lies inside a DontCare box
                b = dcs[rng.randint(len(dcs))]
                w, h = b[2] - b[0], b[3] - b[1]
                f["bbox"][i] = [b[0] + 0.1 * w, b[1] + 0.1 * h, b[2] - 0.2 * w, b[3] - 0.1 * h]
        for key in j:
            d[key] = np.concatenate([d[key], f[key]], 0)
        d["name"] = np.concatenate([d["name"], np.array(NAMES)[rng.randint(0, 3, n_fp)]]).astype("<U16")
    m = k + n_fp
    d["truncated"] = np.zeros(m)
    d["occluded"] = np.zeros(m, np.int64)
    d["score"] = np.concatenate([rng.uniform(0.4, 1.0, k), rng.uniform(0.05, 0.7, n_fp)])   # false positives score lower
    return d


def make_scene(rng, n_img, n_obj=(2, 9), empty_gt=(), empty_dt=(), jitter=None):
    """(gt_annos, dt_annos) of n_img images; the listed image indices get no ground truth / no detection."""
    gts, dts = [], []
    for i in range(n_img):
        g = make_gt(rng, 0 if i in empty_gt else int(rng.randint(*n_obj)))
        d = make_dt(rng, g, jitter=jitter)
        if i in empty_dt:
            d = make_dt(rng, make_gt(rng, 0), max_fp=0)
        gts.append(g)
        dts.append(d)
    return gts, dts
