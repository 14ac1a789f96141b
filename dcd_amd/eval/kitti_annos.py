"""KITTI label / result text files <-> annotation dicts.

`read_annos` restates `get_label_anno` / `get_label_annos` (DGDE/data/datasets/evaluation/kitti_object_eval_python/
kitti_common.py:295-374) and `write_detections` restates `generate_kitti_3d_detection` (evaluate.py:33-53), quirks included:
  * names are `str.capitalize()`d on reading, so 'DontCare' becomes 'Dontcare' and 'Person_sitting' stays;
  * a missing file, an empty file or a first line shorter than 15 characters gives an empty annotation;
  * `dimensions` is reordered from the file's h w l to l h w;
  * the score column exists only when the FIRST line has 16 fields, otherwise the scores are zeros;
  * a result file keeps its trailing newline (the reference's `check_last_line_break` fails inside its bare `try` on a
    missing `import os`), and an empty prediction is one empty line.
"""
import csv
import os

import numpy as np

ID_TYPE_CONVERSION = {0: "Car", 1: "Pedestrian", 2: "Cyclist"}      # evaluate.py:35-39 == kitti_files.TYPE_ID_CONVERSION


def read_anno(path):
    lines = []
    if os.path.isfile(path):
        with open(path, "r") as f:
            lines = f.readlines()
    content = [] if len(lines) == 0 or len(lines[0]) < 15 else [line.strip().split(" ") for line in lines]
    anno = {
        "name": np.array([x[0].capitalize() for x in content]),
        "truncated": np.array([float(x[1]) for x in content]),
        "occluded": np.array([int(x[2]) for x in content]),
        "alpha": np.array([float(x[3]) for x in content]),
        "bbox": np.array([[float(v) for v in x[4:8]] for x in content]).reshape(-1, 4),
        "dimensions": np.array([[float(v) for v in x[8:11]] for x in content]).reshape(-1, 3)[:, [2, 0, 1]],
        "location": np.array([[float(v) for v in x[11:14]] for x in content]).reshape(-1, 3),
        "rotation_y": np.array([float(x[14]) for x in content]).reshape(-1),
    }
    if len(content) != 0 and len(content[0]) == 16:
        anno["score"] = np.array([float(x[15]) for x in content])
    else:
        anno["score"] = np.zeros([len(anno["bbox"])])
    return anno


def read_annos(folder, image_ids=None):
    """One annotation dict per image id (strings, '<id>.txt' in `folder`); every file of the folder when ids is None."""
    if image_ids is None:
        return [read_anno(os.path.join(folder, f)) for f in os.listdir(folder)]
    return [read_anno(os.path.join(folder, idx + ".txt")) for idx in image_ids]


def read_imageset(path):
    with open(path, "r") as f:
        return [line.strip() for line in f.readlines()]


def rounded_rows(rows):
    """The values `write_detections` writes: float32 rows rounded to 4 decimals in float32."""
    rows = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
    if len(rows) == 0:
        return np.zeros((0, 14), np.float32)
    return rows.astype(np.float32, copy=False).reshape(len(rows), -1).round(4)


def write_detections(rows, path):
    """rows (n, 14) float32: class id, alpha, x1 y1 x2 y2, h w l, x y z, ry, score -- the `PostProcessor` output."""
    rows = rounded_rows(rows)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter=" ", lineterminator="\n")
        if len(rows) == 0:
            w.writerow([])
        for p in rows:
            w.writerow([ID_TYPE_CONVERSION[int(p[0])], 0, 0] + p[1:].tolist())
