"""Generates tests/golden/gmw_infer.npz by RUNNING THE REFERENCE'S GMW INFERENCE (imported from /root/reference/GMW) on the CPU:
`load_data('valid')`, the body of `validate` (GMW/main.py:524-548) with the seeded reference model in eval mode, and `GMW_data`
(main.py:123-205), which rewrites the KITTI result files with the refined locations.

Run in the build container only (`python tests/golden/make_golden_gmw_infer.py`, its own process).  Nothing is copied: the modules
are imported where they lie, with the stand-ins `make_golden_gmw.py` lists; `compute_z`, `get_up`, `compute_reg_loss` and the
class `GMW_data` are compiled from the AST of GMW/main.py and executed as they are.

Input: six objects in three images (3 + 2 + 1) and a fourth image of the split without detections.  Keypoints, yaw and location
come from `make_golden_gmw.inputs`; boxes, dims and scores are seeded, every value a float32 (what `engine.gen_data` writes); one
yaw lies below -pi and one above pi, the two branches of the writer's wrapping.

Stored: the records (as the JSON text the loader reads), what the reference's loader made of them, `pred_depth` and
`pred_location` as the reference computed them in fp32, the text of every result file, and KITTI labels for the four images:
the refined boxes with `eval/synthetic.py`-style jitter, re-seeded until every BEV / 3-D overlap between a label and a result
box (this project's float64 clipping, make_golden_eval.exact_overlaps) is at least 0.01 away from 0.7 / 0.5 / 0.25 -- a location
that is off by 2e-5 relative moves an overlap by about 1e-3 at most.
"""
import ast
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/GMW"
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from make_golden_gmw import inputs  # noqa: E402

IMAGES = (("000003", 3), ("000010", 2), ("000021", 1), ("000034", 0))
CLEARANCE = 0.01


def f32(a):
    """float32 values as the Python floats `tolist()` gives: what the detector's records hold."""
    return np.asarray(a, np.float32).tolist()


def make_records(seed=5):
    n = sum(c for _, c in IMAGES)
    k2, k3, rot, loc = inputs(seed=13, B=n)
    rng = np.random.default_rng(seed)
    rot[1, 0] = -np.pi - 0.3
    rot[4, 0] = np.pi + 0.4
    dim = np.stack([rng.uniform(1.4, 1.8, n), rng.uniform(1.5, 1.9, n), rng.uniform(3.0, 4.5, n)], 1)      # h w l
    x0, y0 = rng.uniform(0, 1000, n), rng.uniform(100, 200, n)
    box = np.stack([x0, y0, x0 + rng.uniform(60, 220, n), y0 + rng.uniform(60, 150, n)], 1)
    score = np.sort(rng.uniform(0.3, 1.0, n))[::-1].copy()
    records, i = {}, 0
    for img, count in IMAGES:
        records[img] = []
        for _ in range(count):
            records[img].append({"kpts_2d": f32(k2[i]), "kpts_3d": f32(k3[i]), "pred_rot": f32(rot[i]), "box": f32(box[i]),
                                 "dim": f32(dim[i]), "pred_location": f32(loc[i]), "score": f32(score[i:i + 1]), "cat": "Car"})
            i += 1
    return records


def reference_namespace():
    sys.argv = sys.argv[:1]                       # yi2018cvpr/config.py parses the command line
    sys.modules["cv2"] = types.ModuleType("cv2")
    torch.cholesky = torch.linalg.cholesky
    sys.path.insert(0, REF)
    from model.model import GMW                   # noqa: E402
    from lib.losses import correspondenceLoss     # noqa: E402
    from utilities.dataset_utilities import load_data  # noqa: E402
    import math
    tree = ast.parse(open(os.path.join(REF, "main.py")).read())
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name in ("compute_z", "get_up", "compute_reg_loss"))
            or (isinstance(n, ast.ClassDef) and n.name == "GMW_data")]
    ns = {"torch": torch, "np": np, "os": os, "json": json, "math": math}
    exec(compile(ast.Module(body=body, type_ignores=[]), "GMW/main.py", "exec"), ns)
    ns.update(GMW=GMW, correspondenceLoss=correspondenceLoss, load_data=load_data)
    return ns


def make_labels(result_texts, ids):
    """Label text per image + the smallest distance of any overlap from a threshold; re-seeded until that is >= CLEARANCE."""
    from dcd_amd.eval import kitti_annos
    from make_golden_eval import exact_overlaps, label_lines
    tmp = tempfile.mkdtemp()
    try:
        dts = []
        for img, text in zip(ids, result_texts):
            with open(os.path.join(tmp, img + ".txt"), "w") as f:
                f.write(text)
            dts.append(kitti_annos.read_anno(os.path.join(tmp, img + ".txt")))
        seed = 0
        while True:
            rng = np.random.RandomState(seed)
            texts, clear = [], np.inf
            for img, d in zip(ids, dts):
                n = len(d["name"])
                if n == 0:                                          # the image without detections: one car that is missed
                    g = dict(name=np.array(["Car"]), truncated=np.zeros(1), occluded=np.zeros(1, np.int64), alpha=np.array([0.3]),
                             bbox=np.array([[400.0, 150.0, 520.0, 230.0]]), dimensions=np.array([[3.9, 1.5, 1.6]]),
                             location=np.array([[2.0, 1.6, 25.0]]), rotation_y=np.array([0.4]))
                else:
                    g = dict(name=d["name"].copy(), truncated=np.zeros(n), occluded=np.zeros(n, np.int64),
                             alpha=d["alpha"] + rng.normal(0, 0.2, n), bbox=d["bbox"] + rng.normal(0, 1.0, (n, 4)),
                             dimensions=d["dimensions"] + rng.normal(0, 0.05, (n, 3)),
                             location=d["location"] + rng.normal(0, 0.10, (n, 3)),
                             rotation_y=d["rotation_y"] + rng.normal(0, 0.08, n))
                text = label_lines(g)
                texts.append(text)
                if n:
                    with open(os.path.join(tmp, "gt.txt"), "w") as f:
                        f.write(text)
                    gr = kitti_annos.read_anno(os.path.join(tmp, "gt.txt"))
                    bev, iou3d, _ = exact_overlaps(d, gr)
                    for ov in (bev, iou3d):
                        clear = min(clear, min(np.abs(ov - t).min() for t in (0.7, 0.5, 0.25)))
            print("labels: seed %d, clearance %.4f" % (seed, clear))
            if clear >= CLEARANCE:
                return texts, clear, seed
            seed += 1
    finally:
        shutil.rmtree(tmp)


def main():
    records = make_records()
    ns = reference_namespace()
    ids = [img for img, _ in IMAGES]
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(tmp, "training", "ImageSets"))
        with open(os.path.join(tmp, "training", "ImageSets", "val.txt"), "w") as f:
            f.write("".join(i + "\n" for i in ids))
        records_json = json.dumps(records, indent=4)
        with open(os.path.join(tmp, "gen_data_infer.json"), "w") as f:
            f.write(records_json)
        args = types.SimpleNamespace(kitti_path=tmp, val_data_path=os.path.join(tmp, "gen_data_infer.json"), log_dir=tmp,
                                     local_rank=0, gpu=None, test_all=False, cls_weight=0.1, reg_weight=1.0)
        data = ns["load_data"](args, "valid")
        kitti_eval = ns["GMW_data"](args)

        torch.manual_seed(0)
        model = ns["GMW"](None).eval()
        with torch.no_grad():
            kpts_2d, kpts_3d, pred_rot, raw_location, dim, img_idx = (torch.from_numpy(data[k]) for k in (
                "kpts_2d", "kpts_3d", "pred_rot", "gt_location", "dim", "img_idx"))
            # main.py:524-548
            pre_depths, good_idx = ns["compute_z"](kpts_2d, kpts_3d, pred_rot)
            raw_location = raw_location.clone()
            reg_weights, edge_P = model(kpts_2d, kpts_3d, pred_rot, args)
            reg_loss, pred_depth = ns["compute_reg_loss"](pre_depths, reg_weights, raw_location[:, -1], good_idx)
            raw_depth = raw_location[:, 2]
            scale = pred_depth / raw_depth
            h = dim[:, 0]
            raw_location[:, 1] -= h / 2
            pred_location = scale.unsqueeze(-1) * raw_location
            pred_location[:, 1] += h / 2
            kitti_eval.replace_location(pred_location, img_idx)
        texts = [open(os.path.join(kitti_eval.result_dir, i + ".txt")).read() for i in ids]
    finally:
        shutil.rmtree(tmp)

    labels, clear, label_seed = make_labels(texts, ids)
    out = {"records_json": np.array(records_json), "ids": np.array(ids), "result_texts": np.array(texts),
           "label_texts": np.array(labels), "label_clearance": np.float64(clear), "label_seed": np.int64(label_seed),
           "pred_depth": pred_depth.numpy(), "pred_location": pred_location.numpy()}
    for k in ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "dim", "img_idx"):
        out["loader_" + k] = data[k]
    np.savez_compressed(os.path.join(HERE, "gmw_infer.npz"), **out)
    print("gmw_infer.npz: pred_depth %s vs raw %s" % (out["pred_depth"], data["gt_location"][:, 2]))
    print("".join(texts))


if __name__ == "__main__":
    main()
