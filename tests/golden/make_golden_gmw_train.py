"""Generates tests/golden/gmw_train.npz by RUNNING THE REFERENCE'S `load_data` (GMW/utilities/dataset_utilities.py:11-36) on a
ragged `gen_data_train.json`: 3 iterations holding 2, 0 and 3 objects of 73 keypoints.

Run in the build container only (`python tests/golden/make_golden_gmw_train.py`, its own process).  Nothing is copied: the module is
imported where it lies (set GMW_REFERENCE to the reference's GMW directory); `tqdm`, imported there and never called on this path,
gets an empty stand-in when it is not installed, as `cv2` does in make_golden_gmw.py.
The JSON comes from `records()`, which the test shares; values are float64 with more digits than float32 holds, so the fixture
also pins where the rounding happens.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GMW_REFERENCE", "/root/reference/GMW")
COUNTS = (2, 0, 3)


def records(seed=3, counts=COUNTS, K=73):
    """The parsed JSON: {'kpts_2d': [iteration][object][K][2], 'kpts_3d': [..][K][3], 'pred_rot': [..], 'gt_location': [..][3]}."""
    rng = np.random.default_rng(seed)
    out = {"kpts_2d": [], "kpts_3d": [], "pred_rot": [], "gt_location": []}
    for n in counts:
        out["kpts_2d"].append((rng.random((n, K, 2)) - 0.5).tolist())
        out["kpts_3d"].append(((rng.random((n, K, 3)) - 0.5) * 4).tolist())
        out["pred_rot"].append((rng.random(n) * 2 * np.pi - np.pi).tolist())
        out["gt_location"].append((rng.random((n, 3)) * 40 + 2).tolist())
    return out


def main():
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stand_in = types.ModuleType("tqdm")
        stand_in.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = stand_in
    sys.path.insert(0, REF)
    from utilities.dataset_utilities import load_data      # noqa: E402
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gen_data_train.json")
        with open(path, "w") as f:
            json.dump(records(), f)
        data = load_data(types.SimpleNamespace(train_data_path=path), "train")
    out = {k: data[k] for k in ("kpts_2d", "kpts_3d", "pred_rot", "gt_location")}
    np.savez_compressed(os.path.join(HERE, "gmw_train.npz"), **out)
    print("gmw_train.npz:", {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
