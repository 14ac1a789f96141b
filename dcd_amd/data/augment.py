"""The label half of the reference's only training augmentation, `RandomHorizontallyFlip.__call__`
(DGDE/data/augmentations/augmentations.py:28-87), restated on the raw-value dict `encode_targets` / `pack_raw` take
(image_size, P, trunc_occ, box2d, hwl, t, ry, alpha, find_pcl, kpts3d[, cls]).  The image half runs on the device
(csrc/images.hip).  A pure function of the raw values: the reference mutates its `Object3d` records and the calibration in
place; here a new dict comes back and the input is left alone.

Types follow the reference: the box is flipped in float64 from the values given (`obj.xmin` / `obj.xmax` are the parsed
floats, not the float32 `box2d`); it stays float64 in the result, as `obj.xmin` does, and is rounded to float32 where the
encoder packs it (`pack_raw`), which is where `obj.box2d` is rounded.  Rounding the box first and flipping it then can land
one float32 step away.  The one exception is a sample marked `box2d_float32=True` (a right-camera view of
`KittiFiles`): the reference overwrites `obj.xmin .. obj.ymax` of such a view with float32 scalars, so its flip runs in float32
under NumPy >= 2, the NumPy that wrote tests/golden/right_views.npz; that box is flipped in float32 here and stays float32.
`t` is the float32 array `Object3d` keeps, `ry` / `alpha` are Python floats.  `kpts3d` is NOT mirrored: the reference leaves the object-frame key points alone (its own comment at
augmentations.py:71), and tests/golden/target_encoding_flipped.npz pins that."""
import math

import numpy as np


def convert_rot_to_alpha(ry3d, z3d, x3d):
    """`convertRot2Alpha` (DGDE/data/datasets/kitti_utils.py:31-40)."""
    alpha = ry3d - math.atan2(x3d, z3d)
    while alpha > math.pi:
        alpha -= math.pi * 2
    while alpha < (-math.pi):
        alpha += math.pi * 2
    return alpha


def flip_sample(sample):
    """Raw label values of one image -> the values after a horizontal flip (a new dict; arrays are copies)."""
    img_w = int(sample["image_size"][0])
    out = dict(sample)
    if sample.get("box2d_float32", False):
        # a right view (kitti.py:290-293): `obj.xmin .. obj.ymax` are float32 scalars there, and NumPy >= 2 keeps
        # `int - float32 - int` in float32 (the Python integers are weak), one rounding per operation
        box = np.array(sample["box2d"], dtype=np.float32).reshape(-1, 4)
        w = box[:, 2] - box[:, 0]
        box[:, 0] = np.float32(img_w) - box[:, 2] - np.float32(1)
        box[:, 2] = box[:, 0] + w
    else:
        box = np.array(sample["box2d"], dtype=np.float64).reshape(-1, 4)
        w = box[:, 2] - box[:, 0]                                   # augmentations.py:47-50
        box[:, 0] = img_w - box[:, 2] - 1
        box[:, 2] = box[:, 0] + w
    out["box2d"] = box                                              # float32 where the encoder packs it, like `obj.box2d` (:50)
    t = np.array(sample["t"], dtype=np.float32).reshape(-1, 3)      # :68-70
    t[:, 0] = -t[:, 0]
    out["t"] = t
    ry = np.array(sample["ry"], dtype=np.float64).reshape(-1)
    alpha = np.empty_like(ry)
    for i in range(len(ry)):
        r = float(ry[i])
        r = (-math.pi - r) if r < 0 else (math.pi - r)              # :53-57
        while r > math.pi:
            r -= math.pi * 2
        while r < (-math.pi):
            r += math.pi * 2
        ry[i] = r
        alpha[i] = convert_rot_to_alpha(r, t[i, 2], t[i, 0])        # :73
    out["ry"], out["alpha"] = ry, alpha
    P = np.array(sample["P"], dtype=np.float64).reshape(3, 4)       # :81-83
    P[0, 2] = img_w - P[0, 2] - 1
    P[0, 3] = -P[0, 3]
    out["P"] = P
    return out
