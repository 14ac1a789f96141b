"""Fixtures of the right-camera views and of the unlabelled `test` split (dcd_amd/data/kitti_files.py, the float32 branch of
dcd_amd/data/augment.py), produced by RUNNING THE REFERENCE'S OWN `KITTIDataset` where it lies, in the style of
make_golden_input.py (same stand-in modules, the objects of make_golden_targets.scenes() as templates; .npz / text / PNG data
only, nothing of the reference's program text is stored).  Build container only.

Writes
  kitti_right/      a KITTI directory at a 96 x 32 canvas (INPUT.WIDTH_TRAIN x HEIGHT_TRAIN, as input_images.npz): ImageSets/
                    {train,test}.txt, label_2, calib, kpts_ann and seeded-noise PNGs in image_2 and image_3.  `P3` differs from `P2`
                    in KITTI's own way (P[0, 3] / P[0, 0] = -0.47 against +0.062).  Four images: 000000 (96 x 32) holds an object
                    whose right-view projection lies inside the image, one clipped at the left, one at the right, one at the
                    bottom, one at the top, a 'Van' and a 'DontCare'; 000001 (77 x 25) and 000003 (58 x 26) hold cars (one without
                    point-cloud key points), a 'Pedestrian' and a 'Cyclist', which DGDE.yaml's DETECT_CLASSES drops; 000002 holds
                    only a 'Van' and a 'DontCare', so training removes it before the doubling.  Every corner of every kept object
                    has z > 0 (asserted below).  There are enough right-view boxes that the flip in float32 and the flip in
                    float64 land on different float32 values for at least one of them (tests/test_right_views_host.py asserts it).
  right_views.npz   `numpy_version`; for every index i of `KITTIDataset(is_train=True, augment=True)` under
                    DATASETS.USE_RIGHT_IMAGE: `in<i>_*` the raw values the reference holds after `filtrate_objects` with its flip
                    not drawn (box2d: the float32 `obj.box2d`; xyxy: `obj.xmin .. obj.ymax` in the dtype the reference holds them
                    in -- float64 as parsed for a left view, float32 for a right view), `in<i>_P` = `Calibration.P`,
                    `out<i>_*` every ParamsList field unflipped; `fin<i>_*`, `flipP<i>`, `flip<i>_*` the same with the reference's
                    own flip drawn (`random` seeded, the reference is not patched: the augmentation object is only wrapped by a
                    recorder that copies what it returns).  `test<j>_*`: the fields of the reference's test-mode target
                    (`split='test'`, is_train=False) of image j."""
import copy
import itertools
import json
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_targets as mt  # noqa: E402

IN_W, IN_H = 96, 32
F = 60.0
P2_A = np.array([[F, 0.0, 46.9, 0.062 * F], [0.0, F, 15.5, 0.018], [0.0, 0.0, 1.0, 0.002745884]])
P3_A = np.array([[F, 0.0, 46.9, -0.47 * F], [0.0, F, 15.5, 0.0021], [0.0, 0.0, 1.0, 0.003]])
P2_B = np.array([[58.8, 0.0, 38.2, 0.065 * 58.8], [0.0, 58.8, 12.1, -0.029], [0.0, 0.0, 1.0, 0.004981016]])
P3_B = np.array([[58.8, 0.0, 38.2, -0.468 * 58.8], [0.0, 58.8, 12.1, 0.0032], [0.0, 0.0, 1.0, 0.0041]])


def scenes():
    """[(image (w, h), P2, P3, [object dict])]: the objects of make_golden_targets.scenes() (dimensions, key points) moved to
    where a 96 x 32 image at a focal length of 60 px sees them."""
    pool = [o for _, _, objs in mt.scenes() for o in objs if o["type"] == "Car"]
    taken = itertools.cycle(pool)                   # (a template may serve two images: the annotations are looked up per image)

    def put(x, z, ry, typ="Car", trunc=0.0, occ=0, y=1.65, pcl=True):
        o = copy.deepcopy(next(taken))
        o.update(type=typ, trunc=trunc, occ=occ, t=(round(x, 2), round(y, 2), round(z, 2)), ry=round(ry, 2), box=None, pcl=pcl)
        return o
    out = []
    out.append(((96, 32), P2_A, P3_A, [
        put(0.4, 15.0, 0.3),                        # inside the image in both views
        put(-10.5, 14.0, 0.1, trunc=0.5),           # the right view cuts it at the left edge
        put(11.0, 15.0, -0.2, trunc=0.4),           # ... at the right edge
        put(0.2, 5.0, 0.05, trunc=0.3),             # ... at the bottom edge
        put(1.0, 8.0, 1.4, y=-1.0),                 # ... at the top edge
        put(3.0, 12.0, -1.7, typ="Van"), put(0.0, 20.0, 0.0, typ="DontCare")]))
    out.append(((77, 25), P2_B, P3_B, [put(-1.5, 12.0, 1.2, typ="Pedestrian"), put(2.0, 18.0, -0.4, typ="Cyclist", occ=1),
                                       put(0.5, 25.0, 2.9, pcl=False), put(-3.1, 13.0, 0.6), put(4.2, 17.0, -1.1),
                                       put(-6.3, 21.0, 2.2, occ=1)]))
    out.append(((96, 32), P2_A, P3_A, [put(1.0, 9.0, -1.7, typ="Van"), put(0.0, 20.0, 0.0, typ="DontCare")]))
    out.append(((58, 26), P2_B, P3_B, [put(0.3, 16.0, -3.0), put(-2.0, 22.0, 0.7, occ=2), put(3.7, 19.0, 1.9),
                                       put(-4.4, 24.0, -0.8), put(1.9, 11.0, 0.2, trunc=0.2)]))
    return out


def write_directory(root, sc):
    """make_golden_targets.write_dataset's label_2 / kpts_ann / ImageSets texts (boxes from `P2`), then this fixture's own calib
    files (`P3` distinct), seeded-noise PNGs for both cameras and ImageSets/test.txt."""
    from PIL import Image
    mt.write_dataset(root, [(img, P2, objs) for img, P2, _, objs in sc])
    os.makedirs(os.path.join(root, "image_3"), exist_ok=True)
    rng = np.random.RandomState(23)
    for i, (img, P2, P3, _) in enumerate(sc):
        name = "%06d" % i
        with open(os.path.join(root, "calib", name + ".txt"), "w") as f:
            flat = {k: " ".join("%.12e" % v for v in P.reshape(-1)) for k, P in (("P0", P2), ("P1", P2), ("P2", P2), ("P3", P3))}
            f.write("P0: %s\nP1: %s\nP2: %s\nP3: %s\n" % (flat["P0"], flat["P1"], flat["P2"], flat["P3"]))
            f.write("R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 1 0 0 0 0 1 0 0 0 0 1 0\nTr_imu_to_velo: 1 0 0 0 0 1 0 0 0 0 1 0\n")
        for d in ("image_2", "image_3"):
            noise = rng.randint(0, 256, (img[1], img[0], 3)).astype(np.uint8)
            Image.fromarray(noise, mode="RGB").save(os.path.join(root, d, name + ".png"))
    shutil.copy(os.path.join(root, "ImageSets", "train.txt"), os.path.join(root, "ImageSets", "test.txt"))


def raw_values(objs, prefix, out):
    n = len(objs)
    out[prefix + "n"] = np.array(n)
    out[prefix + "type"] = np.array([o.type for o in objs])
    out[prefix + "trunc_occ"] = np.array([[o.truncation, float(o.occlusion)] for o in objs], np.float64).reshape(n, 2)
    out[prefix + "box2d"] = np.array([o.box2d for o in objs]).reshape(n, 4)
    assert out[prefix + "box2d"].dtype == np.float32
    xyxy = [np.asarray([o.xmin, o.ymin, o.xmax, o.ymax]) for o in objs]       # numpy's own choice of dtype for the four scalars
    assert len({a.dtype for a in xyxy}) == 1
    out[prefix + "xyxy"] = np.stack(xyxy).reshape(n, 4)
    out[prefix + "hwl"] = np.array([[o.h, o.w, o.l] for o in objs], np.float64).reshape(n, 3)
    out[prefix + "t"] = np.array([o.t for o in objs], np.float32).reshape(n, 3)
    out[prefix + "ry"] = np.array([o.ry for o in objs], np.float64)
    out[prefix + "alpha"] = np.array([o.alpha for o in objs], np.float64)
    out[prefix + "find_pcl"] = np.array([o.find_pcl for o in objs], np.int32)
    out[prefix + "kpts3d"] = np.array([o.extra_kpts_3D for o in objs], np.float64).reshape(n, mt.N_EXTRA, 3)


def target_fields(target, prefix, out):
    for name in target.fields():
        if name in ("calib", "ori_img", "img_idx"):
            continue
        out[prefix + name] = np.asarray(target.get_field(name))
    out[prefix + "size"] = np.array(target.size)


class Recorder:
    """Stands where the data set keeps its augmentation: calls it, and keeps a copy of the objects it returns."""

    def __init__(self, inner):
        self.inner, self.objs = inner, None

    def __call__(self, img, objs, calib):
        img, objs, calib = self.inner(img, objs, calib)
        self.objs = copy.deepcopy(objs)
        return img, objs, calib


def golden_right_views(root, sc):
    from data.datasets.kitti import KITTIDataset
    cfg = mg.ref_cfg(["INPUT.WIDTH_TRAIN", IN_W, "INPUT.HEIGHT_TRAIN", IN_H, "DATASETS.USE_RIGHT_IMAGE", True])
    flip_seed = next(s for s in range(100) if random.Random(s).random() < 0.5)
    keep_seed = next(s for s in range(100) if random.Random(s).random() >= 0.5)
    ds = KITTIDataset(cfg, root, is_train=True, transforms=None, augment=True)
    ds.augmentation = rec = Recorder(ds.augmentation)
    N = ds.num_samples
    assert len(ds) == 2 * N and N == 3, (len(ds), N)
    out = {"numpy_version": np.array(np.__version__), "input_size": np.array([IN_W, IN_H]), "n_images": np.array(N),
           "n_views": np.array(len(ds)), "kept": np.array([f[:-4] for f in ds.image_files])}
    front = True
    for i in range(len(ds)):
        right = i >= N
        random.seed(keep_seed)
        img, target, idx = ds[i]
        assert idx == ds.image_files[i % N][:-4]
        P = np.asarray(target.get_field("calib").P, np.float64)
        w, h = sc[int(idx)][0]
        out["in%d_id" % i], out["in%d_is_right" % i] = np.array(idx), np.array(right)
        out["in%d_image_size" % i], out["in%d_P" % i] = np.array([w, h]), P
        assert (P == ds.get_calibration(i % N, use_right_cam=right).P).all()   # (np.testing is unusable under the np.bool alias)
        raw_values(rec.objs, "in%d_" % i, out)
        assert out["in%d_xyxy" % i].dtype == (np.float32 if right else np.float64)
        target_fields(target, "out%d_" % i, out)
        for o in rec.objs:
            front &= bool((o.generate_corners3d()[:, 2] > 0).all())
        random.seed(flip_seed)
        img, target, idx = ds[i]
        fP = np.asarray(target.get_field("calib").P, np.float64)
        assert fP[0, 3] == -P[0, 3] and fP[0, 2] != P[0, 2], "the reference did not flip"
        out["flipP%d" % i] = fP
        raw_values(rec.objs, "fin%d_" % i, out)
        target_fields(target, "flip%d_" % i, out)
    assert front, "a kept object has a corner behind the camera"
    return out


def golden_test_split(root, out):
    from data.datasets.kitti import KITTIDataset
    cfg = mg.ref_cfg(["INPUT.WIDTH_TRAIN", IN_W, "INPUT.HEIGHT_TRAIN", IN_H, "DATASETS.TEST_SPLIT", "test"])
    ds = KITTIDataset(cfg, root, is_train=False, transforms=None, augment=False)
    out["test_n"] = np.array(len(ds))
    for j in range(len(ds)):
        img, target, idx = ds[j]
        assert sorted(target.fields()) == ["calib", "edge_indices", "edge_len", "final_output_h", "final_output_w", "ori_img", "pad_size"]
        out["test%d_id" % j] = np.array(idx)
        out["test%d_P" % j] = np.asarray(target.get_field("calib").P, np.float64)
        for name in ("pad_size", "edge_len", "edge_indices", "final_output_w", "final_output_h"):
            out["test%d_%s" % (j, name)] = np.asarray(target.get_field(name))


def main():
    mg.install_stubs()
    for name in ("matplotlib", "matplotlib.pyplot"):            # imported at module level by kitti.py, unused on this path
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    np.bool, np.int, np.bool8, np.float = bool, int, np.bool_, float        # aliases numpy 2 removed (kitti.py:367,386,505)
    sys.path.insert(0, mg.REF)
    sc = scenes()
    dst = os.path.join(HERE, "kitti_right")
    with tempfile.TemporaryDirectory() as tmp:
        write_directory(tmp, sc)
        with open(os.path.join(tmp, "kpts_ann", "kpts_ann_val.json"), "w") as f:      # the reference's 'test' branch opens both files;
            json.dump({}, f)                                                           # this one stays in the temporary directory
        os.chdir(tmp)                                            # kitti.py opens 'kpts_ann/kpts_ann_train.json' relative to the cwd
        out = golden_right_views(tmp, sc)
        golden_test_split(tmp, out)
        os.chdir(HERE)
        os.remove(os.path.join(tmp, "kpts_ann", "kpts_ann_val.json"))
        if os.path.isdir(dst):
            shutil.rmtree(dst)
        for d in ("label_2", "calib", "ImageSets", "kpts_ann", "image_2", "image_3"):
            shutil.copytree(os.path.join(tmp, d), os.path.join(dst, d))
    path = os.path.join(HERE, "right_views.npz")
    np.savez_compressed(path, **out)
    N = int(out["n_images"])
    print("numpy %s; wrote kitti_right/ (%d images, the reference keeps %s) and right_views.npz %.1f KB" %
          (np.__version__, len(sc), list(out["kept"]), os.path.getsize(path) / 1024))
    for i in range(2 * N):
        print("view %d %s right=%d kept %d trunc %d box2d\n%s" % (i, out["in%d_id" % i], out["in%d_is_right" % i], int(out["out%d_reg_mask" % i].sum()),
                                                                int(out["out%d_trunc_mask" % i].sum()), out["in%d_box2d" % i]))


if __name__ == "__main__":
    main()
