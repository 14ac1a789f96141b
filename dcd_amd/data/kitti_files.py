"""Reading a KITTI object-detection directory into what the device input pipeline takes: decoded uint8 frames and the raw label
values of `encode_targets` / `pack_raw`.  Host code (numpy / json / PIL), no GPU involved.

Restates the file side of the reference's `KITTIDataset` (DGDE/data/datasets/kitti.py): the image list of
`ImageSets/<split>.txt` (:48-56), `label_2/*.txt` parsed as `Object3d` does (kitti_utils.py:64-112, `read_label` :492-496) with
the key-point annotations of `kpts_ann/kpts_ann_<split>.json` matched by the `dim` distance (:100-112; 'trainval' and every
other split name merge the val and train files, kitti.py:119-127), the class whitelist `DATASETS.DETECT_CLASSES`
(`filtrate_objects`, :246-260), `P2` of `calib/*.txt` (kitti_utils.py:219-227, :269-289), and the training-time removal of images
without a kept object (kitti.py:130-141).  The annotation file is looked up under `root` (the reference opens it relative to the
working directory).

Right-camera views (kitti.py:63, :144-148, :276-296).  With `DATASETS.USE_RIGHT_IMAGE` a training list of N images has 2 N
indices: i < N is the left view of image i, i >= N the right view of image i - N, under the same `img_id`; the images without a
kept object are removed BEFORE the doubling.  With `DATASETS.INFER_ON_RIGHT_IMG` every index of an evaluation list is a right
view.  A right view decodes `image_3/<id>.png`, takes `P3` of the calibration file, and replaces every object's 2-D box by the
clipped projection of its eight corners through `P3`, stored as float32 exactly as kitti.py:287-293 stores it; such a sample
carries `box2d_float32=True`, which tells `flip_sample` to flip the box in the reference's float32 arithmetic.

An unlabelled split (`test`, kitti.py:281, :301, :338-352) needs `ImageSets/test.txt`, the images and `calib` only:
`has_labels` is False, neither `label_2` nor `kpts_ann` is opened, and every sample has zero objects.

Every label value stays float64 as parsed (the box of a left view included: the flip needs it, dcd_amd/data/augment.py), except
`t`, which `Object3d` keeps as a float32 array and from which it derives `alpha`."""
import json
import os

import numpy as np

from dcd_amd.data.augment import convert_rot_to_alpha

TYPE_ID_CONVERSION = {"Car": 0, "Pedestrian": 1, "Cyclist": 2, "Van": -4, "Truck": -4, "Person_sitting": -2, "Tram": -99,
                      "Misc": -99, "DontCare": -1}                  # kitti.py:394-404


def parse_label_line(line, anns, n_extra):
    """One line of a label_2 file -> dict of the values an `Object3d` holds (kitti_utils.py:64-112)."""
    data = line.split(" ")
    v = [float(x) for x in data[1:]]                                # v[k] = data[k + 1]
    h, w, l = v[7], v[8], v[9]
    t = np.array((v[10], v[11], v[12]), dtype=np.float32)
    ry = v[13]
    for ann in anns:
        if np.linalg.norm(np.array(ann["dim"]) - np.array([h, w, l])) < 0.05 and ann["find_pcl"]:
            kpts3d = np.array(ann["3dkeypoints"], dtype=np.float64).reshape(-1, 3)
            find_pcl = 1
            break
    else:
        kpts3d = np.zeros((n_extra, 3)) - 1.
        find_pcl = 0
    kpts3d[:, 1] -= h / 2
    return dict(type=data[0], trunc_occ=(v[0], float(int(v[1]))), box2d=(v[3], v[4], v[5], v[6]), hwl=(h, w, l), t=t, ry=ry,
                alpha=convert_rot_to_alpha(ry, t[2], t[0]), find_pcl=find_pcl, kpts3d=kpts3d)


def read_p(path, key):
    """The projection matrix named `key` ("P2", "P3", ...) of a KITTI calibration file as a (3, 4) float64 matrix."""
    with open(path, "r") as f:
        for line in f:
            line = line.rstrip()
            if line:
                name, value = line.split(":", 1)
                if name == key:
                    return np.array([float(x) for x in value.split()], dtype=np.float64).reshape(3, 4)
    raise ValueError("%s has no %s line" % (path, key))


def read_p2(path):
    """`P2` of a KITTI calibration file as a (3, 4) float64 matrix."""
    return read_p(path, "P2")


def corners_3d(hwl, ry, t):
    """The eight corners of an object's 3-D box in camera coordinates, (8, 3) float64: `Object3d.generate_corners3d`
    (kitti_utils.py:131-151), with the same numpy calls so that the sums come out in the same order."""
    h, w, l = hwl
    x = [l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2]
    y = [0, 0, 0, 0, -h, -h, -h, -h]
    z = [w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2]
    R = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    return np.dot(R, np.vstack([x, y, z])).T + t


def projected_box(obj, P, image_size):
    """The 2-D box of a right view (kitti.py:286-293): the projection of the eight corners through `P`, clipped to the image,
    as a float32 array (xmin, ymin, xmax, ymax)."""
    img_w, img_h = image_size
    c = corners_3d(obj["hwl"], obj["ry"], obj["t"])
    uv = np.dot(np.hstack((c, np.ones((c.shape[0], 1)))), np.transpose(P))      # `project_rect_to_image`, kitti_utils.py:361-369
    uv[:, 0] /= uv[:, 2]
    uv[:, 1] /= uv[:, 2]
    return np.array([max(uv[:, 0].min(), 0), max(uv[:, 1].min(), 0), min(uv[:, 0].max(), img_w - 1), min(uv[:, 1].max(), img_h - 1)],
                    dtype=np.float32)


class KittiFiles:
    def __init__(self, root, split, cfg, is_train=True):
        self.root, self.split, self.is_train = root, split, is_train
        self.has_labels = split != "test"
        if is_train and not self.has_labels:
            raise ValueError("the %r split has no labels: it cannot be trained on (is_train=True)" % split)
        self.use_right = bool(cfg.DATASETS.USE_RIGHT_IMAGE) and bool(is_train)               # kitti.py:63
        self.infer_right = bool(cfg.DATASETS.INFER_ON_RIGHT_IMG) and not is_train
        self.classes = tuple(cfg.DATASETS.DETECT_CLASSES)
        self.n_extra = cfg.MODEL.HEAD.EXTRA_KPTS_NUM
        with open(os.path.join(root, "ImageSets", "%s.txt" % split), "r") as f:
            self.ids = [line.replace("\n", "") for line in f]
        self.ids = [i for i in self.ids if i]

        def ann_file(name):
            with open(os.path.join(root, "kpts_ann", "kpts_ann_%s.json" % name), "r") as f:
                return json.load(f)
        if not self.has_labels:
            self.kpts_ann = {}
        elif split in ("val", "train"):
            self.kpts_ann = ann_file(split)
        else:
            self.kpts_ann = ann_file("val")
            self.kpts_ann.update(ann_file("train"))
        if is_train:                                                # kitti.py:130-141, before the doubling of :144-148
            self.ids = [name for name in self.ids if self._objects(name)]

    def _objects(self, name):
        if not self.has_labels:
            return []
        anns = self.kpts_ann[str(int(name[-6:]))]                   # kitti.py:167
        with open(os.path.join(self.root, "label_2", name + ".txt"), "r") as f:
            lines = [line.rstrip() for line in f]
        objs = [parse_label_line(line, anns, self.n_extra) for line in lines if line]
        return [o for o in objs if o["type"] in self.classes]

    def __len__(self):
        return 2 * len(self.ids) if self.use_right else len(self.ids)

    def _view(self, i):
        """(position in `ids`, is it a right view) of index i (kitti.py:276-278)."""
        n = len(self.ids)
        if self.use_right and i >= n:
            if i >= 2 * n:
                raise IndexError("view %d of %d images with both cameras" % (i, n))
            return i - n, True
        return i, self.infer_right

    def is_right(self, i):
        return self._view(i)[1]

    def img_id(self, i):
        return self.ids[self._view(i)[0]]

    def _image(self, i):
        from PIL import Image
        j, right = self._view(i)
        return Image.open(os.path.join(self.root, "image_3" if right else "image_2", self.ids[j] + ".png"))

    def frame(self, i):
        """The decoded image: (h, w, 3) uint8 RGB."""
        return np.array(self._image(i).convert("RGB"), dtype=np.uint8)

    def sample(self, i):
        """The raw-value dict of view i (`image_size` (w, h) from the image file's header)."""
        j, right = self._view(i)
        with self._image(i) as im:
            image_size = im.size
        objs = self._objects(self.ids[j])
        n = len(objs)
        P = read_p(os.path.join(self.root, "calib", self.ids[j] + ".txt"), "P3" if right else "P2")

        def col(key, shape, dtype=np.float64):
            return np.array([o[key] for o in objs], dtype=dtype).reshape((n,) + shape)
        out = dict(image_size=np.array(image_size, dtype=np.int64), P=P,
                   trunc_occ=col("trunc_occ", (2,)), box2d=col("box2d", (4,)), hwl=col("hwl", (3,)), t=col("t", (3,), np.float32),
                   ry=col("ry", ()), alpha=col("alpha", ()), find_pcl=col("find_pcl", (), np.int32),
                   kpts3d=col("kpts3d", (self.n_extra, 3)), cls=np.array([TYPE_ID_CONVERSION[o["type"]] for o in objs], dtype=np.int32))
        if right:
            out["box2d"] = np.array([projected_box(o, P, image_size) for o in objs], dtype=np.float32).reshape(n, 4)
            out["box2d_float32"] = True                             # `flip_sample` then flips the box as the reference does
        return out
