"""Reading a KITTI object-detection directory into what the device input pipeline takes: decoded uint8 frames and the raw label
values of `encode_targets` / `pack_raw`.  Host code (numpy / json / PIL), no GPU involved.

Restates the file side of the reference's `KITTIDataset` (DGDE/data/datasets/kitti.py): the image list of
`ImageSets/<split>.txt` (:48-56), `label_2/*.txt` parsed as `Object3d` does (kitti_utils.py:64-112, `read_label` :492-496) with
the key-point annotations of `kpts_ann/kpts_ann_<split>.json` matched by the `dim` distance (:100-112; 'trainval' and every
other split name merge the val and train files, kitti.py:119-127), the class whitelist `DATASETS.DETECT_CLASSES`
(`filtrate_objects`, :246-260), `P2` of `calib/*.txt` (kitti_utils.py:219-227, :269-289), and the training-time removal of images
without a kept object (kitti.py:130-141).  The annotation file is looked up under `root` (the reference opens it relative to the
working directory).  Right-camera images and a `test` split without labels are not supported.

Every label value stays float64 as parsed (the box included: the flip needs it, dcd_amd/data/augment.py), except `t`, which
`Object3d` keeps as a float32 array and from which it derives `alpha`."""
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


def read_p2(path):
    """`P2` of a KITTI calibration file as a (3, 4) float64 matrix."""
    with open(path, "r") as f:
        for line in f:
            line = line.rstrip()
            if line:
                key, value = line.split(":", 1)
                if key == "P2":
                    return np.array([float(x) for x in value.split()], dtype=np.float64).reshape(3, 4)
    raise ValueError("%s has no P2 line" % path)


class KittiFiles:
    def __init__(self, root, split, cfg, is_train=True):
        self.root, self.split, self.is_train = root, split, is_train
        if split == "test":
            raise NotImplementedError("the test split has no labels; KittiFiles reads labelled splits only")
        self.classes = tuple(cfg.DATASETS.DETECT_CLASSES)
        self.n_extra = cfg.MODEL.HEAD.EXTRA_KPTS_NUM
        with open(os.path.join(root, "ImageSets", "%s.txt" % split), "r") as f:
            self.ids = [line.replace("\n", "") for line in f]
        self.ids = [i for i in self.ids if i]

        def ann_file(name):
            with open(os.path.join(root, "kpts_ann", "kpts_ann_%s.json" % name), "r") as f:
                return json.load(f)
        if split in ("val", "train"):
            self.kpts_ann = ann_file(split)
        else:
            self.kpts_ann = ann_file("val")
            self.kpts_ann.update(ann_file("train"))
        if is_train:                                                # kitti.py:130-141
            self.ids = [name for name in self.ids if self._objects(name)]

    def _objects(self, name):
        anns = self.kpts_ann[str(int(name[-6:]))]                   # kitti.py:167
        with open(os.path.join(self.root, "label_2", name + ".txt"), "r") as f:
            lines = [line.rstrip() for line in f]
        objs = [parse_label_line(line, anns, self.n_extra) for line in lines if line]
        return [o for o in objs if o["type"] in self.classes]

    def __len__(self):
        return len(self.ids)

    def img_id(self, i):
        return self.ids[i]

    def _image(self, i):
        from PIL import Image
        return Image.open(os.path.join(self.root, "image_2", self.ids[i] + ".png"))

    def frame(self, i):
        """The decoded image: (h, w, 3) uint8 RGB."""
        return np.array(self._image(i).convert("RGB"), dtype=np.uint8)

    def sample(self, i):
        """The raw-value dict of image i (`image_size` (w, h) from the image file's header)."""
        with self._image(i) as im:
            image_size = im.size
        objs = self._objects(self.ids[i])
        n = len(objs)

        def col(key, shape, dtype=np.float64):
            return np.array([o[key] for o in objs], dtype=dtype).reshape((n,) + shape)
        return dict(image_size=np.array(image_size, dtype=np.int64), P=read_p2(os.path.join(self.root, "calib", self.ids[i] + ".txt")),
                    trunc_occ=col("trunc_occ", (2,)), box2d=col("box2d", (4,)), hwl=col("hwl", (3,)), t=col("t", (3,), np.float32),
                    ry=col("ry", ()), alpha=col("alpha", ()), find_pcl=col("find_pcl", (), np.int32),
                    kpts3d=col("kpts3d", (self.n_extra, 3)), cls=np.array([TYPE_ID_CONVERSION[o["type"]] for o in objs], dtype=np.int32))
