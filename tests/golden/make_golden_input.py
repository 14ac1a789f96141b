"""Fixtures of the device input pipeline (dcd_amd/data/{input_pipeline,augment,kitti_files}.py, csrc/images.hip), produced by
RUNNING THE REFERENCE'S OWN CODE where it lies, in the style of make_golden_targets.py (same stand-in modules, same fabricated
scenes; .npz / text data only, nothing of the reference's program text is stored).  Build container only.

One thing has to be supplied beyond make_golden.install_stubs: `torchvision` is absent in this image, and the reference's
DGDE/data/transforms/transforms.py calls `torchvision.transforms.functional.to_tensor` / `.normalize`.  The stand-in module
gets them as the two torch expressions torchvision itself applies to a uint8 HWC image --
`from_numpy(img).permute(2, 0, 1).contiguous().float().div(255)` and `.sub(mean[:, None, None]).div(std[:, None, None])` with
`mean` / `std` as fp32 tensors.  Everything the reference itself owns runs as the reference's code: the flip
(`RandomHorizontallyFlip`), `KITTIDataset.pad_image`, `build_transforms` with the `[2, 1, 0]` permutation and its order relative to
the normalisation, and the config values (PIXEL_MEAN / PIXEL_STD / TO_BGR / AUG_PARAMS).

Writes
  input_images.npz            four frames of seeded uint8 noise at a 96 x 32 input (77 x 25: pad (9, 3); 58 x 26: pad (19, 3), KITTI's
                              own odd pad_x; 96 x 32: no pad; 95 x 32: pad 0 left, one border column right); the first 256 pixels of the
                              96 x 32 frame hold, per channel, the ramp (arange(256) + 85 channel) % 256, so all 768 table entries
                              occur; per frame the reference's output unflipped / flipped for TO_BGR False / True (16 tensors).
  target_encoding_flipped.npz the three scenes of make_golden_targets.py through `KITTIDataset(..., augment=True)[i]` with
                              `random` seeded so that the reference's own draw comes out below 0.5 (the reference is not
                              patched); inputs are the UNFLIPPED raw values (box in float64: xmin, ymin, xmax, ymax as parsed),
                              outputs every ParamsList field, `flipP<i>` the flipped calibration matrix.
  kitti_files/                label_2, calib, ImageSets, kpts_ann texts of those scenes plus a fourth holding only a 'Van' and a
                              'DontCare', as written for the reference to read, and kitti_files.npz: the reference's own parse
                              (`filtrate_objects(read_label(...))`, `Calibration.P`) per image and the image list its
                              `KITTIDataset(is_train=True)` keeps."""
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_targets as mt  # noqa: E402

IN_W, IN_H = 96, 32
FRAME_SIZES = ((77, 25), (58, 26), (96, 32), (95, 32))      # (w, h)


def frames():
    rng = np.random.RandomState(11)
    out = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in FRAME_SIZES]
    ramp = (np.arange(256)[:, None] + 85 * np.arange(3)[None, :]) % 256
    out[2].reshape(-1, 3)[:256] = ramp.astype(np.uint8)
    return out


def install_torchvision_functional():
    F = sys.modules["torchvision.transforms.functional"]

    def to_tensor(pic):
        return torch.from_numpy(np.array(pic)).permute(2, 0, 1).contiguous().float().div(255)

    def normalize(tensor, mean, std):
        mean = torch.as_tensor(mean, dtype=tensor.dtype)
        std = torch.as_tensor(std, dtype=tensor.dtype)
        return tensor.sub(mean[:, None, None]).div(std[:, None, None])
    F.to_tensor, F.normalize = to_tensor, normalize
    sys.modules["torchvision.transforms"].functional = F


def golden_images():
    from PIL import Image
    from data.augmentations.augmentations import RandomHorizontallyFlip
    from data.datasets.kitti import KITTIDataset
    from data.transforms import build_transforms
    canvas = types.SimpleNamespace(input_height=IN_H, input_width=IN_W)
    out = {"input_size": np.array([IN_W, IN_H])}
    for i, f in enumerate(frames()):
        out["frame%d" % i] = f
        for flip in (0, 1):
            img = Image.fromarray(f, mode="RGB")
            if flip:
                img, _, _ = RandomHorizontallyFlip(2.0)(img, None, types.SimpleNamespace(P=mt.P2.copy()))      # p > 1: always
            img, pad = KITTIDataset.pad_image(canvas, img)
            assert tuple(pad) == ((IN_W - f.shape[1]) // 2, (IN_H - f.shape[0]) // 2)
            for bgr in (0, 1):
                cfg = mg.ref_cfg(["INPUT.TO_BGR", bool(bgr)])
                t, _ = build_transforms(cfg)(img, None)
                assert t.dtype == torch.float32 and tuple(t.shape) == (3, IN_H, IN_W)
                out["out%d_flip%d_bgr%d" % (i, flip, bgr)] = t.numpy()
    path = os.path.join(HERE, "input_images.npz")
    np.savez_compressed(path, **out)
    print("wrote input_images.npz %.1f KB" % (os.path.getsize(path) / 1024))


def raw_values(objs, prefix, out):
    out[prefix + "n"] = np.array(len(objs))
    out[prefix + "trunc_occ"] = np.array([[o.truncation, float(o.occlusion)] for o in objs], np.float64).reshape(-1, 2)
    out[prefix + "box2d"] = np.array([[o.xmin, o.ymin, o.xmax, o.ymax] for o in objs], np.float64).reshape(-1, 4)      # as parsed
    out[prefix + "hwl"] = np.array([[o.h, o.w, o.l] for o in objs], np.float64).reshape(-1, 3)
    out[prefix + "t"] = np.array([o.t for o in objs], np.float32).reshape(-1, 3)
    out[prefix + "ry"] = np.array([o.ry for o in objs], np.float64)
    out[prefix + "alpha"] = np.array([o.alpha for o in objs], np.float64)
    out[prefix + "find_pcl"] = np.array([o.find_pcl for o in objs], np.int32)
    out[prefix + "kpts3d"] = np.array([o.extra_kpts_3D for o in objs], np.float64).reshape(-1, mt.N_EXTRA, 3)


def golden_flipped_targets(cfg):
    from data.datasets.kitti import KITTIDataset
    seed = next(s for s in range(100) if random.Random(s).random() < 0.5)
    sc = mt.scenes()
    with tempfile.TemporaryDirectory() as tmp:
        mt.write_dataset(tmp, sc)
        os.chdir(tmp)                                            # kitti.py opens 'kpts_ann/kpts_ann_train.json' relative to the cwd
        ds = KITTIDataset(cfg, tmp, is_train=True, transforms=None, augment=True)
        assert len(ds) == len(sc)
        out = {"n_images": np.array(len(ds))}
        for i in range(len(ds)):
            objs = ds.filtrate_objects(ds.get_label_objects(i))             # the UNFLIPPED parse = the input of flip_sample
            out["in%d_image_size" % i] = np.array(sc[i][0])
            out["in%d_P" % i] = np.asarray(ds.get_calibration(i).P, np.float64)
            raw_values(objs, "in%d_" % i, out)
            random.seed(seed)                                    # the reference's own `random.random() < self.p` then flips
            img, target, idx = ds[i]
            P = np.asarray(target.get_field("calib").P, np.float64)
            assert P[0, 3] == -out["in%d_P" % i][0, 3] and P[0, 2] != out["in%d_P" % i][0, 2], "the reference did not flip"
            out["flipP%d" % i] = P
            for name in target.fields():
                if name in ("calib", "ori_img", "img_idx"):
                    continue
                out["out%d_%s" % (i, name)] = np.asarray(target.get_field(name))
            out["out%d_size" % i] = np.array(target.size)
        os.chdir(HERE)
    path = os.path.join(HERE, "target_encoding_flipped.npz")
    np.savez_compressed(path, **out)
    print("wrote target_encoding_flipped.npz %.1f KB; objects kept per image:" % (os.path.getsize(path) / 1024),
          [int(out["out%d_reg_mask" % i].sum()) for i in range(len(sc))], "truncated:", [int(out["out%d_trunc_mask" % i].sum()) for i in range(len(sc))])


def golden_kitti_files(cfg):
    from data.datasets.kitti import KITTIDataset
    from data.datasets.kitti_utils import Calibration, read_label
    sc = mt.scenes()
    extra = mt.scenes()[0]                                       # objects drawn like scene 0's, retyped: nothing passes the class filter
    van, dontcare = extra[2][4], extra[2][5]
    assert van["type"] == "Van" and dontcare["type"] == "DontCare"
    sc.append(((1238, 374), mt.P2_B, [van, dontcare]))
    dst = os.path.join(HERE, "kitti_files")
    with tempfile.TemporaryDirectory() as tmp:
        mt.write_dataset(tmp, sc)
        os.chdir(tmp)
        ds = KITTIDataset(cfg, tmp, is_train=True, transforms=None, augment=False)
        out = {"n_images": np.array(len(sc)), "kept": np.array([f[:-4] for f in ds.image_files]),
               "image_sizes": np.array([s[0] for s in sc])}
        for i in range(len(sc)):
            name = "%06d" % i
            objs = ds.filtrate_objects(read_label(os.path.join(tmp, "label_2", name + ".txt"), ds.kpts_ann[str(i)], mt.N_EXTRA))
            out["in%d_P" % i] = np.asarray(Calibration(os.path.join(tmp, "calib", name + ".txt")).P, np.float64)
            raw_values(objs, "in%d_" % i, out)
            out["in%d_type" % i] = np.array([o.type for o in objs])
        os.chdir(HERE)
        if os.path.isdir(dst):
            shutil.rmtree(dst)
        for d in ("label_2", "calib", "ImageSets", "kpts_ann"):
            shutil.copytree(os.path.join(tmp, d), os.path.join(dst, d))
    path = os.path.join(dst, "kitti_files.npz")
    np.savez_compressed(path, **out)
    print("wrote kitti_files/ (%d images, the reference keeps %s for training), kitti_files.npz %.1f KB"
          % (len(sc), list(out["kept"]), os.path.getsize(path) / 1024))


def main():
    mg.install_stubs()
    install_torchvision_functional()
    for name in ("matplotlib", "matplotlib.pyplot"):            # imported at module level by kitti.py, unused on this path
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    np.bool, np.int, np.bool8, np.float = bool, int, np.bool_, float        # aliases numpy 2 removed (kitti.py:367,386,505)
    sys.path.insert(0, mg.REF)
    cfg = mg.ref_cfg()
    golden_images()
    golden_flipped_targets(cfg)
    golden_kitti_files(cfg)


if __name__ == "__main__":
    main()
