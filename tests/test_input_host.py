"""Host half of the device input pipeline, without a GPU: the label flip (dcd_amd/data/augment.py), the formula of the image
kernel as a torch restatement, the KITTI directory reader (dcd_amd/data/kitti_files.py) and the flip-flag draw, each against
fixtures the REFERENCE's own code produced (tests/golden/make_golden_input.py)."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle_targets as OT  # noqa: E402
from oracle import target_oracle as TO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RAW_KEYS = ("image_size", "P", "trunc_occ", "box2d", "hwl", "t", "ry", "alpha", "find_pcl", "kpts3d")


def load_flipped():
    return np.load(os.path.join(GOLDEN, "target_encoding_flipped.npz"))


def raw_inputs(g, i):
    return {k: g["in%d_%s" % (i, k)] for k in RAW_KEYS}


def restate_images(frames, flips, in_h, in_w, mean, std, to_bgr):
    """The formula of `dcd_preprocess_images` (include/dcd_hip.h) in torch, on the CPU: table look-up of the source byte, border
    from byte 0, the table row of the SOURCE channel under TO_BGR.  Pinned bit for bit by tests/golden/input_images.npz below,
    which lets the GPU tests use it at sizes the fixture cannot afford to store."""
    from dcd_amd.data.input_pipeline import normalisation_table
    table = normalisation_table(mean, std)
    out = torch.empty((len(frames), 3, in_h, in_w), dtype=torch.float32)
    for b, (f, flip) in enumerate(zip(frames, flips)):
        f = torch.as_tensor(np.asarray(f))
        h, w = f.shape[:2]
        pad_x, pad_y = (in_w - w) // 2, (in_h - h) // 2
        canvas = torch.zeros((in_h, in_w, 3), dtype=torch.uint8)
        canvas[pad_y:pad_y + h, pad_x:pad_x + w] = f.flip(1) if flip else f
        for c in range(3):
            k = 2 - c if to_bgr else c
            out[b, c] = table[k][canvas[:, :, k].long()]
    return out


def test_flip_sample_matches_reference_fixture():
    """1. `flip_sample` -> oracle.target_oracle.encode_image equals what the reference's `KITTIDataset(augment=True)[i]` made of
    the same scenes with its flip drawn: every ParamsList field, integers exact, floats 1e-7 of the field's range."""
    from dcd_amd.data.augment import flip_sample
    g = load_flipped()
    assert int(g["n_images"]) == 3
    kept = trunc = 0
    for i in range(3):
        raw = raw_inputs(g, i)
        assert raw["box2d"].dtype == np.float64
        flipped = flip_sample(raw)
        np.testing.assert_array_equal(flipped["P"], g["flipP%d" % i])
        np.testing.assert_array_equal(flipped["kpts3d"], raw["kpts3d"])       # the reference does not mirror the key points
        got = TO.encode_image(**flipped)
        OT.compare(got, g, i, 1e-7)
        kept += int(got["reg_mask"].sum())
        trunc += int(got["trunc_mask"].sum())
    assert kept >= 12 and trunc >= 3


def test_flip_sample_differs_from_the_unflipped_targets():
    """The flipped fixture is not the unflipped one: the comparison above cannot pass by ignoring the flip."""
    g = load_flipped()
    with pytest.raises(AssertionError):
        OT.compare(TO.encode_image(**raw_inputs(g, 0)), g, 0, 1e-7)


def test_flip_sample_twice_is_the_identity():
    """Box (as the float32 `box2d` the encoder consumes; the float64 values carry the last-bit rounding of `img_w - x - 1`), `t`
    and `P` come back exactly, `ry` / `alpha` to 1e-12."""
    from dcd_amd.data.augment import flip_sample
    g = load_flipped()
    for i in range(3):
        raw = raw_inputs(g, i)
        keep = {k: np.array(v, copy=True) for k, v in raw.items()}
        once = flip_sample(raw)
        twice = flip_sample(once)
        for k in RAW_KEYS:                                                    # a pure function: the input is left alone
            np.testing.assert_array_equal(raw[k], keep[k])
        assert not np.array_equal(once["t"], raw["t"])
        np.testing.assert_array_equal(np.asarray(twice["box2d"], np.float32), np.asarray(raw["box2d"], np.float32))
        np.testing.assert_array_equal(twice["t"], raw["t"])
        np.testing.assert_array_equal(twice["P"], raw["P"])
        assert np.abs(twice["ry"] - raw["ry"]).max() <= 1e-12
        assert np.abs(twice["alpha"] - raw["alpha"]).max() <= 1e-12


def test_image_formula_restatement_is_bit_equal_to_reference():
    """2. All four frames x flip x TO_BGR: the restatement above against the reference's flip / pad_image / build_transforms."""
    from dcd_amd.config import get_cfg
    g = np.load(os.path.join(GOLDEN, "input_images.npz"))
    in_w, in_h = (int(v) for v in g["input_size"])
    cfg = get_cfg()
    frames = [g["frame%d" % i] for i in range(4)]
    assert [f.shape[:2] for f in frames] == [(25, 77), (26, 58), (32, 96), (32, 95)]
    seen = set()
    for bgr in (0, 1):
        for flip in (0, 1):
            got = restate_images(frames, [flip] * 4, in_h, in_w, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, bool(bgr))
            for i in range(4):
                ref = torch.from_numpy(g["out%d_flip%d_bgr%d" % (i, flip, bgr)])
                assert torch.equal(got[i], ref), (i, flip, bgr)
                seen.add((i, flip, bgr))
    assert len(seen) == 16
    for c in range(3):                                                        # the ramp pins every one of the 768 table entries
        assert len(np.unique(frames[2][:, :, c])) == 256


def write_kitti_dir(tmp_path, sizes, noise_seed=None):
    """The committed label / calib / image-set / annotation texts plus image_2/*.png written here; returns (root, frames)."""
    from PIL import Image
    root = str(tmp_path / "kitti")
    shutil.copytree(os.path.join(GOLDEN, "kitti_files"), root)
    os.makedirs(os.path.join(root, "image_2"))
    rng = np.random.RandomState(noise_seed if noise_seed is not None else 0)
    frames = []
    for i, (w, h) in enumerate(sizes):
        f = rng.randint(0, 256, (h, w, 3)).astype(np.uint8) if noise_seed is not None else np.zeros((h, w, 3), np.uint8)
        Image.fromarray(f, mode="RGB").save(os.path.join(root, "image_2", "%06d.png" % i))
        frames.append(f)
    return root, frames


def test_kitti_files_matches_reference_parse(tmp_path):
    """3. `KittiFiles` over the committed directory equals the reference's own parse field by field, exactly."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles, TYPE_ID_CONVERSION
    g = np.load(os.path.join(GOLDEN, "kitti_files", "kitti_files.npz"))
    sizes = [tuple(int(v) for v in s) for s in g["image_sizes"]]
    root, frames = write_kitti_dir(tmp_path, sizes, noise_seed=5)
    cfg = get_cfg()
    train = KittiFiles(root, "train", cfg, is_train=True)
    assert [train.img_id(i) for i in range(len(train))] == [str(v) for v in g["kept"]] == ["000000", "000001", "000002"]
    ev = KittiFiles(root, "train", cfg, is_train=False)
    assert len(ev) == int(g["n_images"]) == 4
    total = 0
    for i in range(len(ev)):
        s = ev.sample(i)
        assert ev.img_id(i) == "%06d" % i
        assert tuple(s["image_size"]) == sizes[i]
        n = int(g["in%d_n" % i])
        assert len(s["ry"]) == n
        total += n
        for k in RAW_KEYS[1:]:
            ref = g["in%d_%s" % (i, k)]
            assert s[k].shape == ref.shape and s[k].dtype == ref.dtype, (i, k, s[k].shape, s[k].dtype, ref.shape, ref.dtype)
            np.testing.assert_array_equal(s[k], ref, err_msg="image %d field %s" % (i, k))
        assert [TYPE_ID_CONVERSION[str(t)] for t in g["in%d_type" % i]] == list(s["cls"])
        np.testing.assert_array_equal(ev.frame(i), frames[i])
    assert int(g["in3_n"]) == 0 and total == 15                               # scene 3: nothing passes the class filter
    for i in range(len(train)):                                               # the training list indexes the same records
        np.testing.assert_array_equal(train.sample(i)["box2d"], g["in%d_box2d" % i])


def test_flip_flag_draw():
    """4. Seeded draws repeat; evaluation never flips; a second AUG_PARAMS entry (RandomResize) is refused."""
    from dcd_amd import _lib
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    cfg = get_cfg()
    dev = torch.device("cuda:0")                                              # constructing touches no GPU
    a = DeviceInputPipeline(cfg, dev, is_train=True, seed=0).draw_flips(64)
    b = DeviceInputPipeline(cfg, dev, is_train=True, seed=0).draw_flips(64)
    assert a == b and 16 < sum(a) < 48 and all(isinstance(v, bool) for v in a)
    assert DeviceInputPipeline(cfg, dev, is_train=True, seed=1).draw_flips(64) != a
    assert DeviceInputPipeline(cfg, dev, is_train=False, seed=0).draw_flips(64) == [False] * 64
    two = get_cfg(opts=["INPUT.AUG_PARAMS", [[0.5], [-1, [[1280, 384]]]]])
    with pytest.raises(NotImplementedError):
        DeviceInputPipeline(two, dev)
    with pytest.raises(_lib.DcdHipError):
        DeviceInputPipeline(cfg, torch.device("cpu"))
