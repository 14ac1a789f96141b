"""Right-camera views and the unlabelled `test` split, without a GPU: `KittiFiles` (dcd_amd/data/kitti_files.py) and the float32
branch of `flip_sample` (dcd_amd/data/augment.py) over tests/golden/kitti_right/ against what the REFERENCE's own `KITTIDataset`
held for the same files under DATASETS.USE_RIGHT_IMAGE (tests/golden/make_golden_right.py -> right_views.npz), and the host half of
`engine.inference.inference` on a split without labels, driven by a stub pass.

Boxes of right views are float32 and compared bit for bit; every other raw value is compared exactly, as
tests/test_input_host.py compares the left view; encoded targets at its 1e-7 of the field's range."""
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_input_host as IH  # noqa: E402
import test_oracle_targets as OT  # noqa: E402
from oracle import target_oracle as TO  # noqa: E402

RIGHT_ROOT = os.path.join(IH.GOLDEN, "kitti_right")
RAW_KEYS = IH.RAW_KEYS


def load_right():
    return np.load(os.path.join(IH.GOLDEN, "right_views.npz"))


class Fields:
    """The keys `<prefix><i>_<name>` of the fixture under the names `out<i>_<name>`, which is what `OT.compare` reads."""

    def __init__(self, g, prefix):
        self.g, self.prefix = g, prefix
        self.files = ["out" + k[len(prefix):] for k in g.files if k.startswith(prefix) and k[len(prefix)].isdigit()]

    def __getitem__(self, key):
        return self.g[self.prefix + key[len("out"):]]


def right_cfg(*opts):
    from dcd_amd.config import get_cfg
    return get_cfg(opts=["DATASETS.USE_RIGHT_IMAGE", True] + list(opts))


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def check_raw(s, g, prefix, right, what):
    """One sample against the fixture's raw values `<prefix>*`: the box in the reference's own dtype, the rest exactly."""
    n = int(g[prefix + "n"])
    assert len(s["ry"]) == n, what
    for k in RAW_KEYS[2:]:
        if k == "box2d":
            continue
        ref = g[prefix + k]
        assert s[k].shape == ref.shape and s[k].dtype == ref.dtype, (what, k, s[k].shape, s[k].dtype, ref.shape, ref.dtype)
        np.testing.assert_array_equal(s[k], ref, err_msg="%s field %s" % (what, k))
    xyxy, box32 = g[prefix + "xyxy"], g[prefix + "box2d"]
    assert s["box2d"].shape == (n, 4) and s["box2d"].dtype == xyxy.dtype == (np.float32 if right else np.float64), what
    if right:
        np.testing.assert_array_equal(bits(s["box2d"]), bits(xyxy), err_msg=what)
    else:
        np.testing.assert_array_equal(s["box2d"], xyxy, err_msg=what)
    np.testing.assert_array_equal(bits(np.asarray(s["box2d"], np.float32)), bits(box32), err_msg=what)      # what the encoder packs


def test_lengths_ids_and_raw_values_of_both_views():
    """1. len = 2 N, the right half repeats the ids of the left, `image_3` / `P3` / the projected float32 boxes, and targets
    encoded from them (oracle/target_oracle.py) equal the reference's `ParamsList` of every view."""
    from dcd_amd.data.kitti_files import KittiFiles, read_p, read_p2
    from PIL import Image
    g = load_right()
    assert np.lib.NumpyVersion(str(g["numpy_version"])) >= "2.0.0"             # the flip of float32 boxes below is NumPy 2's
    N, V = int(g["n_images"]), int(g["n_views"])
    files = KittiFiles(RIGHT_ROOT, "train", right_cfg(), is_train=True)
    assert len(files) == V == 2 * N == 6 and files.has_labels is True
    in_w, in_h = (int(v) for v in g["input_size"])
    kept = trunc = 0
    for i in range(V):
        right = bool(g["in%d_is_right" % i])
        assert right == (i >= N) == files.is_right(i)
        assert files.img_id(i) == str(g["in%d_id" % i]) == files.img_id(i % N)
        s = files.sample(i)
        folder = "image_3" if right else "image_2"
        with Image.open(os.path.join(RIGHT_ROOT, folder, files.img_id(i) + ".png")) as im:
            assert tuple(s["image_size"]) == im.size == tuple(int(v) for v in g["in%d_image_size" % i])
            np.testing.assert_array_equal(files.frame(i), np.array(im.convert("RGB")))
        np.testing.assert_array_equal(s["P"], g["in%d_P" % i])
        calib = os.path.join(RIGHT_ROOT, "calib", files.img_id(i) + ".txt")
        np.testing.assert_array_equal(s["P"], read_p(calib, "P3" if right else "P2"))
        np.testing.assert_array_equal(read_p2(calib), read_p(calib, "P2"))
        assert ("box2d_float32" in s) == right
        check_raw(s, g, "in%d_" % i, right, "view %d" % i)
        assert [str(t) for t in g["in%d_type" % i]] == ["Car"] * len(s["cls"]) and list(s["cls"]) == [0] * len(s["cls"])
        got = TO.encode_image(**{k: s[k] for k in RAW_KEYS}, input_size=(in_w, in_h))
        OT.compare(got, Fields(g, "out"), i, 1e-7)
        kept += int(got["reg_mask"].sum())
        trunc += int(got["trunc_mask"].sum())
    assert not np.array_equal(files.frame(0), files.frame(N))                  # the two cameras' files do differ
    assert not np.array_equal(g["in0_P"], g["in%d_P" % N])
    assert abs(g["in%d_P" % N][0, 3] / g["in%d_P" % N][0, 0] + 0.47) < 0.01 and abs(g["in0_P"][0, 3] / g["in0_P"][0, 0] - 0.06) < 0.01
    assert kept >= 12 and trunc >= 1
    with pytest.raises(IndexError):
        files.sample(V)
    with pytest.raises(IndexError):
        files.img_id(V)


def test_fixture_hits_every_clipping_case():
    """2. On the fixture itself: among the right-view boxes one lies strictly inside the image, one is cut by max(., 0) and one by
    min(., w - 1) or min(., h - 1); a class outside DETECT_CLASSES was written; and the unclipped projection really lay outside."""
    from dcd_amd.data.kitti_files import corners_3d
    g = load_right()
    N = int(g["n_images"])
    inside = low = high = 0
    for i in range(N, 2 * N):
        w, h = (int(v) for v in g["in%d_image_size" % i])
        for o, box in enumerate(g["in%d_box2d" % i]):
            c = corners_3d(g["in%d_hwl" % i][o], float(g["in%d_ry" % i][o]), g["in%d_t" % i][o])
            assert (c[:, 2] > 0).all()                                         # nothing behind the camera in this fixture
            uv = np.hstack((c, np.ones((8, 1)))) @ g["in%d_P" % i].T
            u, v = uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2]
            cut_low = (box[0] == 0 and u.min() < 0) or (box[1] == 0 and v.min() < 0)
            cut_high = (box[2] == w - 1 and u.max() > w - 1) or (box[3] == h - 1 and v.max() > h - 1)
            low, high = low + bool(cut_low), high + bool(cut_high)
            inside += bool(box[0] > 0 and box[1] > 0 and box[2] < w - 1 and box[3] < h - 1)
    assert inside >= 1 and low >= 1 and high >= 1, (inside, low, high)
    types_written = set()
    for name in os.listdir(os.path.join(RIGHT_ROOT, "label_2")):
        with open(os.path.join(RIGHT_ROOT, "label_2", name)) as f:
            types_written |= {line.split(" ")[0] for line in f if line.strip()}
    from dcd_amd.config import get_cfg
    assert types_written - set(get_cfg().DATASETS.DETECT_CLASSES)


def float64_flip_box(box, img_w):
    """The rule `flip_sample` has applied to every box so far, written out: float64 from the values given."""
    box = np.array(box, dtype=np.float64).reshape(-1, 4)
    w = box[:, 2] - box[:, 0]
    box[:, 0] = img_w - box[:, 2] - 1
    box[:, 2] = box[:, 0] + w
    return box


def test_flip_of_both_views_and_of_the_existing_inputs():
    """3. `flip_sample` of every view equals the raw values the reference held after its own flip: float32 boxes of right views bit
    for bit (float32 arithmetic, NumPy >= 2), float64 boxes of left views exactly; `P`, `t`, `ry`, `alpha` exactly; the targets
    encoded from them equal the reference's flipped `ParamsList`.  The inputs of target_encoding_flipped.npz -- float64 boxes, and
    the same boxes handed in as float32 arrays without the marker -- are still flipped in float64."""
    from dcd_amd.data.augment import flip_sample
    from dcd_amd.data.kitti_files import KittiFiles
    g = load_right()
    N, V = int(g["n_images"]), int(g["n_views"])
    in_w, in_h = (int(v) for v in g["input_size"])
    files = KittiFiles(RIGHT_ROOT, "train", right_cfg(), is_train=True)
    differs = 0
    for i in range(V):
        s = files.sample(i)
        before = {k: np.array(s[k], copy=True) for k in RAW_KEYS}
        f = flip_sample(s)
        for k in RAW_KEYS:                                                      # a pure function: the input is left alone
            np.testing.assert_array_equal(s[k], before[k])
        np.testing.assert_array_equal(f["P"], g["flipP%d" % i])
        check_raw(f, g, "fin%d_" % i, i >= N, "flipped view %d" % i)
        np.testing.assert_array_equal(f["image_size"], s["image_size"])
        got = TO.encode_image(**{k: f[k] for k in RAW_KEYS}, input_size=(in_w, in_h))
        OT.compare(got, Fields(g, "flip"), i, 1e-7)
        if i >= N:                                                              # does the float64 rule land elsewhere?
            differs += int((np.asarray(float64_flip_box(s["box2d"], int(s["image_size"][0])), np.float32) != f["box2d"]).sum())
    print("float32 box values where the float64 rule would have given another float32: %d" % differs)
    assert differs >= 1                                                         # the fixture does tell the two rules apart
    gf = IH.load_flipped()
    for i in range(int(gf["n_images"])):
        raw = IH.raw_inputs(gf, i)
        want = float64_flip_box(raw["box2d"], int(raw["image_size"][0]))
        got = flip_sample(raw)["box2d"]
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
        as32 = dict(raw, box2d=np.asarray(raw["box2d"], np.float32))
        got32 = flip_sample(as32)["box2d"]
        assert got32.dtype == np.float64
        np.testing.assert_array_equal(got32, float64_flip_box(as32["box2d"], int(raw["image_size"][0])))


def test_images_without_kept_objects_leave_before_the_doubling():
    """4. 000002 holds a 'Van' and a 'DontCare' only: it is in neither half of the training list, and in the evaluation list."""
    from dcd_amd.data.kitti_files import KittiFiles
    g = load_right()
    files = KittiFiles(RIGHT_ROOT, "train", right_cfg(), is_train=True)
    ids = [files.img_id(i) for i in range(len(files))]
    kept = [str(v) for v in g["kept"]]
    assert ids == kept + kept == ["000000", "000001", "000003"] * 2 and "000002" not in ids
    ev = KittiFiles(RIGHT_ROOT, "train", right_cfg(), is_train=False)          # USE_RIGHT_IMAGE counts in training only
    assert [ev.img_id(i) for i in range(len(ev))] == ["000000", "000001", "000002", "000003"]
    assert not any(ev.is_right(i) for i in range(len(ev))) and len(ev.sample(2)["ry"]) == 0
    infer = KittiFiles(RIGHT_ROOT, "train", right_cfg("DATASETS.INFER_ON_RIGHT_IMG", True), is_train=False)
    assert len(infer) == 4 and all(infer.is_right(i) for i in range(4))
    N = int(g["n_images"])
    for j, i in enumerate((0, 1, 3)):                                          # every index a right view, the length unchanged
        s = infer.sample(i)
        np.testing.assert_array_equal(s["P"], g["in%d_P" % (N + j)])
        np.testing.assert_array_equal(bits(s["box2d"]), bits(g["in%d_box2d" % (N + j)]))
    train = KittiFiles(RIGHT_ROOT, "train", right_cfg("DATASETS.INFER_ON_RIGHT_IMG", True, "DATASETS.USE_RIGHT_IMAGE", False), is_train=True)
    assert len(train) == 3 and not any(train.is_right(i) for i in range(3))    # INFER_ON_RIGHT_IMG counts in evaluation only


def test_defaults_return_what_they_returned(tmp_path):
    """5. Both switches false on tests/golden/kitti_files/: the values of kitti_files.npz (on purpose the check of
    tests/test_input_host.py once more), float64 boxes, no marker, no right view."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    sizes = [tuple(int(v) for v in s) for s in g["image_sizes"]]
    root, frames = IH.write_kitti_dir(tmp_path, sizes, noise_seed=5)
    cfg = get_cfg()
    assert cfg.DATASETS.USE_RIGHT_IMAGE is False and cfg.DATASETS.INFER_ON_RIGHT_IMG is False
    train = KittiFiles(root, "train", cfg, is_train=True)
    assert [train.img_id(i) for i in range(len(train))] == [str(v) for v in g["kept"]]
    ev = KittiFiles(root, "train", cfg, is_train=False)
    assert len(ev) == int(g["n_images"]) == 4 and ev.has_labels is True
    for i in range(len(ev)):
        s = ev.sample(i)
        assert list(s) == ["image_size", "P", "trunc_occ", "box2d", "hwl", "t", "ry", "alpha", "find_pcl", "kpts3d", "cls"]
        assert not ev.is_right(i) and tuple(s["image_size"]) == sizes[i]
        for k in RAW_KEYS[1:]:
            ref = g["in%d_%s" % (i, k)]
            assert s[k].shape == ref.shape and s[k].dtype == ref.dtype, (i, k)
            np.testing.assert_array_equal(s[k], ref, err_msg="image %d field %s" % (i, k))
        np.testing.assert_array_equal(ev.frame(i), frames[i])


@pytest.fixture()
def unlabelled_root(tmp_path):
    """kitti_right/ without `label_2` and `kpts_ann`: what KITTI's `testing/` holds."""
    root = str(tmp_path / "testing")
    for d in ("ImageSets", "calib", "image_2", "image_3"):
        shutil.copytree(os.path.join(RIGHT_ROOT, d), os.path.join(root, d))
    return root


def test_unlabelled_split(unlabelled_root):
    """6. `test`: no labels, no file under `label_2` / `kpts_ann` opened (the folders are not there), zero-object samples with the
    shapes and dtypes of a labelled sample, `P` as the reference's test-mode target holds it, and no training on it."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    g = load_right()
    cfg = get_cfg()
    files = KittiFiles(unlabelled_root, "test", cfg, is_train=False)
    assert files.has_labels is False and len(files) == int(g["test_n"]) == 4
    labelled = KittiFiles(RIGHT_ROOT, "train", cfg, is_train=False).sample(0)
    for i in range(len(files)):
        assert files.img_id(i) == str(g["test%d_id" % i]) and not files.is_right(i)
        s = files.sample(i)
        assert list(s) == list(labelled)
        np.testing.assert_array_equal(s["P"], g["test%d_P" % i])
        assert tuple(s["image_size"]) == files.frame(i).shape[1::-1]
        for k in RAW_KEYS[2:] + ("cls",):
            assert s[k].dtype == labelled[k].dtype and s[k].shape == (0,) + labelled[k].shape[1:], (i, k, s[k].shape, s[k].dtype)
    right = KittiFiles(unlabelled_root, "test", get_cfg(opts=["DATASETS.INFER_ON_RIGHT_IMG", True]), is_train=False)
    assert right.is_right(0) and right.sample(0)["box2d"].shape == (0, 4) and not np.array_equal(right.frame(0), files.frame(0))
    with pytest.raises(ValueError, match="no labels"):
        KittiFiles(unlabelled_root, "test", cfg, is_train=True)
    with pytest.raises(FileNotFoundError):                                      # a labelled split does need the folders
        KittiFiles(unlabelled_root, "train", cfg, is_train=False)


def test_unlabelled_inference_host_side(unlabelled_root, tmp_path, monkeypatch):
    """7. `inference` on a split without labels with the device pass replaced by a stub that writes each image's file from
    fabricated rows: every id gets its file (an empty one where nothing passes), the result is {}, and neither `read_annos` nor
    `official_eval` runs; `finish_pass` with refined rows leaves one file per id in `kitti_results_for_eval` and returns
    {"gmw": {}}; a pass that skipped an id is an error, not a silent gap."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine import inference as inf
    from dcd_amd.eval import kitti_annos, kitti_ap

    def never(*a, **k):
        raise AssertionError("a split without labels is not read back and not scored")
    monkeypatch.setattr(kitti_annos, "read_annos", never)
    monkeypatch.setattr(kitti_ap, "official_eval", never)
    files = KittiFiles(unlabelled_root, "test", get_cfg(), is_train=False)
    ids = [files.img_id(i) for i in range(len(files))]
    rng = np.random.RandomState(3)
    rows = rng.uniform(1, 50, (4, 5, 14)).astype(np.float32)
    rows[:, :, 0] = 0
    scores = np.sort(rng.uniform(0.3, 0.9, (4, 5)), axis=1)[:, ::-1].astype(np.float32)
    scores[2] = 0.01                                                            # image 2: nothing passes the threshold
    seen = {}

    def stub_pass(model, files_, pipeline, predict_folder, batch_size, workers, want_records, refiner=None):
        seen.update(batch_size=batch_size, want_records=want_records, n=len(files_))
        for b, img_id in enumerate(ids):
            inf.write_image_rows(rows[b], scores[b], 0.2, os.path.join(predict_folder, img_id + ".txt"))
        return {}
    monkeypatch.setattr(inf, "_batched_pass", stub_pass)
    model = torch.nn.Linear(1, 1)
    pipeline = types.SimpleNamespace(is_train=False, device=torch.device("cpu"))
    out = str(tmp_path / "out")
    assert inf.inference(model, files, pipeline, out, batch_size=3) == {}
    assert seen == dict(batch_size=3, want_records=False, n=4) and model.training
    assert sorted(os.listdir(out)) == ["data"]
    assert sorted(os.listdir(os.path.join(out, "data"))) == [i + ".txt" for i in ids]
    texts = [open(os.path.join(out, "data", i + ".txt")).read() for i in ids]
    assert texts[2] == "\n"                                                     # `write_detections`' file without a detection
    assert [len(t.split()) for t in texts] == [5 * 16, 5 * 16, 0, 5 * 16]
    # the refined half: 15 kept rows of images 0, 1 and 3
    kept = np.concatenate([rows[b] for b in (0, 1, 3)])
    host_ids = [ids[b] for b in (0, 1, 3) for _ in range(5)]
    got = inf.finish_pass(files, ids, out, ("R40",), torch.device("cpu"), (kept, host_ids, torch.from_numpy(kept[:, 9:12] + 1)))
    assert got == {"gmw": {}}
    folder = os.path.join(out, "kitti_results_for_eval")
    assert sorted(os.listdir(folder)) == [i + ".txt" for i in ids]
    lines = [len(open(os.path.join(folder, i + ".txt")).read().splitlines()) for i in ids]
    assert lines == [5, 5, 0, 5]
    os.remove(os.path.join(out, "data", ids[1] + ".txt"))
    with pytest.raises(RuntimeError, match="no result file"):
        inf.finish_pass(files, ids, out, ("R40",), torch.device("cpu"))
    # an object without `has_labels` is a labelled split, as before: it is read back
    with pytest.raises(AssertionError, match="not read back"):
        inf.finish_pass(types.SimpleNamespace(root=unlabelled_root, classes=("Car",)), ids, out, ("R40",), torch.device("cpu"))
