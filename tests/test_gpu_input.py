"""GPU half of the device input pipeline: `dcd_preprocess_images` (csrc/images.hip) through the C ABI against the fixture the
REFERENCE's flip / pad_image / build_transforms produced and, at the sizes users run, against the torch restatement that
tests/test_input_host.py pins to that fixture bit for bit; `DeviceInputPipeline` end to end, on a side stream, and from a
KITTI directory into one training step.

Images are compared with `torch.equal`: every output value is one of 768 table entries, so bit equality is derived, not
measured.  Targets are compared at the bars of `test_target_encoding_matches_reference_fixture` (integers exact, floats 1e-6
of the field's range)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_input_host as IH  # noqa: E402
import test_oracle_targets as OT  # noqa: E402

KITTI_SIZES = ((1242, 375), (1224, 370), (1238, 374), (1280, 384))        # (w, h)


def run_kernel(cuda, frames, flips, in_h, in_w, mean, std, to_bgr, row_slack=0, gap=0):
    """`dcd_preprocess_images` on frames laid out by THIS helper (not by the pipeline): image i starts `gap` bytes after the end
    of image i - 1 and its rows are 3 w + row_slack bytes apart, so odd offsets and pitches are exercised; the slack bytes hold
    255 (they must never show).  The output starts as NaN: the kernel has to overwrite all of it."""
    from dcd_amd import _lib
    from dcd_amd.data.input_pipeline import normalisation_table
    rec, pos = [], gap
    for f, flip in zip(frames, flips):
        h, w = f.shape[:2]
        rec.append((pos, 3 * w + row_slack, h, w, int(flip)))
        pos += h * (3 * w + row_slack) + gap
    host = np.full(pos, 255, np.uint8)
    for f, (off, pitch, h, w, _) in zip(frames, rec):
        rows = np.lib.stride_tricks.as_strided(host[off:], shape=(h, 3 * w), strides=(pitch, 1))
        rows[:] = f.reshape(h, 3 * w)
    src = torch.from_numpy(host).to(cuda)
    images = torch.tensor(rec, dtype=torch.int64).to(cuda)
    table = normalisation_table(mean, std).to(cuda)
    out = torch.full((len(frames), 3, in_h, in_w), float("nan"), dtype=torch.float32, device=cuda)
    _lib.check(_lib.lib().dcd_preprocess_images(_lib.stream_of(out), src.data_ptr(), src.numel(), images.data_ptr(), table.data_ptr(),
                                                len(frames), in_h, in_w, int(to_bgr), out.data_ptr()), "dcd_preprocess_images")
    return out.cpu()


def noise_frames(sizes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in sizes]


def test_preprocess_images_matches_reference_fixture(cuda):
    """5. All four fixture frames x flip x TO_BGR in batches of four, two source layouts: `torch.equal` to the reference."""
    from dcd_amd.config import get_cfg
    cfg = get_cfg()
    g = np.load(os.path.join(IH.GOLDEN, "input_images.npz"))
    in_w, in_h = (int(v) for v in g["input_size"])
    frames = [g["frame%d" % i] for i in range(4)]
    for row_slack, gap in ((0, 0), (5, 3)):
        for bgr in (0, 1):
            for flips in ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 0, 1)):
                got = run_kernel(cuda, frames, flips, in_h, in_w, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, bgr, row_slack, gap)
                for i in range(4):
                    ref = torch.from_numpy(g["out%d_flip%d_bgr%d" % (i, flips[i], bgr)])
                    assert torch.equal(got[i], ref), (row_slack, gap, bgr, flips, i)


@pytest.mark.parametrize("in_w,sizes", [(1280, KITTI_SIZES), (1278, KITTI_SIZES[:3])], ids=["vector-1280", "scalar-1278"])
def test_preprocess_images_at_kitti_size(cuda, in_w, sizes):
    """6. Eight frames of mixed KITTI sizes, flags [1,0,1,0,0,1,1,0], both TO_BGR settings, against the pinned restatement; the
    1278-wide canvas takes the scalar-store path."""
    from dcd_amd.config import get_cfg
    cfg = get_cfg()
    in_h = 384
    flips = [1, 0, 1, 0, 0, 1, 1, 0]
    frames = noise_frames([sizes[i % len(sizes)] for i in range(8)], seed=21)
    assert len({f.shape for f in frames}) == len(sizes)
    for bgr, (row_slack, gap) in ((0, (0, 0)), (1, (1, 7))):
        got = run_kernel(cuda, frames, flips, in_h, in_w, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, bgr, row_slack, gap)
        ref = IH.restate_images(frames, flips, in_h, in_w, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, bool(bgr))
        assert torch.equal(got, ref), (in_w, bgr)


def test_preprocess_images_rejects_bad_arguments_and_ignores_bad_records(cuda):
    """Status codes, and the promise of the header that a record outside the source buffer reads nothing (all border)."""
    from dcd_amd import _lib
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import normalisation_table
    cfg = get_cfg()
    L = _lib.lib()
    table = normalisation_table(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD)
    src = torch.full((4 * 8 * 3,), 200, dtype=torch.uint8, device=cuda)
    rec = torch.tensor([[0, 24, 4, 8, 0], [48, 24, 4, 8, 0], [0, 24, 40, 8, 0], [-1, 24, 4, 8, 0]], dtype=torch.int64, device=cuda)
    out = torch.full((4, 3, 8, 12), float("nan"), device=cuda)
    tb = table.to(cuda)
    s = _lib.stream_of(out)
    assert L.dcd_preprocess_images(s, src.data_ptr(), src.numel(), rec.data_ptr(), tb.data_ptr(), 4, 8, 12, 0, out.data_ptr()) == 0
    border = table[:, 0].reshape(3, 1, 1).expand(3, 8, 12)
    got = out.cpu()
    assert torch.equal(got[0, :, 2:6, 2:10], table[:, 200].reshape(3, 1, 1).expand(3, 4, 8))
    for b in (1, 2, 3):                                   # runs past the end / taller than the canvas / negative offset
        assert torch.equal(got[b], border), b
    assert L.dcd_preprocess_images(s, None, src.numel(), rec.data_ptr(), tb.data_ptr(), 4, 8, 12, 0, out.data_ptr()) == 1
    assert L.dcd_preprocess_images(s, src.data_ptr(), 0, rec.data_ptr(), tb.data_ptr(), 4, 8, 12, 0, out.data_ptr()) == 1
    assert L.dcd_preprocess_images(s, src.data_ptr(), src.numel(), rec.data_ptr(), tb.data_ptr(), 0, 8, 12, 0, out.data_ptr()) == 1
    assert L.dcd_preprocess_images(s, src.data_ptr(), src.numel(), rec.data_ptr(), tb.data_ptr(), 4, 8, 0, 0, out.data_ptr()) == 1


def fixture_samples():
    g = IH.load_flipped()
    return g, OT.load(), [IH.raw_inputs(g, i) for i in range(int(g["n_images"]))]


def tensor_fields(t):
    return {name: t.get_field(name).cpu().numpy() for name in t.fields() if torch.is_tensor(t.get_field(name))}


def test_pipeline_targets_and_images_follow_the_flags(cuda):
    """7. A mixed flag vector: flipped images' targets equal target_encoding_flipped.npz, the others target_encoding.npz;
    `Calib_P` and `calib` carry the flipped matrix; the images equal the restatement."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    gf, gu, samples = fixture_samples()
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(cuda)])
    frames = noise_frames([tuple(int(v) for v in s["image_size"]) for s in samples], seed=3)
    pipe = DeviceInputPipeline(cfg, cuda, is_train=True, seed=0)
    for flags in ([True, False, True], [False, True, False]):
        images, targets = pipe(frames, samples, img_ids=["a", "b", "c"], flip=flags)
        assert pipe.last_flip == flags and len(targets) == 3
        assert images.shape == (3, 3, 384, 1280) and images.dtype == torch.float32 and images.device == cuda
        ref = IH.restate_images(frames, flags, 384, 1280, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR)
        assert torch.equal(images.cpu(), ref)
        for i, (t, f) in enumerate(zip(targets, flags)):
            got = tensor_fields(t)
            OT.compare(got, gf if f else gu, i, 1e-6)
            P = gf["flipP%d" % i] if f else gf["in%d_P" % i]
            np.testing.assert_array_equal(t.get_field("calib").P, P)
            kept = got["reg_mask"].astype(bool)
            assert kept.any()
            np.testing.assert_array_equal(got["Calib_P"][kept], np.broadcast_to(P.astype(np.float32), (int(kept.sum()), 3, 4)))
            assert t.get_field("img_idx") == "abc"[i]
    # the draw: the object's own generator, reproducible
    _, _ = pipe(frames, samples)
    again = DeviceInputPipeline(cfg, cuda, is_train=True, seed=0)
    again(frames, samples)
    assert again.last_flip == DeviceInputPipeline(cfg, cuda, is_train=True, seed=0).draw_flips(3)
    ev = DeviceInputPipeline(cfg, cuda, is_train=False, seed=0)
    ev(frames, samples)
    assert ev.last_flip == [False] * 3


def test_pipeline_refuses_what_it_cannot_do(cuda):
    from dcd_amd import _lib
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    _, _, samples = fixture_samples()
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False])
    pipe = DeviceInputPipeline(cfg, cuda)
    frames = noise_frames([tuple(int(v) for v in s["image_size"]) for s in samples], seed=3)
    with pytest.raises(ValueError):                       # larger than the canvas: the multi-scale branch is not built
        big = dict(samples[0], image_size=np.array([1300, 375]))
        pipe([np.zeros((375, 1300, 3), np.uint8)], [big])
    with pytest.raises(ValueError):                       # image_size disagrees with the frame
        pipe([frames[1]], [samples[0]])
    with pytest.raises(ValueError):
        pipe([frames[0].astype(np.float32)], [samples[0]])
    with pytest.raises(_lib.DcdHipError):
        DeviceInputPipeline(cfg, "cpu")


def test_pipeline_on_a_side_stream(cuda):
    """8. Four consecutive different batches through ONE pipeline on a second stream (two pinned slots, so slots are reused),
    consumed on the current stream after `wait_stream`, against the same batches each through a fresh pipeline on the current
    stream."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    _, _, samples = fixture_samples()
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False])
    sizes = [tuple(int(v) for v in s["image_size"]) for s in samples]
    batches = []
    for k in range(4):
        order = [(k + j) % 3 for j in range(8)]
        flags = [bool((k + j * j) % 2) for j in range(8)]
        batches.append((noise_frames([sizes[i] for i in order], seed=100 + k), [samples[i] for i in order], flags))
    pipe = DeviceInputPipeline(cfg, cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    outs = [pipe(f, s, flip=fl, stream=side) for f, s, fl in batches]
    torch.cuda.current_stream(cuda).wait_stream(side)
    sums = [o[0].double().sum() for o in outs]             # consumed on the current stream
    for k, (f, s, fl) in enumerate(batches):
        images, targets = DeviceInputPipeline(cfg, cuda)(f, s, flip=fl)
        assert torch.equal(outs[k][0], images), k
        assert float(sums[k]) == float(images.double().sum())
        for a, b in zip(outs[k][1], targets):
            fa, fb = tensor_fields(a), tensor_fields(b)
            assert set(fa) == set(fb)
            for name in fa:
                np.testing.assert_array_equal(fa[name], fb[name], err_msg="batch %d field %s" % (k, name))
    assert not torch.equal(outs[0][0], outs[2][0])         # the batches that shared a slot do differ


def test_one_training_step_from_files(cuda, tmp_path):
    """9. KittiFiles over the fixture directory with seeded-noise PNGs -> pipeline -> `train_step` at the default 384 x 1280
    input: finite losses; the step's inputs are bit-equal to the restatement's images and to `encode_targets` on
    `flip_sample`'d samples."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.augment import flip_sample
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.target_encoder import encode_targets
    from dcd_amd.engine.trainer import build_optimizer, init_like_trained, train_step
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path, [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False])
    files = KittiFiles(root, cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    assert len(files) == 3
    frames = [files.frame(i) for i in range(3)]
    samples = [files.sample(i) for i in range(3)]
    ids = [files.img_id(i) for i in range(3)]
    flags = [True, False, True]
    pipe = DeviceInputPipeline(cfg, cuda, is_train=True, seed=0)
    images, targets = pipe(frames, samples, img_ids=ids, flip=flags)
    ref_images = IH.restate_images(frames, flags, 384, 1280, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR)
    assert torch.equal(images.cpu(), ref_images)
    ref_targets = encode_targets([flip_sample(s) if f else s for s, f in zip(samples, flags)], cfg, cuda, ids)
    for a, b in zip(targets, ref_targets):
        fa, fb = tensor_fields(a), tensor_fields(b)
        assert set(fa) == set(fb) and a.get_field("img_idx") == b.get_field("img_idx")
        for name in fa:
            np.testing.assert_array_equal(fa[name], fb[name], err_msg=name)
        np.testing.assert_array_equal(a.get_field("calib").P, b.get_field("calib").P)
    assert sum(int(t.get_field("reg_mask").sum()) for t in targets) >= 12
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda).train()
    init_like_trained(model)
    opt = build_optimizer(model, cfg)
    loss_dict, _ = train_step(model, opt, images, targets)
    vals = {k: float(v.detach()) for k, v in loss_dict.items()}
    assert vals and all(np.isfinite(v) for v in vals.values()), vals
