"""`dcd_decode_detections` (csrc/decode.hip) on the device: against the reference's `PostProcessor` fixture, against the op-by-op
chain (`PostProcessor.forward` / `forward_batch`, themselves pinned to the reference) with per-image calibration and on candidates
where every clamp and branch occurs, isolation of a broken candidate, run-to-run bits, and the refusals.  Shapes are the
fixtures': 24 x 80 maps, 2 images, K = 50 (16 for the random candidates), 73 key points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import golden_inputs as gi  # noqa: E402
import test_decode_host as DH  # noqa: E402
from test_host_golden import load, small_cfg  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(*tensors):
    return [None if t is None else t.detach().cpu().numpy() for t in tensors]


def _pp(cuda, *opts):
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head.detector_infer import make_post_processor
    return make_post_processor(get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(cuda), "MODEL.USE_SYNC_BN", False,
                                             "INPUT.WIDTH_TRAIN", 320, "INPUT.HEIGHT_TRAIN", 96] + list(opts)))


def _maps(cuda, n=2):
    preds, targets = gi.loss_inputs()
    return ({"cls": torch.from_numpy(preds["cls"][:n]).to(cuda), "reg": torch.from_numpy(preds["reg"][:n]).to(cuda)},
            [t.to(cuda) for t in targets[:n]])


def test_kernel_matches_the_reference_fixture(cuda):
    from dcd_amd import ops
    from dcd_amd.model.head.detector_infer import make_post_processor
    g = load("post_processor")
    pp = make_post_processor(small_cfg(str(cuda)))
    vectors, topk, targets = DH.fixture_candidates(pp, cuda)
    table = pp._image_table(targets, cuda)
    rows, aux, k2, k3 = _np(*ops.decode_detections(vectors, topk, table, pp.decode_spec(), records=True))
    DH.check_against_fixture(rows, aux, k2, k3, g, "device")
    r = g["pred_extra_kpts_2d"]
    assert np.abs(DH.image_kpts_from_normalised(k2, table.cpu().numpy()) - r).max() <= 1e-6 * (np.abs(r).max() + 1e-6)
    # without the record flag: the same rows, no key points
    rows2, aux2, none2, none3 = ops.decode_detections(vectors, topk, table, pp.decode_spec())
    assert none2 is None and none3 is None
    assert np.array_equal(rows2.cpu().numpy(), rows) and np.array_equal(aux2.cpu().numpy(), aux)


def test_threshold_keeps_a_prefix_of_the_fixture_rows(cuda, tmp_path):
    from dcd_amd.engine.inference import keep_prefix, write_image_rows
    g = load("post_processor")
    ref = g["result"]
    scale = np.abs(ref).max(0) + 1e-6
    preds, targets = _maps(cuda, 1)
    pp = _pp(cuda, "TEST.DETECTIONS_THRESHOLD", 0.8)
    rows, aux, recs = pp.decode_fused(preds, targets)
    assert recs is None and rows.shape == (50, 14)
    rows, aux = _np(rows, aux)
    assert (np.diff(aux[:, 0]) <= 0).all()                                       # descending: the kept rows are a prefix
    n = keep_prefix(aux[:, 0], pp.det_threshold)
    assert n == 27 == int((aux[:, 0] >= 0.8).sum())
    assert (np.abs(rows[:n] - ref[:27]) / scale).max() <= 1e-4
    # the same cut as the chain's own threshold
    with torch.no_grad():
        chain = pp(preds, targets)[0].cpu().numpy()
    assert chain.shape == (27, 14) and (np.abs(rows[:n] - chain) / scale).max() <= 1e-4
    path = str(tmp_path / "000000.txt")
    assert write_image_rows(rows, aux[:, 0], pp.det_threshold, path) == 27 and len(open(path).read().splitlines()) == 27
    pp = _pp(cuda, "TEST.DETECTIONS_THRESHOLD", 1.0)
    rows, aux, _ = pp.decode_fused(preds, targets)
    rows, aux = _np(rows, aux)
    assert write_image_rows(rows, aux[:, 0], pp.det_threshold, path) == 0
    assert open(path).read() == "\n"


def _perturb(targets):
    """Intrinsics, padding and image size that differ between the images, as
    test_batched_post_processor_equals_the_image_by_image_decode perturbs them."""
    from dcd_amd.data.calibration import Calibration
    for i, t in enumerate(targets, start=1):
        P = np.array(t.get_field("calib").P, dtype=np.float64).copy()
        s_ = 1.0 + 0.01 * i
        P[0, 0] *= s_; P[1, 1] *= s_; P[0, 2] += i; P[1, 2] -= 0.5 * i  # noqa: E702
        t.add_field("calib", Calibration(P))
        t.add_field("pad_size", t.get_field("pad_size") + (i % 3))
        t.size = (t.size[0] - 2 * (i % 4), t.size[1] - (i % 2))
    return targets


def test_every_image_is_decoded_with_its_own_calibration(cuda):
    from dcd_amd import ops
    from dcd_amd.engine.inference import keep_prefix
    preds, targets = _maps(cuda, 2)
    targets = _perturb(targets)
    pp = _pp(cuda)                                                            # the shipped threshold
    rows, aux, _ = pp.decode_fused(preds, targets)
    rows, aux = _np(rows, aux)
    K = pp.max_detection
    for i in range(2):
        one = {k: v[i:i + 1] for k, v in preds.items()}
        with torch.no_grad():
            ref, info, _ = pp(one, targets[i:i + 1])
        ref, raw = ref.cpu().numpy(), info["vis_scores"].cpu().numpy().reshape(-1)
        block, scores = rows[i * K:(i + 1) * K], aux[i * K:(i + 1) * K, 0]
        n = keep_prefix(scores, pp.det_threshold)
        assert n == len(ref) > 0
        np.testing.assert_array_equal(block[:n, 0], ref[:, 0])
        np.testing.assert_array_equal(scores[:n], raw)
        assert (np.abs(block[:n] - ref) / (np.abs(ref).max(0) + 1e-6)).max() <= 1e-4, i
    # the table is read per image: with its two rows swapped the result changes
    topk = ops.select_topk(preds["cls"], K, fuse_nms=True)
    vectors = ops.select_point_of_interest(2, topk[1], preds["reg"])
    table = pp._image_table(targets, cuda)
    same = ops.decode_detections(vectors, topk, table, pp.decode_spec())[0].cpu().numpy()
    swapped = ops.decode_detections(vectors, topk, table.flip(0).contiguous(), pp.decode_spec())[0].cpu().numpy()
    assert np.array_equal(same, rows)
    assert not np.array_equal(swapped[:K], rows[:K]) and not np.array_equal(swapped[K:], rows[K:])


def test_candidates_where_every_clamp_and_branch_occurs(cuda):
    """Seeded random head outputs handed over as `vectors` (K = 16, B = 2; sigmas and seed found on the CPU, see
    test_decode_host.BRANCH_SIGMA); the conditions are asserted on the chain's output, then the rows are compared with it."""
    from dcd_amd import ops
    pp = DH.branch_post_processor(cuda)
    vectors, topk, targets = DH.branch_inputs(pp, cuda)
    ref, info, vis = DH.chain_on_candidates(pp, vectors, topk, targets)
    DH.assert_every_branch_occurs(pp, vectors, targets, ref, info)
    rows, aux, _, _ = _np(*ops.decode_detections(vectors, topk, pp._image_table(targets, cuda), pp.decode_spec()))
    DH.compare_with_chain(rows, aux, ref, info, vis)


def test_a_broken_candidate_touches_nobody_else_and_runs_are_bit_equal(cuda):
    from dcd_amd import ops
    pp = DH.branch_post_processor(cuda)
    vectors, topk, targets = DH.branch_inputs(pp, cuda)
    table, spec = pp._image_table(targets, cuda), pp.decode_spec()
    clean = _np(*ops.decode_detections(vectors, topk, table, spec, records=True))
    again = _np(*ops.decode_detections(vectors, topk, table, spec, records=True))
    for a, b in zip(clean, again):                                            # determinism: the same bits
        assert np.array_equal(a, b, equal_nan=True)
    broken = vectors.clone()
    huge, nan = 5, DH.BRANCH_K + 3                                            # one candidate in each image
    broken[0, 5] = 1e30
    broken[1, 3] = float("nan")
    out = _np(*ops.decode_detections(broken, topk, table, spec, records=True))   # (no error status: the call returns)
    others = np.ones(DH.BRANCH_B * DH.BRANCH_K, bool)
    others[[huge, nan]] = False
    for a, b in zip(clean, out):
        assert np.array_equal(a[others], b[others], equal_nan=True)
    assert not np.array_equal(clean[0][huge], out[0][huge], equal_nan=True)
    torch.cuda.synchronize()


def test_refused_configurations(cuda, tmp_path):
    from dcd_amd import _lib, ops
    pp = DH.branch_post_processor(cuda)
    vectors, topk, targets = DH.branch_inputs(pp, cuda)
    table, spec = pp._image_table(targets, cuda), pp.decode_spec()
    # K = 129 and nk = 129: the error status, nothing launched (the outputs keep their sentinel)
    L = _lib.lib()
    rows = torch.full((DH.BRANCH_B * DH.BRANCH_K, 14), -7.0, device=cuda)
    aux = torch.full((DH.BRANCH_B * DH.BRANCH_K, 4), -7.0, device=cuda)
    vec = vectors.reshape(-1, vectors.shape[-1]).contiguous()

    def status(a):
        return L.dcd_decode_detections(_lib.stream_of(vec), vec.data_ptr(), topk[0].data_ptr(), topk[2].data_ptr(), topk[3].data_ptr(),
                                       topk[4].data_ptr(), table.data_ptr(), a, rows.data_ptr(), aux.data_ptr(), None, None)
    a = ops.decode_args(spec, DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])
    a.K = 129
    assert status(a) == 1
    a = ops.decode_args(dict(spec, nk=129), DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])
    assert status(a) == 1
    a = ops.decode_args(dict(spec, orientation=ops.DECODE_ORIENTATION["head-axis"]), DH.BRANCH_B, DH.BRANCH_K, vec.shape[1])
    assert status(a) == 1
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((aux == -7.0).all())
    with pytest.raises(_lib.DcdHipError):
        ops.decode_detections(vectors, topk, table, dict(spec, nk=129))
    # head-axis: decode_fused raises with the reason
    pp_axis = _pp(cuda, "INPUT.ORIENTATION", "head-axis")
    preds, tg = _maps(cuda, 1)
    with pytest.raises(NotImplementedError, match="head-axis"):
        pp_axis.decode_fused(preds, tg)
    pp_iou = _pp(cuda, "TEST.EVAL_DIS_IOUS", True)
    with pytest.raises(NotImplementedError):
        pp_iou.decode_fused(preds, tg)


def test_head_axis_inference_falls_back_to_the_chain(cuda, tmp_path):
    """`inference(batch_size=2)` on a head-axis model: the fused decode refuses, the one-image loop writes the files.  (The device
    target encoder implements the multi-bin configuration only; what it encodes for evaluation does not depend on the model's
    orientation head, so the files and the pipeline keep the shipped configuration.)"""
    import test_input_host as IH
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path, [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False])
    files = KittiFiles(root, "train", cfg, is_train=False)
    torch.manual_seed(0)
    model = KeypointDetector(get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "INPUT.ORIENTATION", "head-axis"])).to(cuda)
    init_like_trained(model)
    assert not model.heads.post_processor.anno_encoder.multibin
    out = str(tmp_path / "out")
    result = inference(model, files, DeviceInputPipeline(cfg, cuda, is_train=False), out, batch_size=2)
    assert sorted(os.listdir(os.path.join(out, "data"))) == [files.img_id(i) + ".txt" for i in range(len(files))]
    assert "R40" in result
