"""The eval-time decode of csrc/decode_math.h compiled for the HOST (tests/host/host_decode.cpp: the kernel's candidate loop in
plain loops) against the reference's own `PostProcessor` output on pinned predictor maps (tests/golden/post_processor.npz), plus
the host-side pieces of the batched evaluation: the finite plan and the prefix rule.  The GPU build of the same header is checked
in test_gpu_decode.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import golden_inputs as gi  # noqa: E402
from test_host_golden import load, small_cfg  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host_decode(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_decode") / "libhost_decode.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_decode.cpp"), "-o", out])
    return ctypes.CDLL(out)


def run_host(lib, vectors, topk, table, spec, records=True):
    """`ops.decode_detections` on host tensors through the host build: (rows, aux, kpts2d, kpts3d) as numpy arrays."""
    from dcd_amd import ops
    scores, _, classes, ys, xs = topk
    B, K = scores.shape
    f = lambda t: np.ascontiguousarray(t.detach().float().numpy().reshape(-1))  # noqa: E731
    vec = np.ascontiguousarray(vectors.detach().float().numpy().reshape(B * K, -1))
    a = ops.decode_args(spec, B, K, vec.shape[1], records)
    rows, aux = np.full((B * K, 14), np.nan, np.float32), np.full((B * K, 4), np.nan, np.float32)
    k2, k3 = np.full((B * K, a.nk, 2), np.nan, np.float32), np.full((B * K, a.nk, 3), np.nan, np.float32)
    arrays = [vec, f(scores), f(classes), f(ys), f(xs), np.ascontiguousarray(table.numpy().astype(np.float32))]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = lib.host_decode_detections(*[p(x) for x in arrays], ctypes.byref(a), p(rows), p(aux), p(k2), p(k3))
    assert st == 0
    return rows, aux, k2, k3


def fixture_candidates(pp, device="cpu"):
    """Image 0 of the pinned predictor maps through the top-K and the POI gather: (vectors (1, 50, 415), topk, targets)."""
    from dcd_amd.model.layers.utils import select_point_of_interest, select_topk
    preds, targets = gi.loss_inputs()
    cls = torch.from_numpy(preds["cls"][:1]).to(device)
    reg = torch.from_numpy(preds["reg"][:1]).to(device)
    topk = select_topk(cls, K=pp.max_detection, fuse_nms=True)
    vectors = select_point_of_interest(1, topk[1], reg)
    return vectors, topk, [targets[0].to(device)]


def check_against_fixture(rows, aux, k2, k3, g, what):
    """The bars of `check_post_processor` (test_host_golden.py): class ids and raw scores equal, every other column of the rows
    within 1e-4 of that column's largest magnitude in the fixture, the fusion diagnostics at the same bar, the arg-max index
    equal, the key points within 1e-6 of their scale.  Returns the worst row-column ratio."""
    ref = g["result"]
    assert rows.shape == ref.shape
    np.testing.assert_array_equal(rows[:, 0], ref[:, 0])
    np.testing.assert_array_equal(aux[:, 0], g["vis_scores"].reshape(-1))
    scale = np.abs(ref).max(0) + 1e-6
    err = np.abs(rows - ref) / scale
    print("%s: worst column ratios %s" % (what, np.array2string(err.max(0), precision=2)))
    assert err.max() <= 1e-4, "decoded rows deviate: column %d by %.3e" % (int(err.max(0).argmax()), err.max())

    def close(a, key, t):
        r = g[key]
        assert np.abs(a.reshape(r.shape) - r).max() <= t * (np.abs(r).max() + 1e-6), key
    close(aux[:, 2], "uncertainty_conf", 1e-4)
    close(aux[:, 1], "estimated_depth_error", 1e-4)
    np.testing.assert_array_equal(aux[:, 3].astype(np.int64), g["min_uncertainty"].reshape(-1))
    close(k2, "gen_kpts_2d", 1e-6)
    close(k3, "gen_kpts_3d", 1e-6)
    close(k3, "pred_extra_kpts_3d", 1e-6)
    return float(err.max())


def image_kpts_from_normalised(k2, table):
    """u = x f_u + c_u, v = y f_v + c_v in float64: the image key points the K-normalised ones came from (one image).  The
    normalisation costs two fp32 roundings, 1.2e-7 |u - c_u| <= 2.4e-7 of the largest coordinate: inside the 1e-6 bar."""
    P = table[0, 4:].reshape(3, 4).astype(np.float64)
    k2 = k2.astype(np.float64)
    return np.stack((k2[..., 0] * P[0, 0] + P[0, 2], k2[..., 1] * P[1, 1] + P[1, 2]), axis=-1)


def test_host_build_matches_the_reference_fixture(cpu_backend, host_decode):
    from dcd_amd.model.head.detector_infer import make_post_processor
    g = load("post_processor")
    pp = make_post_processor(small_cfg("cpu"))
    vectors, topk, targets = fixture_candidates(pp)
    table = pp._image_table(targets, "cpu")
    rows, aux, k2, k3 = run_host(host_decode, vectors, topk, table, pp.decode_spec())
    check_against_fixture(rows, aux, k2, k3, g, "host build")
    # the image key points themselves (the fixture holds them in pixels): back from the normalised ones
    r = g["pred_extra_kpts_2d"]
    assert np.abs(image_kpts_from_normalised(k2, table.numpy()) - r).max() <= 1e-6 * (np.abs(r).max() + 1e-6)


def test_host_build_is_the_chain_on_the_other_branches(cpu_backend, host_decode):
    """`linear` dimensions (offset * std + mean) and the `exp` depth mode are one branch each in the header: against the
    op-by-op chain on the same candidates, at the fixture bar."""
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head.detector_infer import make_post_processor
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "MODEL.USE_SYNC_BN", False, "INPUT.WIDTH_TRAIN", 320,
                        "INPUT.HEIGHT_TRAIN", 96, "MODEL.HEAD.DIMENSION_REG", ["linear", True, True], "MODEL.HEAD.DEPTH_MODE", "exp",
                        "TEST.DETECTIONS_THRESHOLD", 0.0])
    pp = make_post_processor(cfg)
    vectors, topk, targets = fixture_candidates(pp)
    preds, _ = gi.loss_inputs()
    with torch.no_grad():
        ref, info, vis = pp({"cls": torch.from_numpy(preds["cls"][:1]), "reg": torch.from_numpy(preds["reg"][:1])}, targets)
    ref = ref.numpy()
    assert ref.shape == (50, 14)
    rows, aux, _, _ = run_host(host_decode, vectors, topk, pp._image_table(targets, "cpu"), pp.decode_spec())
    scale = np.abs(ref).max(0) + 1e-6
    assert (np.abs(rows - ref) / scale).max() <= 1e-4
    np.testing.assert_array_equal(aux[:, 3].astype(np.int64), vis["min_uncertainty"].numpy())


def test_finite_evaluation_plan():
    from dcd_amd.data.batches import EvalPlan
    plan = EvalPlan(7, 3)
    assert len(plan) == 3
    assert [plan(k)[0] for k in range(3)] == [[0, 1, 2], [3, 4, 5], [6]]
    assert all(not any(plan(k)[1]) and len(plan(k)[1]) == len(plan(k)[0]) for k in range(3))
    with pytest.raises(IndexError):
        plan(3)                                                   # never wraps around
    one = EvalPlan(4, 8)
    assert len(one) == 1 and one(0) == ([0, 1, 2, 3], [False] * 4)
    assert len(EvalPlan(0, 4)) == 0
    for bad in (0, -1):
        with pytest.raises(ValueError):
            EvalPlan(7, bad)


def test_prefix_rule_on_the_fixture_rows(tmp_path):
    """Raw scores leave the top-K in descending order, so `score >= threshold` keeps a prefix: 27 rows of the fixture at 0.8
    (scores 27 and 28 are 0.80105 and 0.79936), none at 1.0 -- then the file is the reference's empty prediction."""
    from dcd_amd.engine.inference import keep_prefix, write_image_rows
    from dcd_amd.eval import kitti_annos
    g = load("post_processor")
    rows, scores = g["result"], g["vis_scores"].reshape(-1)
    assert (np.diff(scores) <= 0).all()
    assert scores[26] >= 0.8 > scores[27]
    assert keep_prefix(scores, 0.8) == 27 == int((scores >= 0.8).sum())
    path = str(tmp_path / "000001.txt")
    assert write_image_rows(rows, scores, 0.8, path) == 27
    back = kitti_annos.read_anno(path)
    assert len(back["name"]) == 27
    np.testing.assert_allclose(back["score"], rows[:27, 13], atol=5.1e-5)
    np.testing.assert_allclose(back["bbox"], rows[:27, 2:6], atol=5.1e-5, rtol=1e-6)
    assert write_image_rows(rows, scores, 1.0, path) == 0
    assert open(path).read() == "\n" and len(kitti_annos.read_anno(path)["name"]) == 0
    assert keep_prefix(scores, 0.0) == 50 and keep_prefix(np.array([np.nan, 0.9]), 0.5) == 0


# ---- seeded random candidates on which every clamp and branch of the decode occurs ------------------------------------------
# N(0, sigma^2) per head.  Why these sigmas: the box distances must reach past both image borders from cells of an 80 x 24 map
# (30 cells); exp(-x) must leave DEPTH_RANGE = [0.1, 100] at both ends (|x| > 4.6: sigma 4); the fused error 4 / sum(1 / sigma_i)
# must fall below 0.01 and above 1 (log sigma beyond -4.6: sigma 3); the rest only has to spread over its branches.
BRANCH_SIGMA = {'2d_dim': 30.0, '3d_offset': 0.5, 'corner_offset': 2.0, 'corner_uncertainty': 3.0, '3d_dim': 0.3, 'ori_cls': 1.0,
                'ori_offset': 1.0, 'depth': 4.0, 'depth_uncertainty': 3.0, 'extra_kpts_2d': 2.0, 'extra_kpts_3d': 1.0}
BRANCH_SEED = 0
BRANCH_B, BRANCH_K = 2, 16


def branch_inputs(pp, device="cpu", seed=BRANCH_SEED):
    """(vectors (2, 16, 415), topk, targets): random head outputs handed over directly, scores descending per image."""
    rng = np.random.RandomState(seed)
    sl = pp.key2channel
    B, K = BRANCH_B, BRANCH_K
    vec = np.zeros((B, K, sum(sl.channels)), np.float32)
    for key in sl.keys:
        s = sl(key)
        vec[:, :, s] = rng.normal(0, BRANCH_SIGMA[key], (B, K, s.stop - s.start))
    scores = -np.sort(-rng.uniform(0.05, 0.95, (B, K)), axis=1)
    classes = rng.randint(0, 3, (B, K))
    ys, xs = rng.randint(0, 24, (B, K)), rng.randint(0, 80, (B, K))
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)  # noqa: E731
    topk = (t(scores), t(ys * 80 + xs, torch.int64), t(classes), t(ys), t(xs))
    _, targets = gi.loss_inputs()
    return t(vec), topk, [x.to(device) for x in targets[:B]]


def chain_on_candidates(pp, vectors, topk, targets):
    """`PostProcessor.forward_batch` -- the op-by-op chain -- on handed-over candidates, nothing cut: (rows, info, vis)."""
    B = vectors.shape[0]
    assert pp.det_threshold == 0.0
    heat = torch.zeros((B, 3, 24, 80), device=vectors.device)
    with torch.no_grad():
        rows, info, vis, image_of = pp.forward_batch({'cls': heat, 'reg': None, 'reg_pois': vectors, 'topk': topk}, targets)
    assert rows.shape[0] == vectors.shape[0] * vectors.shape[1]
    return rows, info, vis


def assert_every_branch_occurs(pp, vectors, targets, rows, info):
    """On the CHAIN's own output (rows, info of `chain_on_candidates`) and on the chain's own helper functions applied to the
    inputs: each clamp and branch of the decode happens at least once."""
    enc, sl = pp.anno_encoder, pp.key2channel
    vec = vectors.reshape(-1, vectors.shape[-1])
    n_per = vectors.shape[1]
    rows = rows.detach().cpu().double()
    box = rows[:, 2:6]
    lim = torch.tensor([[t.size[0] - 1, t.size[1] - 1] * 2 for t in targets], dtype=torch.float64).repeat_interleave(n_per, 0)
    assert (box == 0).any(), "no box side clamped at 0"
    assert (box == lim).any(), "no box side clamped at size - 1"
    corners = vec[:, sl('corner_offset')].view(-1, 10, 2)[:, :, 1]
    heights = corners[:, [8, 0, 2, 1, 3]] - corners[:, [9, 4, 6, 5, 7]]
    assert (heights <= 0).any() and (heights > 0).any(), "key-point heights on one side of 0 only"
    lo, hi = enc.depth_range
    direct = enc.decode_depth(vec[:, sl('depth')].squeeze(-1))
    dims = enc.decode_dimension(rows[:, 0].to(vec.device), vec[:, sl('3d_dim')])
    kd = enc.decode_depth_from_keypoints_batch(vec[:, sl('corner_offset')].view(-1, 10, 2), dims, [t.get_field("calib") for t in targets][:1])
    assert (direct == lo).any() and (direct == hi).any(), "the direct depth does not reach both ends of DEPTH_RANGE"
    # (a key-point depth f_u h / (4 height + EPS) at the lower end, 0.1, would take a projected height of ~2 500 cells)
    assert (kd == hi).any() and ((kd > lo) & (kd < hi)).any(), "no key-point depth clamped at the upper end of DEPTH_RANGE"
    # orientation: the bin is the chain's arg-max of the softmax; alpha = wrap(ori), roty = wrap(ori + ray), |ray| < pi / 2 (z > 0)
    nb = enc.orien_bin_size
    best = torch.softmax(vec[:, sl('ori_cls')].view(-1, nb, 2), dim=2)[..., 1].argmax(dim=1)
    assert sorted(set(best.tolist())) == list(range(nb)), "not every orientation bin is chosen"
    off = vec[:, sl('ori_offset')].view(-1, nb, 2)[torch.arange(vec.shape[0]), best]
    ori = (torch.atan2(off[:, 0], off[:, 1]) + enc.alpha_centers.to(vec.device)[best]).cpu().double()
    two_pi = 2 * np.pi
    a = torch.round((rows[:, 1] - ori) / two_pi)
    r = a + torch.round((rows[:, 12] - rows[:, 1]) / two_pi)
    assert (r == -1).any(), "roty never wrapped from above"
    assert (r == 1).any(), "roty never wrapped from below"
    err = info['estimated_depth_error'].detach().cpu()
    assert (err < 0.01).any(), "depth_error never clamped at 0.01"
    assert (err > 1).any(), "depth_error never clamped at 1"
    conf = info['uncertainty_conf'].detach().cpu()
    assert (conf == 0).any() and (conf == 1 - torch.tensor(0.01)).any()


def branch_post_processor(device):
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head.detector_infer import make_post_processor
    return make_post_processor(get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(device), "MODEL.USE_SYNC_BN", False,
                                             "INPUT.WIDTH_TRAIN", 320, "INPUT.HEIGHT_TRAIN", 96, "TEST.DETECTIONS_THRESHOLD", 0.0]))


def compare_with_chain(rows, aux, ref_rows, info, vis):
    """Rows at 1e-4 of each column's largest magnitude in the chain's rows; classes, raw scores and the arg-max index equal."""
    ref = ref_rows.detach().cpu().numpy()
    np.testing.assert_array_equal(rows[:, 0], ref[:, 0])
    np.testing.assert_array_equal(aux[:, 0], info['vis_scores'].detach().cpu().numpy().reshape(-1))
    np.testing.assert_array_equal(aux[:, 3].astype(np.int64), vis['min_uncertainty'].detach().cpu().numpy())
    assert np.isfinite(ref).all()
    err = np.abs(rows - ref) / (np.abs(ref).max(0) + 1e-6)
    print("worst column ratios against the chain: %s" % np.array2string(err.max(0), precision=2))
    assert err.max() <= 1e-4, "column %d deviates by %.3e" % (int(err.max(0).argmax()), err.max())


def test_host_build_on_candidates_where_every_clamp_and_branch_occurs(cpu_backend, host_decode):
    pp = branch_post_processor("cpu")
    vectors, topk, targets = branch_inputs(pp)
    ref, info, vis = chain_on_candidates(pp, vectors, topk, targets)
    assert_every_branch_occurs(pp, vectors, targets, ref, info)
    rows, aux, _, _ = run_host(host_decode, vectors, topk, pp._image_table(targets, "cpu"), pp.decode_spec())
    compare_with_chain(rows, aux, ref, info, vis)
