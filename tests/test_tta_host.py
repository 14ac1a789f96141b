"""The mirrored-view merge of csrc/tta_math.h compiled for the HOST (tests/host/host_tta.cpp: the kernel's image loop in plain
loops) against the float64 restatement tests/tta_refs.py, on hand-made pairs of views where one rule each decides, then on the
seeded scenes the GPU test uses; and the route from the configuration and the command line to the pass, which needs no device.
The GPU build of the same header is checked in test_gpu_tta.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import tta_refs as R  # noqa: E402
from test_nms_host import block, row  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MODE_ID = {"2d": 1, "bev": 2, "3d": 3}

# Fused floats of the float32 build against float64, per column scale (tta_refs.fused_distance).  A fused float ends a chain of
# at most a dozen float32 operations -- un-mirror, two weights, the weighted sum, the ray, atan2f, the wrap -- on numbers no
# larger than its column's scale, the weights lying in [0, 1] and the inverse depth errors entering as a ratio: 12 roundings of
# 2^-24 relative each are 7.2e-7, and libm's atan2f adds under two units of pi's last place (2.4e-7 / pi each).  Bar: 1e-6.
HOST_BAR = 1e-6
W = 1242


@pytest.fixture(scope="module")
def host_tta(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_tta") / "libhost_tta.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_tta.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.host_tta_merge_detections.restype = ctypes.c_int
    lib.host_tta_merge_detections.argtypes = ([ctypes.c_void_p] * 5 + [ctypes.c_int] * 4 + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 7)
    lib.host_tta_unmirror.restype = None
    lib.host_tta_unmirror.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


def run_host(lib, rows, aux, K, widths, mode, match_thresh, det_threshold, scale, k2=None, k3=None):
    """The host build on (2 B K, .) arrays: (rows, aux, k2, k3, src, mate, overlaps (B, K, K))."""
    rows, aux = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(aux, np.float32)
    widths = np.ascontiguousarray(widths, np.int32)
    B = len(rows) // K // 2
    nk = 0 if k2 is None else k2.shape[1]
    outs = [None if a is None else np.full((B * K,) + a.shape[1:], np.nan, np.float32) for a in (rows, aux, k2, k3)]
    src, mate = np.full(B * K, -7, np.int32), np.full(B * K, -7, np.int32)
    ovl = np.full((B, K, K), np.nan, np.float32)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = lib.host_tta_merge_detections(p(rows), p(aux), p(k2), p(k3), p(widths), B, K, nk, MODE_ID[mode], match_thresh, det_threshold,
                                       scale, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(src), p(mate), p(ovl))
    assert st == 0
    return outs[0], outs[1], outs[2], outs[3], src, mate, ovl


def views(a_rows, m_rows_unmirrored, raw_a=None, raw_m=None, K=None, err_a=None, err_m=None, width=W):
    """One image: view A as given, view M = the mirror image of `m_rows_unmirrored` (so those are what the merge sees after it
    has un-mirrored them, up to float32 rounding).  Both padded to K with far-away rows under the threshold."""
    ra, xa = block(a_rows, raw_a, K)
    K = len(ra)
    rm, xm = block(m_rows_unmirrored, raw_m, K)
    rm = np.stack([R.mirror(r.astype(np.float64), width) for r in rm]).astype(np.float32)
    xa[:, 1] = 0.5 if err_a is None else np.resize(np.asarray(err_a, np.float32), K)
    xm[:, 1] = 0.5 if err_m is None else np.resize(np.asarray(err_m, np.float32), K)
    return np.concatenate([ra, rm]), np.concatenate([xa, xm]), K


def check(lib, rows, aux, K, mode="3d", match_thresh=0.5, det_threshold=0.2, scale=0.5, widths=(W,), k2=None, k3=None, matrices=None):
    """Host build == oracle: decisions, order and copies exactly, fused floats within HOST_BAR.  Returns (oracle, host outputs,
    distance)."""
    want = R.merge_batch(rows, aux, k2, k3, K, widths, mode, match_thresh, det_threshold, scale, matrices)
    got = run_host(lib, rows, aux, K, widths, mode, match_thresh, det_threshold, scale, k2, k3)
    R.assert_decisions_and_copies(got[:6], want, K, det_threshold)
    dist = R.fused_distance(got[0], got[1], want)
    assert dist <= HOST_BAR, dist
    return want, got, dist


def mates(want):
    """[(A rank, M rank)] of the oracle's matched pairs of image 0."""
    return [(a, int(m)) for a, m in enumerate(want["images"][0]["mate_of"]) if m >= 0]


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------
def test_an_exact_mirror_returns_view_a(host_tta):
    objs = [row(cls=0, box=(100.25, 100, 200.5, 180), xyz=(-3.0, 1.6, 20.0), ry=0.3, score=0.9),
            row(cls=1, box=(600, 120, 640, 220), hwl=(1.8, 0.6, 0.8), xyz=(2.0, 1.7, 12.0), ry=-2.9, score=0.8),
            row(cls=2, box=(900, 150, 980, 230), hwl=(1.7, 0.6, 1.8), xyz=(9.0, 1.5, 25.0), ry=3.1, score=0.7)]
    for r in objs:                                                       # an observation angle that belongs to the yaw and the place
        r[1] = R.wrap(float(r[12]) - np.arctan2(float(r[9]), float(r[11])))
    for width in (1242, 1241):
        rows, aux, K = views(objs, objs, K=4, width=width)
        for mode in R.MODES:
            want, got, _ = check(host_tta, rows, aux, K, mode, widths=(width,))
            assert mates(want) == [(0, 0), (1, 1), (2, 2)]
            assert np.array_equal(got[4], np.arange(4)) and list(got[5]) == [0, 1, 2, -1]
            assert np.array_equal(got[0][:3, 13], rows[:3, 13]) and np.array_equal(got[1][:3, 0], aux[:3, 0])
            d = np.abs(got[0][:3].astype(np.float64) - rows[:3])
            d[:, [1, 12]] = np.abs((d[:, [1, 12]] + np.pi) % (2 * np.pi) - np.pi)
            assert (d[:, 2:6] <= 2.5e-4).all() and (d[:, [1, 6, 7, 8, 9, 10, 11, 12]] <= 1e-5).all(), d.max(0)
            assert got[6][0, 0, 0] >= 0.99999 and got[6][0, 2, 2] >= 0.99999


def test_unmirroring_twice_is_the_identity(host_tta):
    rng = np.random.RandomState(0)
    for width in (1242, 1241):
        for _ in range(50):
            x = np.sort(rng.uniform(0, width - 1, 2))
            r = row(box=(x[0], 50.0, x[1], 90.0), xyz=(rng.uniform(-20, 20), 1.6, rng.uniform(3, 60)), ry=rng.uniform(-np.pi, np.pi))
            r[1] = R.wrap(float(r[12]) - np.arctan2(float(r[9]), float(r[11])))
            once, twice = np.zeros(14, np.float32), np.zeros(14, np.float32)
            p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            host_tta.host_tta_unmirror(p(r), width, p(once))
            host_tta.host_tta_unmirror(p(once), width, p(twice))
            want = R.unmirror(r, width)
            assert np.abs(once - want)[[2, 4]].max() <= 1.3e-4 and once[9] == -r[9] and abs(once[12] - want[12]) <= 5e-7
            assert abs(R.wrap(float(once[1]) - want[1])) <= 1e-6
            keep = [0, 3, 5, 6, 7, 8, 9, 10, 11, 13]
            assert np.array_equal(twice[keep], r[keep])
            assert np.abs(twice - r)[[2, 4]].max() <= 2.5e-4                # two roundings at the magnitude of the width
            assert abs(R.wrap(float(twice[12]) - float(r[12]))) <= 1e-6 and abs(R.wrap(float(twice[1]) - float(r[1]))) <= 2e-6


def test_yaw_at_pi_across_the_wrap_and_opposed(host_tta):
    base = dict(box=(100, 100, 200, 180), xyz=(1.0, 1.6, 20.0))
    for rya, rym in ((3.1, -3.1), (-3.1, 3.1), (np.pi, np.pi), (-np.pi, 3.0), (3.14, 3.12)):
        rows, aux, K = views([row(ry=rya, score=0.6, **base)], [row(ry=rym, score=0.3, **base)])
        want, got, _ = check(host_tta, rows, aux, K, "2d")
        assert mates(want) == [(0, 0)]
        d = R.wrap(rym - rya)
        assert abs(R.wrap(float(got[0][0, 12]) - R.wrap(rya + d / 3))) <= 1e-5       # wm = 0.3 / 0.9
    # more than a right angle apart: no mean; the yaw of the higher final score, a tie to A
    for sa, sm, takes_m in ((0.6, 0.3, False), (0.3, 0.6, True), (0.5, 0.5, False)):
        rows, aux, K = views([row(ry=0.2, score=sa, **base)], [row(ry=2.7, score=sm, **base)])
        want, got, _ = check(host_tta, rows, aux, K, "2d")
        assert mates(want) == [(0, 0)]
        assert abs(float(got[0][0, 12]) - (2.7 if takes_m else 0.2)) <= 1e-6
        assert got[0][0, 12] == np.float32(0.2) or takes_m                          # A's yaw keeps its bits


def test_weights_without_usable_scores_or_depth_errors(host_tta):
    a = dict(box=(100, 100, 200, 180), xyz=(1.0, 1.6, 20.0))
    m = dict(box=(104, 100, 204, 180), xyz=(1.2, 1.6, 22.0))
    for sa, sm in ((0.0, 0.0), (np.nan, 0.4), (0.4, np.nan)):
        rows, aux, K = views([row(score=sa, **a)], [row(score=sm, **m)], raw_a=[0.9], raw_m=[0.8])
        want, got, _ = check(host_tta, rows, aux, K, "2d")
        assert mates(want) == [(0, 0)]
        assert np.allclose(got[0][0, 2:6], [102, 100, 202, 180], atol=2e-4) and abs(got[0][0, 11] - 21.0) <= 1e-5
        assert got[1][0, 0] == np.float32(0.5 * (np.float32(0.9) + np.float32(0.8)))
    # usable scores, depth errors 0.5 and 1.5: the depth follows the inverse errors (3 : 1), the box the scores (3 : 1 the other way)
    rows, aux, K = views([row(score=0.2, **a)], [row(score=0.6, **m)], raw_a=[0.9], raw_m=[0.8], err_a=[0.5], err_m=[1.5])
    want, got, _ = check(host_tta, rows, aux, K, "2d")
    assert abs(got[0][0, 11] - 20.5) <= 1e-5 and abs(got[0][0, 2] - 103.0) <= 2e-4 and abs(got[1][0, 1] - 0.75) <= 1e-6
    assert abs(got[0][0, 9] - 20.5 * (0.25 * 1.0 / 20 + 0.75 * 1.2 / 22)) <= 1e-5
    # a depth error that is zero, negative, infinite or NaN: the score weights
    for ea, em in ((0.0, 1.5), (0.5, -1.0), (np.inf, 1.0), (0.5, np.nan)):
        rows, aux, K = views([row(score=0.2, **a)], [row(score=0.6, **m)], raw_a=[0.9], raw_m=[0.8], err_a=[ea], err_m=[em])
        want, got, _ = check(host_tta, rows, aux, K, "2d")
        assert abs(got[0][0, 11] - 21.5) <= 1e-5


def test_class_mismatch_and_the_unmatched_scale(host_tta):
    a = row(cls=1.3, score=0.8)
    rows, aux, K = views([a], [row(cls=2.1, score=0.7)])
    for scale in (0.0, 0.5, 1.0):
        for mode in R.MODES:
            want, got, _ = check(host_tta, rows, aux, K, mode, scale=scale)
            assert mates(want) == [] and got[5][0] == -1
            assert got[0][0, 13] == a[13] * np.float32(scale) and got[1][0, 0] == aux[0, 0] * np.float32(scale)
            assert R.same_bits(got[0][0, :13], a[:13]) and R.same_bits(got[1][0, 1:], aux[0, 1:])
    # the class is the integer part
    rows, aux, K = views([a], [row(cls=1.9, score=0.7)])
    want, _, _ = check(host_tta, rows, aux, K)
    assert mates(want) == [(0, 0)]
    # an M row whose raw score is NaN is not eligible; one under the detection threshold is
    for raw_m, matched in ((np.nan, False), (0.01, True)):
        rows, aux, K = views([a], [row(cls=1.0, score=0.7)], raw_m=[raw_m])
        want, got, _ = check(host_tta, rows, aux, K)
        assert (mates(want) == [(0, 0)]) == matched
        assert (got[6][0, 0, 0] > 0.9) == matched


def test_two_candidates_compete_in_final_score_order(host_tta):
    """A0 (rank 0, final score 0.3) overlaps the one M row better than A1 (rank 1, final score 0.8): A1 is visited first and
    takes it."""
    a0 = row(box=(100, 100, 200, 180), xyz=(0.0, 1.6, 20.0), score=0.3)
    a1 = row(box=(110, 100, 210, 180), xyz=(0.4, 1.6, 20.0), score=0.8)
    m0 = row(box=(101, 100, 201, 180), xyz=(0.04, 1.6, 20.0), score=0.5)
    rows, aux, K = views([a0, a1], [m0], raw_a=[0.9, 0.8], raw_m=[0.7], K=2)
    for mode in R.MODES:
        want, got, _ = check(host_tta, rows, aux, K, mode)
        assert got[6][0, 0, 0] > got[6][0, 1, 0] > 0.5
        assert mates(want) == [(1, 0)]
        # A1's fused raw score (0.75) now ranks above A0's scaled one (0.45)
        assert list(got[4]) == [1, 0] and list(got[5]) == [0, -1]
    # with the final scores the other way round A0 takes it and A1 stays alone
    rows[:2, 13] = [0.8, 0.3]
    want, got, _ = check(host_tta, rows, aux, K)
    assert mates(want) == [(0, 0)]


def test_equal_overlaps_go_to_the_lower_m_rank(host_tta):
    a0 = row(score=0.8)
    twin = row(box=(102, 100, 202, 180), xyz=(0.1, 1.6, 20.0), score=0.5)
    rows, aux, K = views([a0, row(box=(103, 100, 203, 180), xyz=(0.15, 1.6, 20.0), score=0.6)], [twin, twin], raw_m=[0.7, 0.6])
    for mode in R.MODES:
        want, got, _ = check(host_tta, rows, aux, K, mode)
        assert got[6][0, 0, 0] == got[6][0, 0, 1]
        assert mates(want) == [(0, 0), (1, 1)]                            # the second candidate gets the twin that is left


def test_a_scaled_candidate_leaves_the_prefix(host_tta):
    from dcd_amd.engine.inference import keep_prefix
    lonely = row(box=(500, 100, 600, 180), xyz=(8.0, 1.6, 20.0), score=0.3)
    paired = row(score=0.25)
    rows, aux, K = views([lonely, paired], [paired], raw_a=[0.3, 0.25], raw_m=[0.25], K=4)
    want, got, _ = check(host_tta, rows, aux, K, scale=0.5)
    assert mates(want) == [(1, 0)]
    assert list(got[4]) == [1, 0, 2, 3] and got[1][1, 0] == np.float32(0.3) * np.float32(0.5)
    assert keep_prefix(got[1][:, 0], 0.2) == 1 and keep_prefix(aux[:4, 0], 0.2) == 2
    # scale 1: both stay, in their order
    want, got, _ = check(host_tta, rows, aux, K, scale=1.0)
    assert list(got[4]) == [0, 1, 2, 3] and keep_prefix(got[1][:, 0], 0.2) == 2


def test_an_empty_prefix_and_a_single_row(host_tta):
    rows, aux, K = views([], [row(score=0.9)], K=3)
    for mode in R.MODES:
        want, got, _ = check(host_tta, rows, aux, K, mode)
        assert want["images"][0]["n"] == 0 and R.same_bits(got[0], rows[:3]) and R.same_bits(got[1], aux[:3])
        assert list(got[4]) == [0, 1, 2] and list(got[5]) == [-1] * 3 and (got[6] == 0).all()
    for m_rows in ([row(score=0.5)], [row(cls=2, score=0.5)]):
        rows, aux, K = views([row(score=0.9)], m_rows, K=1)
        want, got, _ = check(host_tta, rows, aux, K)
        assert K == 1 and len(got[0]) == 1 and list(got[5]) == [0 if m_rows[0][0] == 0 else -1]


# ---- seeded scenes ----------------------------------------------------------------------------------------------------------------
def test_seeded_scenes_and_the_distance_from_float64(host_tta):
    """The scenes of test_gpu_tta.py, every mode: decisions exactly, and the worst distance of the fused floats from float64 --
    the figure DESIGN.md "Mirrored-view test-time augmentation" quotes and test_gpu_tta.py's bar is four times of."""
    import tta_scenes
    worst = 0.0
    for bk in sorted(tta_scenes.SHAPES):
        s = tta_scenes.scene(bk)
        for mode in R.MODES:
            for nk in (None, 10):
                k2, k3 = (None, None) if nk is None else (np.ascontiguousarray(s["k2"][:, :nk]), np.ascontiguousarray(s["k3"][:, :nk]))
                want, got, dist = check(host_tta, s["rows"], s["aux"], bk[1], mode, s["match_thresh"], s["det_threshold"], 0.5,
                                        s["widths"], k2, k3, s["matrices"])
                worst = max(worst, dist)
            for b, n in enumerate(s["counts"]):
                m = s["matrices"][b][R.MODES.index(mode)]
                assert np.abs(got[6][b, :n] - m).max(initial=0) <= 1e-5 and (got[6][b, n:] == 0).all()
        print("B %d K %d: fused rows %d, distance so far %.3e" % (bk[0], bk[1], int(want["fused"].sum()), worst))
    print("host build, worst distance of a fused float from float64 over its column's scale: %.3e (bar %.1e)" % (worst, HOST_BAR))
    assert worst > 0


# ---- the route from the configuration and the command line, without a device ---------------------------------------------------
BASE = ["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "MODEL.USE_SYNC_BN", False]


def test_the_spec_and_the_configuration_key():
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.inference import TTASpec, resolve_tta
    d = TTASpec()
    assert (d.mode, d.match_thresh, d.unmatched_scale) == ("2d", 0.5, 0.5)
    for bad in (dict(mode="soft"), dict(mode="3D"), dict(match_thresh=-0.1), dict(match_thresh=1.0), dict(match_thresh=float("nan")),
                dict(unmatched_scale=-0.1), dict(unmatched_scale=1.5), dict(unmatched_scale=float("nan"))):
        with pytest.raises(ValueError):
            TTASpec(**bad)
    off, on = get_cfg(opts=BASE), get_cfg(opts=BASE + ["DATASETS.USE_TTA", True])
    assert resolve_tta(off) is None and resolve_tta(on) == TTASpec()
    mine = TTASpec("bev", 0.3, 1.0)
    assert resolve_tta(off, mine) is mine and resolve_tta(on, mine) is mine
    with pytest.raises(TypeError):
        resolve_tta(off, {"mode": "2d"})


def test_the_command_line_flags():
    import argparse
    from dcd_amd.engine.inference import TTASpec, add_tta_arguments, tta_from_arguments
    ap = argparse.ArgumentParser()
    add_tta_arguments(ap)
    assert tta_from_arguments(ap, ap.parse_args([])) is None
    assert tta_from_arguments(ap, ap.parse_args(["--tta"])) == TTASpec()
    got = tta_from_arguments(ap, ap.parse_args(["--tta", "--tta-match", "3d", "--tta-thresh", "0.25", "--tta-unmatched", "0"]))
    assert got == TTASpec("3d", 0.25, 0.0)
    for bad in (["--tta-thresh", "0.3"], ["--tta", "--tta-thresh", "1.0"], ["--tta", "--tta-match", "soft"], ["--tta", "--tta-unmatched", "2"]):
        with pytest.raises(SystemExit):
            tta_from_arguments(ap, ap.parse_args(bad))


class _Files:
    has_labels, root, classes = False, "", ("Car",)

    def __len__(self):
        return 2

    def img_id(self, i):
        return "%06d" % i

    def frame(self, i):
        return np.zeros((4, 6, 3), np.uint8)

    def sample(self, i):
        return {"image_size": (6, 4)}


def _stub_world(use_tta):
    import torch
    from dcd_amd.config import get_cfg

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = get_cfg(opts=BASE + ["DATASETS.USE_TTA", use_tta])

        def forward(self, images, targets):
            return [np.zeros((0, 14), np.float32)]

    class Pipe:
        is_train, device = False, "cpu"

        def __call__(self, frames, samples, img_ids=None):
            return None, None
    return Model(), _Files(), Pipe()


def test_without_tta_no_tta_code_is_reached_and_with_it_the_batched_pass_gets_the_spec(tmp_path, monkeypatch):
    """The one-image loop on stand-ins (no device): with USE_TTA False and tta=None the pass never enters the batched route and
    the merge is never looked up; with USE_TTA True, or a spec, the batched pass is entered with that spec, and its refusal is an
    error that names TTA."""
    from dcd_amd import ops
    from dcd_amd.engine import inference as inf

    def refuse(*a, **k):
        raise AssertionError("no TTA: the merge must not be reached")
    monkeypatch.setattr(ops, "tta_merge_detections", refuse)
    seen = []

    def batched(*a, **k):
        seen.append(k.get("tta"))
        return {}
    monkeypatch.setattr(inf, "_batched_pass", batched)
    model, files, pipe = _stub_world(False)
    assert inf.inference(model, files, pipe, str(tmp_path / "plain")) == {} and seen == []
    assert sorted(os.listdir(str(tmp_path / "plain" / "data"))) == ["000000.txt", "000001.txt"]
    mine = inf.TTASpec("3d", 0.4, 0.0)
    for use_tta, given, want in ((True, None, inf.TTASpec()), (False, mine, mine), (True, mine, mine)):
        model, files, pipe = _stub_world(use_tta)
        out = tmp_path / ("tta_%d" % len(seen))
        (out / "data").mkdir(parents=True)
        for i in ("000000", "000001"):                                   # (the stand-in pass writes nothing: finish_pass wants the files)
            open(str(out / "data" / (i + ".txt")), "w").close()
        assert inf.inference(model, files, pipe, str(out), tta=given) == {}
        assert seen[-1] == want
    assert len(seen) == 3

    def refuses(*a, **k):
        raise NotImplementedError("head-axis orientation")
    monkeypatch.setattr(inf, "_batched_pass", refuses)
    with pytest.raises(NotImplementedError, match="TTA"):
        inf.inference(*_stub_world(True), str(tmp_path / "refused"))
