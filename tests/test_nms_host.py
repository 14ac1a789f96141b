"""The box NMS of csrc/nms_math.h compiled for the HOST (tests/host/host_nms.cpp: the kernel's image loop in plain loops) against
the float64 restatement tests/nms_refs.py, on hand-made blocks where one rule each decides, then on a seeded scene; and the
configuration errors of `PostProcessor`, which need no device.  The GPU build of the same header is checked in test_gpu_nms.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import nms_refs as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MODE_ID = {"2d": 1, "bev": 2, "3d": 3}


@pytest.fixture(scope="module")
def host_nms(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_nms") / "libhost_nms.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_nms.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.host_nms_detections.restype = ctypes.c_int
    lib.host_nms_detections.argtypes = ([ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_int]
                                        + [ctypes.c_void_p] * 5)
    return lib


def run_host(lib, rows, aux, K, mode, thresh, det_threshold, agnostic, k2=None, k3=None):
    """The host build on (B K, .) arrays: (rows_out, aux_out, k2_out, k3_out, overlaps (B, K, K))."""
    rows, aux = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(aux, np.float32)
    B = len(rows) // K
    nk = 0 if k2 is None else k2.shape[1]
    outs = [np.full_like(a, np.nan) if a is not None else None for a in (rows, aux, k2, k3)]
    ovl = np.full((B, K, K), np.nan, np.float32)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = lib.host_nms_detections(p(rows), p(aux), p(k2), p(k3), B, K, nk, MODE_ID[mode], thresh, det_threshold, int(agnostic),
                                 p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(ovl))
    assert st == 0
    return outs[0], outs[1], outs[2], outs[3], ovl


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def row(cls=0, box=(100, 100, 200, 180), hwl=(1.5, 1.6, 4.0), xyz=(0.0, 1.6, 20.0), ry=0.0, score=0.9):
    return np.array([cls, 0.1, *box, *hwl, *xyz, ry, score], np.float32)


def block(rows, raw=None, K=None):
    """rows -> ((K, 14), (K, 4)); raw defaults to the final scores; the block is padded with far-away rows under the threshold."""
    rows = [np.asarray(r, np.float32) for r in rows]
    K = K or max(len(rows), 1)
    raw = [r[13] for r in rows] if raw is None else list(raw)
    pad = K - len(rows)
    rows += [row(box=(900 + 3 * i, 10, 902 + 3 * i, 12), xyz=(-40.0 - 10 * i, 1.6, 70.0), score=0.01) for i in range(pad)]
    raw += [0.01] * pad
    aux = np.zeros((K, 4), np.float32)
    aux[:, 0] = raw
    aux[:, 1:] = np.arange(3 * K).reshape(K, 3)
    return np.stack(rows), aux


def check(lib, rows, aux, K, mode, thresh=0.5, det_threshold=0.2, agnostic=False, expect_keep=None):
    """Host build == oracle: the same permutation and marks, every float copied bit for bit.  Returns the oracle's result of
    image 0."""
    want = R.nms_batch(rows, aux, None, None, K, mode, thresh, det_threshold, agnostic)
    got = run_host(lib, rows, aux, K, mode, thresh, det_threshold, agnostic)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    res = want[4][0]
    if expect_keep is not None:
        assert list(np.nonzero(res["keep"])[0]) == list(expect_keep), res["keep"]
    # the prefix the host cuts is exactly the survivors
    from dcd_amd.engine.inference import keep_prefix
    for b, r in enumerate(want[4]):
        assert keep_prefix(got[1][b * K:(b + 1) * K, 0], det_threshold) == int(r["keep"].sum())
    return res, got


def test_empty_single_identical_and_touching(host_nms):
    for mode in R.MODES:
        # n = 0: nothing over the threshold, the block comes back as it was
        rows, aux = block([], K=3)
        res, got = check(host_nms, rows, aux, 3, mode, expect_keep=[])
        assert res["n"] == 0 and same_bits(got[0], rows) and same_bits(got[1], aux)
        # n = 1
        rows, aux = block([row()], K=2)
        check(host_nms, rows, aux, 2, mode, expect_keep=[0])
        # two identical boxes: overlap exactly 1, the second goes whatever the threshold below 1
        rows, aux = block([row(hwl=(1.5, 2.0, 4.0), ry=0.3, score=0.9), row(hwl=(1.5, 2.0, 4.0), ry=0.3, score=0.8)])
        for thresh in (0.0, 0.5, 0.999999):
            res, got = check(host_nms, rows, aux, 2, mode, thresh=thresh, expect_keep=[0])
            assert got[4][0, 0, 1] == 1.0 == got[4][0, 1, 0] and got[1][1, 0] == -np.inf
        # two touching boxes: overlap exactly 0, both stay at threshold 0 (the rule is a strict >)
        a = row(box=(100, 100, 200, 180), hwl=(1.5, 2.0, 4.0), xyz=(0.0, 1.6, 20.0))
        b = row(box=(200, 100, 300, 180), hwl=(1.5, 2.0, 4.0), xyz=(4.0, 1.6, 20.0), score=0.8)
        rows, aux = block([a, b])
        res, got = check(host_nms, rows, aux, 2, mode, thresh=0.0, expect_keep=[0, 1])
        assert got[4][0, 0, 1] == 0.0


def chain():
    """A > B > C in score along x: B overlaps A (shift 1 m of 4: 3/5), C overlaps B alike and A by 2/6 only."""
    mk = lambda i, s: row(box=(100 + 25 * i, 100, 200 + 25 * i, 180), xyz=(1.0 * i, 1.6, 20.0), score=s)  # noqa: E731
    return [mk(0, 0.9), mk(1, 0.8), mk(2, 0.7)]


def test_a_suppressed_box_suppresses_nothing(host_nms):
    rows, aux = block(chain())
    for mode in R.MODES:
        res, got = check(host_nms, rows, aux, 3, mode, thresh=0.5, expect_keep=[0, 2])
        # output order: survivors A, C in rank order, then B, marked
        assert same_bits(got[0], rows[[0, 2, 1]]) and got[1][2, 0] == -np.inf and np.isfinite(got[1][:2, 0]).all()
        m = res["matrix"][R.MODES.index(mode)]
        assert m[0, 1] > 0.5 and m[1, 2] > 0.5 and m[0, 2] < 0.5
        # visited the other way round (scores reversed) the middle box still goes, by the first one visited
        rev = rows.copy()
        rev[:, 13] = [0.7, 0.8, 0.9]
        check(host_nms, rev, aux, 3, mode, thresh=0.5, expect_keep=[0, 2])


def test_class_aware_against_agnostic(host_nms):
    """A Pedestrian and a Cyclist on the same person."""
    ped = row(cls=1, box=(300, 120, 340, 220), hwl=(1.8, 0.6, 0.8), xyz=(2.0, 1.7, 12.0), ry=0.2, score=0.8)
    cyc = row(cls=2, box=(298, 118, 343, 222), hwl=(1.75, 0.6, 0.9), xyz=(2.02, 1.7, 12.05), ry=0.25, score=0.6)
    rows, aux = block([ped, cyc])
    same = rows.copy()
    same[:, 0] = [1.02, 1.96]                                            # the class is the integer part: two Pedestrians
    for mode in R.MODES:
        check(host_nms, rows, aux, 2, mode, agnostic=False, expect_keep=[0, 1])
        check(host_nms, rows, aux, 2, mode, agnostic=True, expect_keep=[0])
        check(host_nms, same, aux, 2, mode, agnostic=False, expect_keep=[0])


def test_ties_nan_and_a_final_order_that_is_not_the_rank_order(host_nms):
    two = [row(score=0.7), row(score=0.7)]
    rows, aux = block(two, raw=[0.9, 0.8])
    check(host_nms, rows, aux, 2, "3d", expect_keep=[0])                 # a tie goes to the lower rank
    # a NaN final score is visited last: rank 0 is the one that goes
    rows, aux = block([row(score=np.nan), row(score=0.3)], raw=[0.9, 0.8])
    res, got = check(host_nms, rows, aux, 2, "bev", expect_keep=[1])
    assert np.isnan(got[0][1, 13]) and got[1][1, 0] == -np.inf and got[0][0, 13] == np.float32(0.3)
    rows, aux = block([row(score=np.nan), row(score=np.nan)], raw=[0.9, 0.8])
    check(host_nms, rows, aux, 2, "bev", expect_keep=[0])                # two NaNs: the lower rank first
    # UNCERTAINTY_AS_CONFIDENCE: raw scores descending, final scores not -- the chain visited C, B, A keeps C and A as well,
    # but a pair decides by the FINAL score
    rows, aux = block([row(score=0.2), row(score=0.6)], raw=[0.9, 0.8])
    res, got = check(host_nms, rows, aux, 2, "2d", expect_keep=[1])
    assert got[1][0, 0] == np.float32(0.8) and got[1][1, 0] == -np.inf
    # ... and the candidates are still cut by the RAW score: a high final score under the raw threshold is no candidate
    rows, aux = block([row(score=0.5), row(score=0.99)], raw=[0.9, 0.1])
    res, _ = check(host_nms, rows, aux, 2, "2d", expect_keep=[0])
    assert res["n"] == 1


def test_the_candidate_cut_is_the_hosts_float32_comparison(host_nms):
    """0.010131 rounds DOWN to float32: a raw score equal to the rounded value is below the threshold in float64 and at it in
    float32, which is how `keep_prefix` (numpy) and the op-by-op decode (torch) compare.  The kernel must count that row."""
    from dcd_amd.engine.inference import keep_prefix
    t = 0.010131
    edge = np.float32(t)
    assert float(edge) < t
    rows, aux = block([row(score=0.9), row(score=0.8)], raw=[0.9, edge], K=3)
    aux[2, 0] = np.nextafter(edge, np.float32(0))
    assert keep_prefix(aux[:, 0], t) == 2
    res, got = check(host_nms, rows, aux, 3, "3d", det_threshold=t, expect_keep=[0])
    assert res["n"] == 2 and got[1][1, 0] == -np.inf and got[1][2, 0] == aux[2, 0]


def test_the_three_modes_disagree_on_a_yawed_cluster(host_nms):
    """Four yawed boxes: a base, a near copy, a copy stacked above it (one footprint, no shared volume, another image box) and a
    copy whose image box alone coincides with the base's."""
    base = row(box=(400, 150, 520, 230), hwl=(1.5, 1.7, 4.2), xyz=(3.0, 1.6, 25.0), ry=0.7, score=0.9)
    near = row(box=(402, 151, 523, 232), hwl=(1.52, 1.68, 4.1), xyz=(3.1, 1.62, 25.1), ry=0.72, score=0.8)
    stacked = row(box=(400, 40, 520, 120), hwl=(1.5, 1.7, 4.2), xyz=(3.0, -0.2, 25.0), ry=0.7, score=0.7)
    far_same_box = row(box=(400, 150, 520, 230), hwl=(1.5, 1.7, 4.2), xyz=(-9.0, 1.6, 40.0), ry=-1.0, score=0.6)
    rows, aux = block([base, near, stacked, far_same_box])
    check(host_nms, rows, aux, 4, "2d", expect_keep=[0, 2])
    check(host_nms, rows, aux, 4, "bev", expect_keep=[0, 3])
    check(host_nms, rows, aux, 4, "3d", expect_keep=[0, 2, 3])


def test_a_seeded_scene_with_key_points_and_its_overlaps(host_nms):
    s = R.build_scene(seed=3, B=3, K=20, counts=[0, 1, 20], nk=10, confidence=True)
    for mode in R.MODES:
        for agnostic in (False, True):
            want = R.nms_batch(s["rows"], s["aux"], s["k2"], s["k3"], 20, mode, s["thresh"], s["det_threshold"], agnostic, s["matrices"])
            got = run_host(host_nms, s["rows"], s["aux"], 20, mode, s["thresh"], s["det_threshold"], agnostic, s["k2"], s["k3"])
            for g, w in zip(got[:4], want[:4]):
                assert same_bits(g, w)
            for b, n in enumerate(s["counts"]):
                m = s["matrices"][b][R.MODES.index(mode)]
                assert np.abs(got[4][b, :n, :n] - m).max(initial=0) <= 1e-5            # float32 area of a few m^2: see test_gpu_nms
                assert (got[4][b, n:] == 0).all() and (got[4][b, :, n:] == 0).all()


def test_post_processor_validates_the_three_keys():
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head.detector_infer import make_post_processor
    base = ["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "MODEL.USE_SYNC_BN", False]
    pp = make_post_processor(get_cfg(opts=base))
    assert pp.nms_mode == "none"                                         # the default: NMS_THRESH -1 is not looked at
    pp = make_post_processor(get_cfg(opts=base + ["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", 0.5, "TEST.NMS_CLASS_AGNOSTIC", True]))
    assert (pp.nms_mode, pp.nms_thresh, pp.nms_class_agnostic) == ("3d", 0.5, True)
    make_post_processor(get_cfg(opts=base + ["TEST.USE_NMS", "bev", "TEST.NMS_THRESH", 0.0]))
    for mode, thresh in (("3d", -1.0), ("2d", 1.0), ("bev", 1.5), ("3d", float("nan")), ("soft", 0.5), ("3D", 0.5), ("", 0.5)):
        with pytest.raises(ValueError):
            make_post_processor(get_cfg(opts=base + ["TEST.USE_NMS", mode, "TEST.NMS_THRESH", thresh]))
    with pytest.raises(ValueError):                                      # the kernel's limit, said at construction
        make_post_processor(get_cfg(opts=base + ["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", 0.5, "TEST.DETECTIONS_PER_IMG", 129]))
