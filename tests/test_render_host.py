"""The renderer's rule, csrc/render_math.h, compiled for the HOST (tests/host/host_render.cpp: the two kernels in plain loops)
against the float64 / Python-integer restatement tests/render_refs.py: bit for bit on canvas and integer table on hand-made exact
cases where one rule decides each (tests/render_cases.py), within a measured distance on the float ends of a seeded scene; and
the PNG writer of dcd_amd/engine/render.py, which needs no device.  The GPU build of the same header is checked in
test_gpu_render.py against this host build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import render_cases as C  # noqa: E402
import render_refs as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

def build_host_render(directory):
    out = os.path.join(str(directory), "libhost_render.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_render.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    lib.host_render_detections.restype = ci
    lib.host_render_detections.argtypes = [vp, u64] + [vp] * 8 + [ci] * 6 + [ctypes.c_double] * 2 + [vp] * 4
    lib.host_render_primitives.restype = ci
    lib.host_render_primitives.argtypes = [vp, u64, vp, vp] + [ci] * 4 + [vp]
    lib.host_render_slots.restype = ci
    lib.host_render_slots.argtypes = [ci] * 3
    return lib


@pytest.fixture(scope="module")
def host_render(tmp_path_factory):
    return build_host_render(tmp_path_factory.mktemp("host_render"))


def stage(frames):
    """The staged buffer of the input pipeline (`_pack`'s layout) as a numpy array."""
    B = len(frames)
    offsets, nbytes = [], -(-B * 40 // 64) * 64
    for f in frames:
        offsets.append(nbytes)
        nbytes += -(-f.size // 64) * 64
    host = np.zeros(nbytes, np.uint8)
    rec = host[:B * 40].view(np.int64).reshape(B, 5)
    for i, (f, off) in enumerate(zip(frames, offsets)):
        rec[i] = (off, 3 * f.shape[1], f.shape[0], f.shape[1], 0)
        host[off:off + f.size] = f.reshape(-1)
    return host


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def run_host(lib, case):
    """The host build on a case: (canvas, table, counts, ends)."""
    staged = stage(case["frames"])
    B, K = len(case["frames"]), case["K"]
    k2 = case["k2"] if case["keypoints"] else None
    nk = k2.shape[1] if k2 is not None else 0
    gt = case["gt"]
    M = 0 if gt is None else gt[0].shape[1]
    S = lib.host_render_slots(M, K, nk)
    table = np.full((B, S, 12), 77, np.int32)
    counts = np.full(B, -5, np.int32)
    ends = np.full((B, S, 4), np.nan, np.float32)
    canvas = np.full((B, case["in_h"], case["in_w"] + case["in_h"], 3), 99, np.uint8)
    tab = C.image_table(case["P"], [f.shape[1::-1] for f in case["frames"]], case["in_h"], case["in_w"])
    g = [None] * 4 if gt is None else [np.ascontiguousarray(t) for t in gt]
    rows, aux = np.ascontiguousarray(case["rows"], np.float32), np.ascontiguousarray(case["aux"], np.float32)
    st = lib.host_render_detections(_p(staged), staged.size, _p(rows), _p(aux), _p(k2), _p(tab), _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]),
                                    B, K, nk, M, case["in_h"], case["in_w"], case["det"], case["vis"], _p(table), _p(counts), _p(ends),
                                    _p(canvas))
    assert st == 0
    return canvas, table, counts, ends


def run_ref(case):
    heights = [f.shape[0] for f in case["frames"]]
    table, counts, ends = R.batch_table(case["rows"], case["aux"], case["k2"], case["P"], case["gt"], case["K"], heights, case["det"],
                                        case["vis"], case["keypoints"])
    return R.raster(case["frames"], table, counts, case["in_h"], case["in_w"]), table, counts, ends


def run_host_primitives(lib, frames, table, counts, in_h=C.IN_H, in_w=C.IN_W):
    staged = stage(frames)
    canvas = np.full((len(frames), in_h, in_w + in_h, 3), 99, np.uint8)
    st = lib.host_render_primitives(_p(staged), staged.size, _p(table), _p(counts), len(frames), table.shape[1], in_h, in_w, _p(canvas))
    assert st == 0
    return canvas


def picture_mask(frames, in_h, in_w):
    m = np.zeros((len(frames), in_h, in_w + in_h), bool)
    for b, f in enumerate(frames):
        m[b, :f.shape[0], :f.shape[1] + f.shape[0]] = True
    return m


# ---- hand-made exact cases: the whole route --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.HAND_MADE))
def test_host_build_equals_the_restatement_on_exact_cases(host_render, name):
    case = C.HAND_MADE[name]()
    canvas, table, counts, _ = run_host(host_render, case)
    want_canvas, want_table, want_counts, _ = run_ref(case)
    assert np.array_equal(table, want_table), "integer table: first difference at %s" % (np.argwhere(table != want_table)[:1],)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(canvas, want_canvas), "%d canvas bytes differ" % (canvas != want_canvas).sum()
    assert not canvas[~picture_mask(case["frames"], case["in_h"], case["in_w"])].any(), "bytes outside the picture must be 0"


def _drawn(table, b, lo, hi):
    return [i for i in range(lo, hi) if table[b, i, 1] >= 0]


def test_overlap_case_draws_what_the_rule_says(host_render):
    """The case decides the rules it was made for: not only host == restatement."""
    case = C.case_overlap()
    canvas, table, counts, _ = run_host(host_render, case)
    K, per, gt0 = 6, 28, 17 * 3
    assert _drawn(table, 0, 17, 34) == [], "an unused ground-truth slot draws nothing"
    assert len(_drawn(table, 0, 0, 17)) == 17 and len(_drawn(table, 0, 34, 51)) == 17
    for rank in (2, 3, 4, 5):                                              # suppressed, score == vis, under the threshold, NaN
        j = K - 1 - rank
        assert _drawn(table, 0, gt0 + j * per, gt0 + (j + 1) * per) == [], "rank %d must not draw" % rank
    for rank in (0, 1):
        j = K - 1 - rank
        assert len(_drawn(table, 0, gt0 + j * per, gt0 + (j + 1) * per)) == per
    assert counts[1] == 0 and counts[0] == gt0 + K * per
    frame = case["frames"][0]
    # rank 0's rectangle (30, 20)-(90, 60) crosses rank 1's (40, 24)-(100, 64) at (90, 24) and (40, 60): rank 0's green wins,
    # and its predicted-box colour lies over the ground truth's where their edges coincide
    assert tuple(canvas[0, 20, 50]) == (0, 255, 0)
    pred, gt = np.array((25, 202, 173)), np.array((244, 96, 108))
    img = canvas[0, :77, :197]
    assert (img == pred).all(-1).any() and (img == gt).all(-1).any()
    untouched = (img == frame).all(-1)
    assert 0.5 < untouched.mean() < 1.0
    assert np.array_equal(canvas[1, :33, :150], case["frames"][1]) and (canvas[1, :33, 150:183] == 230).all()


def test_near_plane_case_clips_and_drops(host_render):
    case = C.case_near()
    _, table, _, ends = run_host(host_render, case)
    K, nk = 5, 3
    per = 28 + nk
    base0 = (K - 1) * per                                                  # rank 0 is drawn last
    kinds = table[0, base0 + 4:base0 + 18, 1]
    # corners 1, 2, 5, 6 lie at z = 0: edges between two of them go, edges to z = 2 are cut at z = 0.125
    dropped = [i for i, (p, q) in enumerate(R.BOX_EDGES) if {p, q} <= {1, 2, 5, 6}]
    assert [i for i in range(14) if kinds[i] < 0] == dropped and len(dropped) == 4
    cut = R.BOX_EDGES.index((0, 1))
    assert tuple(ends[0, base0 + 4 + cut]) == (224.0, 168.0, 2144.0, 2088.0)   # ((256 + 96 z) / z, (256 + 40 z) / z) at z = 2, 0.125
    base1 = (K - 2) * per                                                  # rank 1: wholly nearer than the plane
    assert (table[0, base1 + 4:base1 + 18, 1] < 0).all() and (table[0, base1 + 18 + nk:base1 + 23 + nk, 1] == 0).all()
    assert table[0, base0 + 18 + 1, 1] < 0 and table[0, base0 + 18, 1] == 0    # the NaN key point, and a drawn one
    label = table[0, base0 + 23 + nk:base0 + 28 + nk]
    assert [R.GLYPH_ORDER[g] for g in label[:, 11]] == list("Y0.99") and label[0, 3] == 3 - 8
    label = table[0, base0 - 2 * per + 23 + nk:base0 - 2 * per + 28 + nk]      # rank 2: a negative score prints 0.00
    assert [R.GLYPH_ORDER[g] for g in label[:, 11]] == list("P0.00")
    label = table[0, base0 - 3 * per + 23 + nk:base0 - 3 * per + 28 + nk]      # rank 3: class 0.75 is class 0; box (-4.5, -3.5)
    assert [R.GLYPH_ORDER[g] for g in label[:, 11]] == list("C0.00") and tuple(label[0, 2:4]) == (-4, -3 - 8)
    label = table[1, base0 + 23 + nk:base0 + 28 + nk]
    assert [R.GLYPH_ORDER[g] for g in label[:, 11]] == list("C0.99")


def test_skipped_coordinates(host_render):
    case = C.case_skips()
    _, table, _, _ = run_host(host_render, case)
    K, per = 4, 28
    rect = lambda rank: table[0, (K - 1 - rank) * per:(K - 1 - rank) * per + 4, 1]   # noqa: E731
    assert list(rect(0)) == [-1, -1, -1, 0]                                # 2^24 is skipped, the left side stays
    assert list(rect(1)) == [0, 0, 0, 0]                                   # 2^24 - 1 is drawn
    assert list(rect(2)) == [-1, -1, -1, -1]
    assert (table[0, (K - 1 - 2) * per + 23:(K - 1 - 2) * per + 28, 1] < 0).all()   # and so is its label
    edges = table[0, (K - 1 - 3) * per + 4:(K - 1 - 3) * per + 18, 1]                # NaN height: the bottom face's edges only
    assert [i for i in range(14) if edges[i] == 0] == [i for i, (p, q) in enumerate(R.BOX_EDGES) if p < 4 and q < 4]


# ---- the raster alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.TABLES))
def test_host_raster_equals_the_restatement(host_render, name):
    table, counts = C.TABLES[name]()
    frames = C.frames_of(C.SIZES, seed=1)
    canvas = run_host_primitives(host_render, frames, table, counts)
    want = R.raster(frames, table, counts, C.IN_H, C.IN_W)
    assert np.array_equal(canvas, want), "%d canvas bytes differ" % (canvas != want).sum()
    assert not canvas[~picture_mask(frames, C.IN_H, C.IN_W)].any()


def test_a_to_b_equals_b_to_a(host_render):
    frames = C.frames_of(C.SIZES, seed=1)
    fwd = run_host_primitives(host_render, frames, *C.table_octants(False))
    back = run_host_primitives(host_render, frames, *C.table_octants(True))
    assert np.array_equal(fwd, back)
    assert np.array_equal(R.raster(frames, *C.table_octants(True), C.IN_H, C.IN_W), fwd)


def test_clipped_walk_equals_the_unclipped_rule():
    """The restatement's own shortcut (the analytic cut of the step range) against the rule walked in full."""
    rng = np.random.RandomState(0)
    for _ in range(200):
        x0, y0, x1, y1 = (int(v) for v in rng.randint(-60, 120, 4))
        T = int(rng.randint(1, 5))
        full = {(x, y) for x, y in R.segment_pixels(x0, y0, x1, y1, T) if 0 <= x < 50 and 0 <= y < 40}
        assert set(R._clipped_segment_pixels(x0, y0, x1, y1, T, 50, 40)) == full


def test_seam_and_rows(host_render):
    table, counts = C.table_seam()
    frames = C.frames_of(C.SIZES, seed=1)
    canvas = run_host_primitives(host_render, frames, table, counts)
    for b, (w, h) in enumerate(C.SIZES):
        assert not (canvas[b, :, w:] == (1, 2, 3)).all(-1).any(), "an image-panel line reached the bird's-eye panel"
        assert not (canvas[b, :, :w] == (3, 2, 1)).all(-1).any(), "a bird's-eye line reached the image panel"
        assert (canvas[b, :, w - 20:w] == (1, 2, 3)).all(-1).any() and (canvas[b, :, w:w + 21] == (3, 2, 1)).all(-1).any()
        assert not (canvas[b] == (9, 9, 9)).all(-1).any() and (canvas[b, h - 1] == (9, 1, 9)).all(-1).any()
        assert not (canvas[b] == (255, 255, 255)).all(-1).any(), "an invalid entry drew"
        assert not canvas[b, h:].any()
        assert tuple(canvas[b, 5, 50]) == (50, 60, 70) and tuple(canvas[b, 25, 50]) == (2, 2, 2)


# ---- the seeded scene: float ends against float64 ---------------------------------------------------------------------------
def ends_distance(ends, want, table, want_table):
    """Worst |difference| over EVERY slot and coordinate; the slots' kinds must agree."""
    assert np.array_equal(table[:, :, 1], want_table[:, :, 1]), "drawn / not drawn differs"
    assert np.isfinite(want).all() and np.isfinite(ends).all()
    return float(np.abs(ends.astype(np.float64) - want).max())


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_float_ends_of_the_seeded_scenes(host_render, name):
    """fp32 against float64 on every slot.  The bar is eight units in the last place of the largest coordinate: a coordinate is the
    end of a chain of about ten fp32 operations (rotation, translation, clip, projection) on values of its own magnitude or less,
    each within half a unit.  What the host build measures is recorded in render_cases.HOST_ENDS_DISTANCE for the device's test."""
    case = C.SCENES[name]()
    canvas, table, counts, ends = run_host(host_render, case)
    _, want_table, _, want = run_ref(case)
    assert (table[:, :, 1] >= 0).sum() > 3000, "the scene must draw"
    worst = ends_distance(ends, want, table, want_table)
    bar = 8 * float(np.spacing(np.float32(np.abs(want).max())))
    print("host build, %s scene, float ends: worst distance from float64 %.4e px (bar %.2e, recorded %.4e)"
          % (name, worst, bar, C.HOST_ENDS_DISTANCE[name]))
    assert worst <= bar
    assert worst <= 1.5 * C.HOST_ENDS_DISTANCE[name], "the recorded distance no longer describes the host build"
    drawn = table[:, :, 1] == 0
    assert np.array_equal(table[:, :, 2:6][drawn], np.trunc(ends[drawn]).astype(np.int32)), "the table is the truncation of the ends"
    assert np.array_equal(canvas, R.raster(case["frames"], table, counts, case["in_h"], case["in_w"])), "canvas != raster of the host's table"
    assert table.shape[1] == R.slots(7, 50, 73)


# ---- the PNG writer ----------------------------------------------------------------------------------------------------------
def test_png_writer_round_trip(tmp_path):
    from PIL import Image
    from dcd_amd.engine.render import PngWriter
    rng = np.random.RandomState(0)
    canvas = rng.randint(0, 256, size=(3, C.IN_H, C.IN_W + C.IN_H, 3)).astype(np.uint8)
    sizes = [(197, 77), (150, 33), (200, 80)]
    ids = ["000003", "000007", "000011"]
    writer = PngWriter(str(tmp_path / "pictures"), workers=2)
    writer.submit(canvas, ids, sizes)
    writer.close()
    assert sorted(os.listdir(str(tmp_path / "pictures"))) == [i + ".png" for i in ids]
    for b, (img_id, (w, h)) in enumerate(zip(ids, sizes)):
        back = np.asarray(Image.open(str(tmp_path / "pictures" / (img_id + ".png"))))
        assert back.shape == (h, w + h, 3) and np.array_equal(back, canvas[b, :h, :w + h])
