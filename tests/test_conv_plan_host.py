"""The convolutions' host arithmetic (csrc/conv_plan.h) on the CPU.

(1) The *_bytes entry points of the built library return the sizes recorded before the header existed
    (tests/golden/conv_plans.json, written by tests/golden/make_golden_conv_plans.py from that commit's library): every shape
    list of tests/test_gpu_conv.py at its own batch and at one and eight images, default environment.
(2) The header compiled with plain g++ (tests/host/conv_plan_host.cpp) returns the same sizes at 256 CUs, the count the library
    falls back to without a device.
(3) At 64, 256 and 304 CUs, for every recorded geometry, form and direction: what conv3x3_run needs is at most what the form's
    *_workspace_bytes advertises (the plans read one member for both, but the advertised size does not know the direction, the
    fp32 form bounds its weights by the larger channel count, and nothing else checks it); the contraction split is 1, 2, 4 or 8;
    the output slices cover the produced channels and the regions cover the map."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_conv_plans as rec  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "conv_plans.json")))
GEOMS = [tuple(q) for q in GOLDEN["geometries"]]
QUERY = ("shape_ok", "need_prepared", "need_raw", "advertised", "ksplit", "nz", "nb", "Kk", "tiles_x", "tiles_y", "rows", "cols")


def test_golden_covers_the_gpu_tests_geometries():
    assert GEOMS == [tuple(q) for q in rec.geometries()]
    assert list(GOLDEN["bytes"]) == rec.SIZE_NAMES
    for name, got in GOLDEN["bytes"].items():
        by_geom = dict(zip(GEOMS, got))
        assert all(by_geom[q] == 0 for q in rec.INVALID), name
        assert all((by_geom[q] > 0) == (name in rec.BATCH_FREE) for q in rec.NO_IMAGE), name
        if name != "s2_wrw_workspace":                           # (its shape rule turns some of the stride-1 shapes away)
            assert all(n > 0 for q, n in by_geom.items() if q not in rec.INVALID + rec.NO_IMAGE), name
    s2 = dict(zip(GEOMS, GOLDEN["bytes"]["s2_wrw_workspace"]))
    assert all(s2[(b, C, H, W, K)] > 0 for B, C, K, H, W in rec.INLINE["test_stride2_conv_native_fp32_kernels"] for b in (B, 1, 8))


def test_library_sizes_are_the_recorded_ones():
    from dcd_amd import _lib
    got = rec.sizes(_lib.lib(), GEOMS)
    for name, want in GOLDEN["bytes"].items():
        bad = [(q, g, w) for q, g, w in zip(GEOMS, got[name], want) if g != w]
        assert not bad, (name, bad[:5])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv_plan") / "libconv_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "conv_plan_host.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    assert L.conv_plan_size_count() == rec.HOST_SIZES

    def sizes(cus, q):
        o = (ctypes.c_ulonglong * rec.HOST_SIZES)()
        L.conv_plan_sizes(cus, (ctypes.c_int * 5)(*q), o)
        return [int(v) for v in o]

    def query(form, cus, q, backward):
        o = (ctypes.c_ulonglong * len(QUERY))()
        if not L.conv_plan_query(form, cus, (ctypes.c_int * 5)(*q), backward, o):
            return None
        return dict(zip(QUERY, (int(v) for v in o)))
    return sizes, query


def test_header_alone_returns_the_recorded_sizes_at_256_cus(host):
    sizes, _ = host
    names = rec.SIZE_NAMES[:rec.HOST_SIZES]
    for i, q in enumerate(GEOMS):
        want = [GOLDEN["bytes"][n][i] for n in names]
        assert sizes(256, q) == want, (q, dict(zip(names, zip(sizes(256, q), want))))


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_a_run_needs_no_more_than_is_advertised_and_the_plan_covers_the_call(host, cus):
    _, query = host
    seen = {"split": 0, "ok": 0, "refused": 0}
    for q in GEOMS:
        for form in range(3):
            for backward in (0, 1):
                p = query(form, cus, q, backward)
                if q in rec.INVALID + rec.NO_IMAGE:
                    assert p is None
                    continue
                what = "%s form %d backward %d at %d CUs: %s" % (q, form, backward, cus, p)
                assert p["need_prepared"] <= p["need_raw"] <= p["advertised"], what
                assert p["ksplit"] in (1, 2, 4, 8), what
                assert p["need_prepared"] == (p["ksplit"] - 1) * q[0] * p["Kk"] * q[2] * q[3] * 4, what
                assert p["nb"] in (1, 2) and p["nz"] * 32 * p["nb"] >= p["Kk"] > (p["nz"] - 1) * 32 * p["nb"], what
                assert p["tiles_x"] * p["cols"] >= q[3] > (p["tiles_x"] - 1) * p["cols"], what
                assert p["tiles_y"] * p["rows"] >= q[2] > (p["tiles_y"] - 1) * p["rows"], what
                seen["split"] += p["ksplit"] > 1
                seen["ok" if p["shape_ok"] else "refused"] += 1
    assert seen["split"] and seen["ok"] and seen["refused"]          # the lists reach split contractions and both verdicts
