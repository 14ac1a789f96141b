"""The DCN workspace map (csrc/dcn_workspace.h) on the CPU.

(1) dcd_dcn_v2_workspace_bytes returns the sizes recorded before the map existed (tests/golden/dcn_workspace_bytes.json, written
    by tests/golden/make_golden_dcn_workspace.py from that commit's library): every list of tests/test_gpu_dcn.py at one and eight
    images and at its own batch, under the per-call switches the size depends on.
(2) The header compiled with plain g++ (tests/host/dcn_workspace_host.cpp) gives, for the same geometries and switches, regions
    that lie inside the advertised size, are aligned for their widest access, and do not overlap within a pass -- except the
    overlays named in FORWARD_OVERLAYS."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_dcn_workspace as rec  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "dcn_workspace_bytes.json")))
GEOMS = [tuple(q) for q in GOLDEN["geometries"]]

# Alignment each region's widest access needs.  256: where the layout rounds to 256 (scalars, the byte tables, the far-tile
# list behind them).  16: float4 / dwordx4 accesses (weight layouts, partials, column buffers, Tt rows).  4: the inverse lists'
# idx / w planes, [B][S][INV_CAP][HW] read one dword per lane.
ALIGN = {"wf": 16, "wb": 16, "scalars": 256, "inv_cnt": 256, "inv_idx": 4, "inv_w": 4, "far_flag": 256, "far_list": 256,
         "dw_part": 16, "blockmax": 256, "tileflag": 256, "dense_col": 16, "dense_part": 16, "sw_wp": 16, "sw_cpart": 16,
         "sw_dwpart": 16, "sw_col": 16, "fwd_wl": 16, "fwd_wf9": 16, "fwd_flags": 4, "fwd_far_count": 4, "fwd_w9": 16}
BACKWARD = ["wf", "wb", "scalars", "inv_cnt", "inv_idx", "inv_w", "far_flag", "far_list", "dw_part", "blockmax", "tileflag",
            "dense_col", "dense_part", "sw_wp", "sw_cpart", "sw_dwpart", "sw_col"]
# The forward re-uses the backward's areas, which are dead then.  The only overlaps there are:
FORWARD_OVERLAYS = {
    "fwd_wl": {"wf", "wb"},                   # the tile kernel's weights Wl over [Wf | Wb]
    "fwd_wf9": {"wf", "wb"},                  # the rescue pass's weights Wf9 over the same area (behind Wl)
    "fwd_w9": {"wf", "wb"},                   # the plain 3x3 route's weights where Wf is
    "fwd_flags": {"scalars", "inv_cnt", "inv_idx"},       # region flags and far counter behind the weights
    "fwd_far_count": {"scalars", "inv_cnt", "inv_idx"},
}
# (backward: none.  Tt shares the column buffer as ONE region, dense_col; the tile flags follow the block maxima as a region of
# their own, so "the tail of the block-maxima area" is not an overlap in the map either)


def test_golden_covers_the_gpu_tests_geometries():
    assert GEOMS == [tuple(q) for q in rec.geometries()]
    assert sorted(GOLDEN["bytes"]) == sorted(rec.env_key(e) for e in rec.ENVS)
    invalid = GEOMS.index((8, 64, 96, 320, 64, 3, 3, 0, 1, 1, 1, 1, 1, 1))
    assert all(v[invalid] == 0 for v in GOLDEN["bytes"].values())
    assert all(n > 0 for v in GOLDEN["bytes"].values() for i, n in enumerate(v) if i != invalid)


def test_workspace_bytes_are_the_recorded_ones():
    from dcd_amd import _lib
    got = rec.sizes(_lib.lib().dcd_dcn_v2_workspace_bytes, GEOMS)
    for key, want in GOLDEN["bytes"].items():
        bad = [(q, g, w) for q, g, w in zip(GEOMS, got[key], want) if g != w]
        assert not bad, (key, bad[:5])


@pytest.fixture(scope="module")
def host_map(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dcn_workspace") / "libdcn_workspace_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "dcn_workspace_host.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.dcn_ws_region_name.restype = ctypes.c_char_p
    names = [L.dcn_ws_region_name(i).decode() for i in range(L.dcn_ws_region_count())]
    assert sorted(names) == sorted(ALIGN)

    def query(q, which):
        regions = (ctypes.c_ulonglong * (2 * len(names)))()
        info = (ctypes.c_ulonglong * 7)()
        if not L.dcn_ws_map((ctypes.c_int * 14)(*q), which, regions, info):
            return None
        reg = {n: (int(regions[2 * i]), int(regions[2 * i + 1])) for i, n in enumerate(names)}
        return reg, dict(zip(("total", "base_end", "dense_end", "has_dense", "has_sweep", "has_tile", "fwd_dense"), map(int, info)))
    return query


def _overlap(a, b):
    return a[1] > 0 and b[1] > 0 and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def _check_regions(reg, used, total, what):
    for n in used:
        off, size = reg[n]
        if size == 0:
            continue
        assert off + size <= total, "%s: %s [%d, %d) leaves the %d advertised bytes" % (what, n, off, off + size, total)
        assert off % ALIGN[n] == 0, "%s: %s at %d is not %d-byte aligned" % (what, n, off, ALIGN[n])
    for i, a in enumerate(used):
        for b in used[i + 1:]:
            assert not _overlap(reg[a], reg[b]), "%s: %s %s overlaps %s %s" % (what, a, reg[a], b, reg[b])


@pytest.mark.parametrize("env", rec.ENVS, ids=rec.env_key)
def test_map_regions_are_inside_aligned_and_disjoint(host_map, monkeypatch, env):
    for k in ("DCD_DCN_DENSE", "DCD_BWD_SWEEP", "DCD_NO_TILE", "DCD_TILE_ROWS", "DCD_SWEEP_SLOTS", "DCD_SWEEP_MIN_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = GOLDEN["bytes"][rec.env_key(env)]
    seen = {"dense": 0, "sweep": 0, "tile": 0, "fwd_dense": 0, "plain": 0}
    for q, nbytes in zip(GEOMS, want):
        back = host_map(q, 0)
        if nbytes == 0:
            assert back is None
            continue
        reg, info = back
        total = info["total"]
        assert total == nbytes, (q, total, nbytes)                       # the stand-alone build of the header agrees with the library
        assert info["base_end"] <= info["dense_end"] <= total
        # a pass's regions: every backward region with a length (a route uses a subset of them)
        _check_regions(reg, BACKWARD, total, "%s backward" % (q,))
        assert (reg["dense_col"][1] > 0) == bool(info["has_dense"]) and (reg["sw_wp"][1] > 0) == bool(info["has_sweep"])
        seen["dense"] += info["has_dense"]
        seen["sweep"] += info["has_sweep"]
        seen["plain"] += not (info["has_dense"] or info["has_sweep"])
        for which in (1, 2):
            freg, finfo = host_map(q, which)
            what = "%s forward %s" % (q, "fp32" if which == 1 else "split")
            assert all(freg[n] == reg[n] for n in BACKWARD[:13]), what      # the shared brackets are where the backward has them
            if finfo["fwd_dense"]:
                assert finfo["has_dense"]
                _check_regions(freg, ["dense_col", "dense_part"], total, what)
                seen["fwd_dense"] += 1
                continue
            tiled = (finfo["has_tile"] and freg["fwd_wl"][1] <= freg["wf"][1] and freg["fwd_wf9"][1] <= freg["wb"][1])
            if tiled:                                     # (and the caller's buffer reaches the far counter: it does, at `total`)
                used = ["fwd_wl", "fwd_wf9", "fwd_flags", "fwd_far_count"]
                seen["tile"] += 1
            elif q[5] * q[6] == 9 and q[3] >= 2 and freg["fwd_w9"][1] <= freg["wf"][1]:
                used = ["fwd_w9"]
            else:
                used = ["wf", "wb"]
            _check_regions(freg, used, total, what)
            for n in used:                                # what an overlay lies over is named above, nothing else
                if n in FORWARD_OVERLAYS:
                    over = {b for b in BACKWARD if _overlap(freg[n], freg[b])}
                    assert over <= FORWARD_OVERLAYS[n], (what, n, sorted(over))
    # the lists reach every bracket and every forward route under the environment that allows it
    if env.get("DCD_DCN_DENSE") != "0":
        assert seen["dense"] and seen["fwd_dense"]
    if env.get("DCD_BWD_SWEEP") != "0":
        assert seen["sweep"]
    assert seen["tile"] and seen["plain"]
