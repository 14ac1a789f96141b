"""The depth report's arithmetic (csrc/depth_report_math.h) compiled for the HOST (tests/host/host_depth_report.cpp: the two kernels
of csrc/depth_report.hip in plain loops): the estimates against the op-by-op chain's own helper functions on the candidates where
every clamp of the decode occurs, the chosen-among-four methods, the bin rule and the five stats against a float64 numpy
restatement, and the tables' independence of how the slots are cut into calls.  The GPU build of the same header is checked in
test_gpu_depth_report.py, which takes its helpers from here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_decode_host as DH  # noqa: E402
from test_decode_host import host_decode  # noqa: E402,F401  (the fixture: the host build of the decode, for method 7's bits)

HERE = os.path.dirname(os.path.abspath(__file__))
NM, ROW, STATS = 10, 13, 5
DIRECT, KPT_CENTER, KPT_02, KPT_13, SOFT, HARD, MEAN, EDGES, ORACLE, GMW = range(NM)
EDGES_SMALL = (0.0, 10.0, 30.0, 80.0)
NUM_CLASSES = 3
U = 2.0 ** -24                       # unit roundoff of float32


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_depth_report") / "libhost_depth_report.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "host", "host_depth_report.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _flat(t, dtype=np.float32):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a.reshape(-1).astype(dtype))


def host_estimates(lib, vectors, ys, xs, classes, gt_z, valid, table, spec, change_args=None):
    """`ops.depth_estimates` on host arrays through the host build: (status, est (B M, 13)); est starts as -7."""
    from dcd_amd import ops
    B, M, C = vectors.shape
    vec = np.ascontiguousarray(vectors.detach().cpu().float().numpy().reshape(B * M, C))
    a = ops.decode_args(spec, B, M, C)
    if change_args is not None:
        change_args(a)
    est = np.full((B * M, ROW), -7.0, np.float32)
    arrays = [vec, _flat(ys), _flat(xs), _flat(classes), _flat(gt_z), _flat(valid, np.uint8), _flat(table)]
    st = lib.host_depth_estimates(*[_p(x) for x in arrays], ctypes.byref(a), _p(est))
    return st, est


def host_accumulate(lib, est, edges, num_classes, tables=None):
    """`ops.depth_accumulate` through the host build, onto `tables` = (table, outside) or fresh zeros: (status, table, outside)."""
    n_bins = len(edges) - 1
    table, outside = tables if tables is not None else (np.zeros((num_classes, max(n_bins, 0), NM, STATS), np.float64),
                                                        np.zeros(num_classes, np.int64))
    est = np.ascontiguousarray(est, dtype=np.float32)
    e = np.asarray(edges, np.float32)
    st = lib.host_depth_accumulate(_p(est), int(est.shape[0]), _p(e), n_bins, num_classes, _p(table), _p(outside))
    return st, table, outside


def numpy_tables(est, edges, num_classes):
    """The float64 restatement of `dcd_depth_accumulate`: the rows of `est` walked in slot order, each booked into its (class,
    bin) cells -- the same sequence of double additions per cell as the build's, so the sums must come out bit-equal."""
    n_bins = len(edges) - 1
    edges = np.asarray(edges, np.float32)
    table, outside = np.zeros((num_classes, n_bins, NM, STATS), np.float64), np.zeros(num_classes, np.int64)
    for row in np.asarray(est, np.float32):
        if row[0] == 0:
            continue
        c, z = int(row[1]), row[2]
        inside = [i for i in range(n_bins) if np.isfinite(z) and edges[i] <= z < edges[i + 1]]
        if not inside:
            outside[c] += 1
            continue
        cell = table[c, inside[0]]
        for m in range(NM):
            d = row[3 + m]
            if not np.isfinite(d):
                cell[m, 4] += 1.0
                continue
            e = np.float64(d) - np.float64(z)
            cell[m, 0] += 1.0
            cell[m, 1] += abs(e)
            cell[m, 2] += e
            cell[m, 3] += e * e
    return table, outside


def numpy_oracle(d4, z):
    """The one of four estimates closest to z in float64, the first on a tie; a NaN distance is never chosen, d4[0] if all are."""
    pick, nearest = -1, 0.0
    for i in range(4):
        e = abs(np.float64(d4[i]) - np.float64(z))
        if e == e and (pick < 0 or e < nearest):
            pick, nearest = i, e
    return d4[max(pick, 0)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def slots_of(topk):
    """(ys, xs, classes) of the branch inputs' top-K, the cells the report is asked at."""
    return topk[3], topk[4], topk[2]


def chain_estimates(pp, vectors, topk, targets):
    """Methods 0-5 and 7 from the op-by-op chain's own functions on the branch candidates: {method: (n,) float64}, the chain's
    arg-max of 1 / sigma, and a finiteness check of every value on every slot."""
    enc, sl = pp.anno_encoder, pp.key2channel
    B, K, C = vectors.shape
    vec = vectors.reshape(B * K, C)
    image_of = torch.arange(B, device=vec.device).repeat_interleave(K)
    calibs = [t.get_field("calib") for t in targets]
    with torch.no_grad():
        direct = enc.decode_depth(vec[:, sl('depth')].squeeze(-1))
        dims = enc.decode_dimension(topk[2].reshape(-1), vec[:, sl('3d_dim')])
        f_u = enc._calib_table(calibs, vec.device)[image_of, 2]
        kd = enc.decode_depth_from_keypoints_batch(vec[:, sl('corner_offset')].view(-1, 10, 2), dims, calibs, f_u=f_u)
        dec = {"direct_depth": direct, "corner_depths": kd, "direct_sigma": vec[:, sl('depth_uncertainty')].exp(),
               "corner_sigma": vec[:, sl('corner_uncertainty')].exp()}
        vis = {}
        soft, _ = pp._fuse_depths(dec, vis)
        best = vis['min_uncertainty']
        four = torch.cat((direct.unsqueeze(1), kd), dim=1)
        hard = four.gather(1, best.view(-1, 1)).squeeze(1)
        rows, _, _ = DH.chain_on_candidates(pp, vectors, topk, targets)
    ref = {DIRECT: direct, KPT_CENTER: kd[:, 0], KPT_02: kd[:, 1], KPT_13: kd[:, 2], SOFT: soft, HARD: hard, EDGES: rows[:, 11]}
    ref = {m: v.detach().cpu().double().numpy() for m, v in ref.items()}
    assert all(v.shape == (B * K,) and np.isfinite(v).all() for v in ref.values()), "the chain is not finite on every slot"
    return ref, best.detach().cpu().numpy()


def compare_estimates(est, ref, best, what):
    """The bar of this header family (`DH.compare_with_chain`): 1e-4 of the column's largest magnitude in the chain's values; the
    `hard` column must be the build's own estimate at the CHAIN's arg-max, bit for bit."""
    for m, want in ref.items():
        err = np.abs(est[:, 3 + m].astype(np.float64) - want).max() / (np.abs(want).max() + 1e-6)
        print("%s, method %d: %.3e of the column's scale" % (what, m, err))
        assert err <= 1e-4, (m, err)
    assert same_bits(est[:, 3 + HARD], est[np.arange(len(est)), 3 + best])


def report_inputs(pp, device="cpu"):
    """The inputs of the second half of the tests: the branch candidates with seeded gt_z ~ U(-5, 95), one gt_z exactly on the
    edge 10 and one on the last edge 80, three empty slots, NaN in the whole vector of one empty slot and in the direct-depth
    channel of one valid slot.  Returns (vectors, ys, xs, classes, gt_z, valid, targets) and the planted slot numbers."""
    vectors, topk, targets = DH.branch_inputs(pp, device)
    ys, xs, classes = slots_of(topk)
    n = DH.BRANCH_B * DH.BRANCH_K
    rng = np.random.RandomState(7)
    gt_z = rng.uniform(-5, 95, n).astype(np.float32)
    planted = {"on_10": 4, "on_80": 21, "empty": (2, 17, 30), "nan_vector": 17, "nan_direct": 9}
    gt_z[planted["on_10"]], gt_z[planted["on_80"]], gt_z[planted["nan_direct"]] = 10.0, 80.0, 25.0
    valid = np.ones(n, np.uint8)
    valid[list(planted["empty"])] = 0
    vectors = vectors.clone()
    flat = vectors.view(n, -1)
    flat[planted["nan_vector"]] = float("nan")
    flat[planted["nan_direct"], pp.key2channel('depth').start] = float("nan")
    dev = vectors.device
    return (vectors, ys, xs, classes, torch.from_numpy(gt_z).to(dev), torch.from_numpy(valid).to(dev), targets), planted


def check_rows_against_numpy(est, gt_z, valid, classes, planted):
    """What does not depend on the libm: the leading columns, the empty rows, `mean` and `oracle` from the build's OWN four
    estimates."""
    gt_z, valid, classes = _flat(gt_z), _flat(valid, np.uint8), _flat(classes)
    on = valid != 0
    assert (est[~on] == 0).all() and same_bits(est[~on], np.zeros_like(est[~on])), "an empty slot's row is not all zeros"
    assert same_bits(est[on, 0], np.ones(on.sum(), np.float32)) and same_bits(est[on, 1], classes[on]) and same_bits(est[on, 2], gt_z[on])
    assert np.isnan(est[on, 3 + GMW]).all()
    d4 = est[:, 3:7]
    for s in np.nonzero(on)[0]:
        want = d4[s].astype(np.float64).sum() / 4.0
        got = est[s, 3 + MEAN]
        if np.isfinite(want):
            # ((d0 + d1) + d2 + d3) in float: three roundings, each at most U of a partial sum <= sum |d|; / 4 is exact
            assert abs(np.float64(got) - want) <= 3.01 * U * np.abs(d4[s].astype(np.float64)).sum() / 4.0, s
        else:
            assert not np.isfinite(got), s
        assert same_bits(est[s, 3 + ORACLE], np.float32(numpy_oracle(d4[s], gt_z[s]))), s
    bad = planted["nan_direct"]
    assert np.isnan(est[bad, 3 + DIRECT]) and np.isfinite(est[bad, 3 + KPT_CENTER:3 + KPT_13 + 1]).all()
    assert np.isfinite(est[bad, 3 + ORACLE])                              # the oracle never picks a NaN while a number stands


def check_tables(table, outside, est, edges, num_classes):
    """Counts, `outside` and the non-finite counts equal, the sums bit-equal to the numpy double sums in slot order."""
    want, want_out = numpy_tables(est, edges, num_classes)
    np.testing.assert_array_equal(outside, want_out)
    np.testing.assert_array_equal(table[..., 0], want[..., 0])
    np.testing.assert_array_equal(table[..., 4], want[..., 4])
    assert same_bits(table, want), "the sums are not the slot-order double sums"
    return want, want_out


# ------------------------------------------------------------------------------------------------------------------ tests
def test_host_build_against_the_op_by_op_chain(cpu_backend, host_report, host_decode):
    pp = DH.branch_post_processor("cpu")
    vectors, topk, targets = DH.branch_inputs(pp)
    ref, best = chain_estimates(pp, vectors, topk, targets)
    n = DH.BRANCH_B * DH.BRANCH_K
    assert len(best) == n == 32
    ys, xs, classes = slots_of(topk)
    st, est = host_estimates(host_report, vectors, ys, xs, classes, np.full(n, 20.0), np.ones(n), pp._image_table(targets, "cpu"),
                             pp.decode_spec())
    assert st == 0
    compare_estimates(est, ref, best, "host build")
    # method 7 is the decode's own reported depth: the same header function in the same lane order, so the same bits
    rows = DH.run_host(host_decode, vectors, topk, pp._image_table(targets, "cpu"), pp.decode_spec(), records=False)[0]
    assert same_bits(est[:, 3 + EDGES], rows[:, 11])


def test_host_build_against_the_numpy_restatement(cpu_backend, host_report):
    pp = DH.branch_post_processor("cpu")
    (vectors, ys, xs, classes, gt_z, valid, targets), planted = report_inputs(pp)
    st, est = host_estimates(host_report, vectors, ys, xs, classes, gt_z, valid, pp._image_table(targets, "cpu"), pp.decode_spec())
    assert st == 0
    check_rows_against_numpy(est, gt_z, valid, classes, planted)
    st, table, outside = host_accumulate(host_report, est, EDGES_SMALL, NUM_CLASSES)
    assert st == 0
    want, want_out = check_tables(table, outside, est, EDGES_SMALL, NUM_CLASSES)
    # the planted values went where the half-open rule sends them
    c10, c80 = int(est[planted["on_10"], 1]), int(est[planted["on_80"], 1])
    alone = np.zeros_like(est)
    alone[0] = est[planted["on_10"]]
    t10 = host_accumulate(host_report, alone[:1], EDGES_SMALL, NUM_CLASSES)[1]
    assert t10[c10, 1, KPT_CENTER, 0] == 1 and t10[c10, 0].sum() == 0, "gt_z = 10 belongs to [10, 30)"
    alone[0] = est[planted["on_80"]]
    _, t80, o80 = host_accumulate(host_report, alone[:1], EDGES_SMALL, NUM_CLASSES)
    assert o80[c80] == 1 and o80.sum() == 1 and not t80.any(), "gt_z = 80 is outside [0, 80) and booked nowhere else"
    n_valid = int(_flat(valid, np.uint8).sum())
    assert n_valid == 29
    for m in range(NM):                                                  # every object once per method: in a bin or outside
        assert table[:, :, m, 0].sum() + table[:, :, m, 4].sum() + outside.sum() == n_valid
    assert outside.sum() >= 2 and (table[..., GMW, 4].sum() == n_valid - outside.sum()) and table[..., GMW, :4].sum() == 0
    # the NaN of the direct head is counted in its own cells (gt_z = 25: bin 1) and the key-point methods of that object are booked
    bad = planted["nan_direct"]
    assert table[int(est[bad, 1]), 1, DIRECT, 4] >= 1 and want[int(est[bad, 1]), 1, KPT_CENTER, 0] >= 1


def test_tables_do_not_depend_on_the_batch_size(cpu_backend, host_report):
    pp = DH.branch_post_processor("cpu")
    (vectors, ys, xs, classes, gt_z, valid, targets), _ = report_inputs(pp)
    _, est = host_estimates(host_report, vectors, ys, xs, classes, gt_z, valid, pp._image_table(targets, "cpu"), pp.decode_spec())
    _, whole, whole_out = host_accumulate(host_report, est, EDGES_SMALL, NUM_CLASSES)
    for step in (16, 1):
        tables = None
        for s in range(0, len(est), step):
            st, t, o = host_accumulate(host_report, est[s:s + step], EDGES_SMALL, NUM_CLASSES, tables)
            assert st == 0
            tables = (t, o)
        assert same_bits(tables[0], whole) and same_bits(tables[1], whole_out), step
    assert whole[..., 0].sum() > 0


def test_oracle_takes_the_first_of_two_equally_near_estimates(cpu_backend, host_report):
    """A tie is planted from the build's own estimates: gt_z = (d_i + d_j) / 2 where that midpoint is a float32, d_i != d_j and
    the other two estimates lie farther away; both distances are then the same double, and the oracle must be d_i (i < j)."""
    pp = DH.branch_post_processor("cpu")
    vectors, topk, targets = DH.branch_inputs(pp)
    ys, xs, classes = slots_of(topk)
    n = DH.BRANCH_B * DH.BRANCH_K
    table, spec = pp._image_table(targets, "cpu"), pp.decode_spec()
    _, est = host_estimates(host_report, vectors, ys, xs, classes, np.zeros(n), np.ones(n), table, spec)
    gt_z, ties = np.full(n, 20.0, np.float32), {}
    for s in range(n):
        d = est[s, 3:7].astype(np.float64)
        for i in range(4):
            for j in range(i + 1, 4):
                mid = (d[i] + d[j]) / 2.0
                rest = [k for k in range(4) if k not in (i, j)]
                if (s not in ties and d[i] != d[j] and np.float64(np.float32(mid)) == mid
                        and all(abs(d[k] - mid) > abs(d[i] - mid) for k in rest)):
                    ties[s] = (i, j)
                    gt_z[s] = np.float32(mid)
    assert ties, "no slot offers an exactly representable midpoint"
    _, est = host_estimates(host_report, vectors, ys, xs, classes, gt_z, np.ones(n), table, spec)
    for s, (i, j) in ties.items():
        assert abs(np.float64(est[s, 3 + i]) - np.float64(gt_z[s])) == abs(np.float64(est[s, 3 + j]) - np.float64(gt_z[s]))
        assert same_bits(est[s, 3 + ORACLE], est[s, 3 + i]) and not same_bits(est[s, 3 + ORACLE], est[s, 3 + j]), (s, i, j)
    print("ties planted on %d slots" % len(ties))


def test_host_build_refuses_what_the_entry_points_refuse(cpu_backend, host_report):
    from dcd_amd import ops
    pp = DH.branch_post_processor("cpu")
    vectors, topk, targets = DH.branch_inputs(pp)
    ys, xs, classes = slots_of(topk)
    n = DH.BRANCH_B * DH.BRANCH_K
    args = (vectors, ys, xs, classes, np.zeros(n), np.ones(n), pp._image_table(targets, "cpu"))
    spec = pp.decode_spec()
    for bad in (dict(spec, nk=129), dict(spec, orientation=ops.DECODE_ORIENTATION["head-axis"])):
        st, est = host_estimates(host_report, *args, bad)
        assert st == 1 and (est == -7).all()
    st, est = host_estimates(host_report, *args, spec, change_args=lambda a: setattr(a, "K", 129))
    assert st == 1 and (est == -7).all()
    est = np.zeros((4, ROW), np.float32)
    for edges, classes_n in ((np.arange(18.0), 3), ((0.0, 10.0, 10.0), 3), ((0.0, 30.0, 20.0), 3), ((0.0, 10.0), 9), ((0.0, np.nan), 3)):
        st, table, outside = host_accumulate(host_report, est, edges, classes_n,
                                             (np.full((8, 16, NM, STATS), -7.0), np.full(9, -7, np.int64)))
        assert st == 1 and (table == -7).all() and (outside == -7).all(), edges
