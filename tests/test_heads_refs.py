"""tests/heads_refs.py on the host: the references that tests/test_gpu_heads_edges.py holds the kernels of csrc/heads.hip to, checked
against plain loops, the numpy oracle, torch and closed-form geometry.  A reference that is wrong would pass a wrong kernel; a bound
that an honest fp32 evaluation misses would fail a right one."""
import math

import numpy as np
import pytest
import torch

import heads_refs as R


# ---- gather / scatter -------------------------------------------------------------------------------------------------------
def _scatter_problem():
    g = torch.Generator().manual_seed(2)
    B, C, HW, M = 2, 3, 10, 9
    base = torch.randn(B, C, HW, generator=g)
    vals = torch.randn(B, M, C, generator=g)
    index = torch.tensor([[0, 3, 3, 9, -1, 10, 15, 3, 7], [5, 5, 5, 5, 5, 5, 5, 5, 5]])
    return base, vals, index


def test_scatter_ref_is_the_plain_loop_and_drops_what_is_out_of_range():
    base, vals, index = _scatter_problem()
    ref, n, S = R.scatter_ref(base, vals, index)
    want, cnt, mag = base.double().clone(), torch.zeros(2, 10, dtype=torch.int64), base.double().abs()
    for b in range(2):
        for m in range(9):
            i = int(index[b, m])
            if 0 <= i < 10:
                want[b, :, i] += vals[b, m].double()
                mag[b, :, i] += vals[b, m].double().abs()
                cnt[b, i] += 1
    assert torch.equal(ref, want) and torch.equal(n, cnt) and torch.allclose(S, mag, rtol=1e-15, atol=0)
    assert n[0].tolist() == [1, 0, 0, 3, 0, 0, 0, 1, 0, 1] and n[1].tolist() == [0, 0, 0, 0, 0, 9, 0, 0, 0, 0]
    # an fp32 sum in list order meets the bound, an fp32 sum with one term dropped or doubled does not
    got = base.clone()
    for b in range(2):
        for m in range(9):
            if 0 <= int(index[b, m]) < 10:
                got[b, :, index[b, m]] += vals[b, m]
    assert R.assert_scatter(got, base, ref, n, S, "host fp32") <= 1.0
    dropped = got.clone()
    dropped[1, :, 5] -= vals[1, 8]
    with pytest.raises(AssertionError):
        R.assert_scatter(dropped, base, ref, n, S, "one term dropped")
    touched = got.clone()
    touched[0, 1, 2] = torch.nextafter(touched[0, 1, 2], torch.tensor(9.0))
    with pytest.raises(AssertionError):
        R.assert_scatter(touched, base, ref, n, S, "one ulp in a cell that no index names")


def test_gather_ref_returns_zero_out_of_range():
    base, _, index = _scatter_problem()
    got = R.gather_ref(base, index)
    for b in range(2):
        for m in range(9):
            i = int(index[b, m])
            want = base[b, :, i].double() if 0 <= i < 10 else torch.zeros(3, dtype=torch.float64)
            assert torch.equal(got[b, m], want)


def test_patch_scatter_ref_is_the_plain_loop_tap_by_tap():
    g0 = torch.Generator().manual_seed(3)
    B, C, M, pitch, L = 2, 2, 5, 6, 30
    base = torch.randn(B, C, L, generator=g0)
    g = torch.randn(B, C * 9, M, generator=g0)
    first = torch.tensor([[0, 1, 1, 15, 22], [7, 7, 7, -3, 40]])       # neighbours, identical windows, windows past both ends
    ref, n, S = R.patch_scatter_ref(base, g, first, pitch)
    want, cnt = base.double().clone(), torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        for m in range(M):
            for t in range(9):
                i = int(first[b, m]) + (t // 3) * pitch + t % 3
                if 0 <= i < L:
                    cnt[b, i] += 1
                    for c in range(C):
                        want[b, c, i] += g[b, c * 9 + t, m].double()
    assert torch.allclose(ref, want, rtol=1e-15, atol=0) and torch.equal(n, cnt)
    # base 22: rows 22..24 and 28..29, the tap at 30 and the third row are past the plane; base -3: only the taps at 3, 4, 5, 9, 10,
    # 11 lie inside; base 40: none
    assert n[0, 28] == 2 and n[0, 29] == 2 and n[0].sum() == 4 * 9 + 5 and n[1].sum() == 3 * 9 + 6
    assert (S >= ref.abs() - 1e-12).all()


# ---- top-K ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,K", [(2, 1, 96, 320, 50), (16, 1, 96, 320, 50), (2, 3, 24, 40, 50), (1, 1, 8, 8, 50),
                                      (3, 1, 96, 320, 100)])
def test_topk_ref_against_the_oracle_and_torch(B, C, H, W, K):
    """On the inputs of test_gpu_heads.py::test_heatmap_decode_exact: every output equal to oracle.heads_oracle.select_topk (a
    lexsort on (index, -value)), and the scores equal to torch.topk's values (whose tie ORDER is unspecified, the values are not)."""
    from oracle import heads_oracle as ho
    rng = np.random.RandomState(B * 7 + C)
    heat = np.clip(1 / (1 + np.exp(-rng.normal(-2, 1.5, (B, C, H, W)))), 1e-4, 1 - 1e-4).astype(np.float32)
    heat[:, :, 3:5, 3:6] = 0.77
    heat[:, :, H - 1, W - 1] = 0.9
    heat[:, :, 0, 0] = 0.9
    for hm in (heat, ho.nms_hm(heat)):
        got, ref = R.topk_ref(hm, K), ho.select_topk(hm, K)
        for g_, r_, nm in zip(got, ref, ("scores", "inds", "clses", "ys", "xs")):
            assert g_.dtype == r_.dtype and np.array_equal(g_, r_), nm
        t = torch.from_numpy(hm).view(B, C, -1)
        per_class = torch.topk(t, K).values.reshape(B, C * K)
        assert np.array_equal(got[0], torch.topk(per_class, K).values.numpy())
    assert np.array_equal(R.nms_ref(heat), ho.nms_hm(heat))


def test_topk_ref_treats_the_two_zeros_as_equal():
    heat = np.full((1, 1, 2, 6), -1.0, np.float32)
    heat[0, 0, 0] = [0.5, -0.0, 0.0, -0.0, 0.0, -0.0]
    scores, inds, clses, ys, xs = R.topk_ref(heat, 4)
    assert inds.tolist() == [[0, 1, 2, 3]] and scores[0, 0] == 0.5 and (scores[0, 1:] == 0).all()
    assert np.signbit(scores[0, 1]) and not np.signbit(scores[0, 2])          # the values are the map's own
    assert clses.tolist() == [[0.0, 0.25, 0.5, 0.75]] and ys.tolist() == [[0.0] * 4] and xs.tolist() == [[0.0, 1.0, 2.0, 3.0]]
    neg = -np.abs(np.random.RandomState(0).normal(size=(1, 2, 3, 5))).astype(np.float32)
    neg[0, 1, 1, 1] = neg[0, 0, 2, 2] = -0.25                                  # equal scores in two classes: class 0 first
    got = R.topk_ref(neg, 3)
    assert (got[0] <= 0).all() and (np.diff(got[0][0]) <= 0).all()
    e = (got[2][0] * 3).round().astype(int).tolist()
    both = [i for i, s in enumerate(got[0][0]) if s == np.float32(-0.25)]
    assert len(both) in (0, 2) and (not both or e[both[0]] < 3 <= e[both[1]])


# ---- IoU-3D -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc():
    import test_host_golden as H
    from dcd_amd.model.anno_encoder import Anno_Encoder
    return Anno_Encoder(H.small_cfg("cpu"))


def test_rect_iou3d_and_the_scene_table():
    assert R.rect_iou3d((0, 2, 0, 1, 0, 4), (1, 3, 0, 1, 0, 4)) == 4.0 / 12.0
    assert R.rect_iou3d((0, 2, 0, 1, 0, 4), (2, 3, 0, 1, 0, 4)) == 0.0
    names = [s["name"] for s in R.iou3d_scenes()]
    for need in ("identical", "disjoint", "shared edge", "shared corner", "inside", "quarter turn", "crossed bars", "octagon",
                 "half height", "no common height"):
        assert need in names
    by = {s["name"]: s for s in R.iou3d_scenes()}
    assert by["shifted"]["expected"] == (3.0 * 1.5 * 1.5) / (2 * 12.0 - 3.0 * 1.5 * 1.5)
    assert by["quarter turn, shifted"]["expected"] == rect_ratio(2.0, 2.0, 1.5, 12.0)      # x in [0, 2] of [-1.5, 2.5], z in [0, 2] of [-0.5, 3.5]


def rect_ratio(ox, oz, h, vol):
    inter = ox * oz * h
    return inter / (2 * vol - inter)


def test_corners64_is_what_encode_box3d_rounds(enc):
    a, b = R.random_pairs(40.0, 16, seed=1)
    c32, c64 = R.encode(enc, a + b).double().numpy(), R.corners64(a + b)
    assert np.abs(c32 - c64).max() <= 3 * 2.0 ** -24 * 64              # sin / cos, two products, two sums below 64 m


@pytest.mark.parametrize("where", ["origin", "moved"])
def test_the_oracle_iou3d_gives_the_closed_forms(enc, where):
    """`oracle/torch_ops.iou_3d` on the corners that `encode_box3d` gives, against answers that need no clipping.  Near the origin
    the corners are exact and so are the zeros; turned by 0.7 rad and moved to (20, 60) the corners are rounded to fp32, and the
    answer holds within what that rounding can do (`corner_rounding_bound` on the measured distance to the float64 corners).  On
    the float64 corners themselves the moved scene gives the value of the unmoved one: the rigid-motion property."""
    from oracle import torch_ops
    scenes = R.iou3d_scenes()
    A, B = [s["a"] for s in scenes], [s["b"] for s in scenes]
    if where == "moved":
        A, B = [R.moved(x, 0.7, 20.0, 60.0) for x in A], [R.moved(x, 0.7, 20.0, 60.0) for x in B]
    a, b = R.encode(enc, A), R.encode(enc, B)
    got = R.oracle_iou3d(a, b)
    assert torch.equal(got.float(), torch_ops.iou_3d(a, b))
    delta = max(np.abs(a.double().numpy() - R.corners64(A)).max(), np.abs(b.double().numpy() - R.corners64(B)).max())
    assert delta <= 3 * 2.0 ** -24 * (4 if where == "origin" else 64)     # only the octagon's corners are not dyadic at the origin
    exact = R.oracle_iou3d(torch.from_numpy(R.corners64(A)), torch.from_numpy(R.corners64(B)))
    for i, s in enumerate(scenes):
        # float64 corners: only the 1e-16 roundings of sin / cos and of the clip itself are left
        assert abs(exact[i].item() - s["expected"]) <= 1e-12, (s["name"], exact[i].item(), s["expected"])
        tol = R.corner_rounding_bound(A[i], B[i], delta) + 1e-12
        assert abs(got[i].item() - s["expected"]) <= tol, (s["name"], got[i].item(), s["expected"], tol)
        if s["zero"] and where == "origin":
            assert got[i].item() == 0.0, s["name"]
    # the target's bottom corners in reverse order (the clip's sign rule turns over): the same value
    rev = b.clone()
    rev[:, 0:4] = b[:, [3, 2, 1, 0]]
    assert (R.oracle_iou3d(a, rev) - got).abs().max().item() <= 1e-12


def test_the_fp32_yardstick_is_accurate_in_the_local_frame_only(enc):
    """`iou3d_fp32` on the random pairs of the device test: translated by the target's corner 0 it stays within a few 2^-24 of
    float64 at every depth; on absolute camera coordinates it loses more than ten times that from 40 m on -- the defect that the
    kernel had, and the reason the yardstick is the local form."""
    worst = {}
    for z in (5.0, 80.0):
        A, B = R.random_pairs(z, 64, seed=int(z))
        a, b = R.encode(enc, A), R.encode(enc, B)
        ref = R.oracle_iou3d(a, b).numpy()
        assert (ref > 0.05).sum() >= 32
        worst[z] = [np.abs(R.iou3d_fp32(a.numpy(), b.numpy(), local=loc).astype(np.float64) - ref).max() for loc in (True, False)]
    print("iou3d_fp32 worst |error|  (local, absolute):", worst)
    assert worst[5.0][0] <= 16 * R.U and worst[80.0][0] <= 16 * R.U
    assert worst[80.0][1] >= 10 * worst[80.0][0] and worst[80.0][1] >= 5e-6


# ---- focal loss -------------------------------------------------------------------------------------------------------------
# The oracle clamps the prediction in fp32 as the reference does, focal_ref in float64: the one cell with pred = 0 sits at
# fp32(1e-10) = 1e-10 (1 + 3.6e-9) there, and its loss -log(p) (1 - p)^alpha differs by 3.6e-9 -- a property of the two clamps.
CLAMP_SLACK = 2e-8
@pytest.mark.parametrize("shape", R.FOCAL_SHAPES)
def test_focal_ref_at_the_reference_exponents_is_the_existing_reference(shape):
    import test_gpu_heads as TH
    from oracle import heads_oracle as ho
    pred, tgt, _, _ = TH.focal_inputs(shape)
    loss, npos, g, bound = R.focal_ref(pred, tgt, 2, 4)
    g0, bound0 = TH.focal_gradient_reference(pred, tgt)
    assert torch.equal(g, g0) and torch.equal(bound, bound0)
    ref_loss, ref_np = ho.focal_loss(pred, tgt)
    assert npos == ref_np and abs(loss - ref_loss) <= CLAMP_SLACK + 1e-12 * abs(ref_loss)


@pytest.mark.parametrize("alpha,beta", R.FOCAL_EXPONENTS)
def test_focal_ref_at_other_exponents_and_targets(alpha, beta):
    from oracle import heads_oracle as ho
    pred, tgt, outside, mz = R.focal_inputs((2, 24, 80))
    loss, npos, g, bound = R.focal_ref(pred, tgt, alpha, beta)
    assert math.isfinite(loss) and torch.isfinite(g).all() and torch.isfinite(bound).all()
    for cell in outside:
        assert g[cell] == 0 and bound[cell] == 0
    assert npos == float((tgt == 1).sum())
    plain = tgt.copy()
    plain[mz] = 0.0
    l2, _, g2, _ = R.focal_ref(pred, plain, alpha, beta)
    assert l2 == loss and torch.equal(g, g2) and g[mz] != 0                 # -0.0 is a plain zero
    for cell in outside:                                                    # ... and the loss is the oracle's without the two cells
        plain[cell] = 0.0
    keep = np.ones(tgt.shape, bool)
    for cell in outside:
        keep[cell] = False
    ref_loss, _ = ho.focal_loss(pred[keep], plain[keep], alpha, beta)
    assert abs(loss - ref_loss) <= CLAMP_SLACK + 1e-12 * abs(ref_loss)
    assert R.focal_ref(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), alpha, beta)[:2] == (0.0, 0.0)


def test_the_powf_tolerance_is_four_times_the_host_fp32_error():
    """FOCAL_POW_RTOL = 4 x what the formula in fp32 torch on the CPU needs against float64 at the non-integer exponents, on the
    inputs of the device test.  The host's `pow` may differ by a unit in the last place from one build of torch to the next, so
    the measurement is held to the constant with a factor of two to spare, not to its digits."""
    import test_gpu_heads as TH
    measured = max(R.focal_fp32_rtol(*R.focal_inputs(shape)[:2], 1.5, 2.5) for shape in R.FOCAL_SHAPES)
    print("focal, (alpha, beta) = (1.5, 2.5): host fp32 needs rtol %.3e; FOCAL_POW_RTOL = %.3e" % (measured, R.FOCAL_POW_RTOL))
    assert R.FOCAL_POW_RTOL / 8 <= measured <= R.FOCAL_POW_RTOL / 2
    assert R.FOCAL_POW_RTOL >= TH.FOCAL_RTOL / 4
