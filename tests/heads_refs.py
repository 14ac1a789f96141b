"""References and derived bounds for the oldest kernels of csrc/heads.hip: POI gather / scatter and the patch scatter, the heat-map
top-K, the focal loss at any exponents and the 3-D IoU.  TEST INFRASTRUCTURE, numpy / torch on the CPU in float64.

None of them shares the construction of the kernel it judges:

  scatter   `index_add_` in float64 with out-of-range indices dropped.  With every destination cell come n, the number of terms
            added to it, and S = |base| + sum |terms|: an fp32 sum of base and n terms rounds n times whatever the order, so
            |got - ref| <= n 2^-24 S to first order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) -- the
            bound holds for atomics in any order and is derived, not measured.  n = 0: the cell must keep the bits of its pre-fill.
  top-K     a stable sort of the negated values per class (value descending, linear index ascending, +0.0 == -0.0), then the
            same rule over the C * K survivors; no radix select, no candidate lists.
  IoU-3D    closed-form answers: axis-aligned boxes by interval arithmetic, crossed bars, the octagon of two squares at 45
            degrees, and the rigid-motion property (turn and move both boxes together: the same value).  No polygon clipping.
            `oracle/torch_ops.iou_3d` -- the same Sutherland-Hodgman construction as the kernel -- is held to these in
            tests/test_heads_refs.py, and only then used for random pairs.
  focal     `focal_formula` / `focal_gradient_reference` of tests/test_gpu_heads.py restated for any (alpha, beta).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 8 * U                      # the floor of the max(4 E_ref, 8 * 2^-24) bars (tests/test_gpu_gmw_refine.py)


# ---- gather / scatter -------------------------------------------------------------------------------------------------------
def gather_ref(feat, index):
    """feat (B, C, HW), index (B, M) int64 -> (B, M, C) float64: feat[b, :, index[b, m]], exactly 0 where the index is outside
    [0, HW)."""
    B, C, HW = feat.shape
    ok = (index >= 0) & (index < HW)
    rows = feat.double().permute(0, 2, 1).gather(1, index.clamp(0, HW - 1)[:, :, None].expand(B, index.shape[1], C))
    return rows * ok[:, :, None]


def _index_add(base, cell, terms):
    """base (B, C, L); cell (B, T) int64, terms (B, C, T): out[b, c, cell[b, t]] += terms[b, c, t] for the cells inside [0, L).
    Returns (out, n, S): float64 sums, n (B, L) terms per cell, S (B, C, L) = |base| + sum |terms|."""
    B, C, L = base.shape
    out, S = base.double().clone(), base.double().abs()
    n = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ok = (cell[b] >= 0) & (cell[b] < L)
        at, t = cell[b][ok], terms[b].double()[:, ok]
        out[b].index_add_(1, at, t)
        S[b].index_add_(1, at, t.abs())
        n[b].index_add_(0, at, torch.ones_like(at))
    return out, n, S


def scatter_ref(base, vals, index):
    """The sum `dcd_poi_scatter_add` forms: base (B, C, HW) fp32 pre-fill, vals (B, M, C), index (B, M) -> (out, n, S)."""
    return _index_add(base, index, vals.permute(0, 2, 1))


def patch_scatter_ref(base, g, first, pitch):
    """`dcd_patch_scatter_add`: out[b, c, first[b, m] + (t // 3) * pitch + t % 3] += g[b, c * 9 + t, m] on base (B, C, L), tap by
    tap: a tap outside [0, L) is dropped, the others of its window stay."""
    B, C, L = base.shape
    M = first.shape[1]
    t = torch.arange(9)
    cell = (first[:, None, :] + ((t // 3) * pitch + t % 3)[None, :, None]).reshape(B, 9 * M)
    return _index_add(base, cell, g.reshape(B, C, 9 * M))


def assert_scatter(got, base, ref, n, S, what):
    """|got - ref| <= n 2^-24 S cell by cell, and the bits of the pre-fill where nothing was added.  Returns the worst ratio."""
    got, base = got.detach().cpu(), base.detach().cpu()
    assert got.shape == ref.shape == base.shape, (what, tuple(got.shape), tuple(ref.shape))
    hit = (n > 0)[:, None, :].expand_as(ref)
    assert torch.equal(got[~hit].view(torch.int32), base[~hit].view(torch.int32)), "%s: a cell that no index names changed" % what
    allowed = n[:, None, :].double() * U * S
    err = (got.double() - ref).abs()
    bad = err > allowed
    assert not bad.any(), "%s: %d cells over n 2^-24 S, first at %s: |got - ref| %.3e, allowed %.3e" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), err[bad][0].item(), allowed[bad][0].item())
    return (err[hit] / allowed[hit].clamp_min(1e-300)).max().item() if hit.any() else 0.0


# ---- top-K ------------------------------------------------------------------------------------------------------------------
def nms_ref(heat):
    """heat * (maxpool3x3(heat) == heat) in heat's own dtype: a negative non-maximum becomes -0.0, as in the reference."""
    B, C, H, W = heat.shape
    pad = np.full((B, C, H + 2, W + 2), -np.inf, heat.dtype)
    pad[:, :, 1:-1, 1:-1] = heat
    mx = np.max([pad[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
    return heat * (mx == heat).astype(heat.dtype)


def topk_ref(heat, K):
    """(scores, inds, clses, ys, xs), each (B, K), of select_topk on heat (B, C, H, W) fp32: per class the K largest by (value
    descending, linear index ascending), then the K largest of the C * K by (value descending, position e in the class-major list
    ascending); clses = e / K in fp32 true division, ys = ind // W, xs = ind % W as fp32.  +0.0 and -0.0 are equal."""
    B, C, H, W = heat.shape
    flat = np.ascontiguousarray(heat, np.float32).reshape(B, C, H * W)
    per = np.argsort(-flat, axis=2, kind="stable")[:, :, :K]                     # a stable sort: equal values keep index order
    sc = np.take_along_axis(flat, per, 2).reshape(B, C * K)
    e = np.argsort(-sc, axis=1, kind="stable")[:, :K]
    inds = np.take_along_axis(per.reshape(B, C * K), e, 1).astype(np.int64)
    return (np.take_along_axis(sc, e, 1), inds, e.astype(np.float32) / np.float32(K), (inds // W).astype(np.float32),
            (inds % W).astype(np.float32))


# ---- IoU-3D: closed forms ---------------------------------------------------------------------------------------------------
def rect_iou3d(a, b):
    """3-D IoU of two AXIS-ALIGNED boxes by interval arithmetic; a box is (x0, x1, y0, y1, z0, z1)."""
    inter, vol = 1.0, [1.0, 1.0]
    for k in range(3):
        inter *= max(0.0, min(a[2 * k + 1], b[2 * k + 1]) - max(a[2 * k], b[2 * k]))
        vol[0] *= a[2 * k + 1] - a[2 * k]
        vol[1] *= b[2 * k + 1] - b[2 * k]
    return inter / (vol[0] + vol[1] - inter)


def _aligned(ry, dims, loc):
    """The intervals of a box (ry a multiple of a quarter turn; dims = (l, h, w), loc = the centre)."""
    l, h, w = dims
    q = int(round(ry / (math.pi / 2)))
    assert abs(ry - q * math.pi / 2) < 1e-12
    ex, ez = (l, w) if q % 2 == 0 else (w, l)
    return (loc[0] - ex / 2, loc[0] + ex / 2, loc[1] - h / 2, loc[1] + h / 2, loc[2] - ez / 2, loc[2] + ez / 2)


def _scene(name, a, b, expected=None, zero=False):
    if expected is None:
        expected = rect_iou3d(_aligned(*a), _aligned(*b))
    assert (expected == 0.0) == zero, name
    return dict(name=name, a=a, b=b, expected=expected, zero=zero)


def iou3d_scenes():
    """Known answers near the origin; a box is (ry, (l, h, w), (x, y, z)) as `Anno_Encoder.encode_box3d` takes it (loc = centre).
    But for the turned boxes (quarter turn, octagon) every coordinate of every corner is a small dyadic number, so the fp32 corners
    are exact; every scene with `zero` is of that kind, and `zero` means exactly 0."""
    car, Q = (4.0, 1.5, 2.0), math.pi / 2
    o = (0.5, 1.0, 1.0)
    bar, sq = (6.0, 2.0, 2.0), (1.0, 1.0, 1.0)
    octagon = 2.0 * (math.sqrt(2.0) - 1.0)              # two unit squares at 45 degrees about one centre: 8 vertices
    return [
        _scene("identical", (0.0, car, o), (0.0, car, o), expected=1.0),
        _scene("disjoint", (0.0, car, o), (0.0, car, (0.5, 1.0, 4.0)), zero=True),
        _scene("shared edge", (0.0, car, o), (0.0, car, (4.5, 1.0, 1.0)), zero=True),
        _scene("shared corner", (0.0, car, o), (0.0, car, (4.5, 1.0, 3.0)), zero=True),
        _scene("shifted", (0.0, car, o), (0.0, car, (1.5, 1.0, 1.5))),
        _scene("inside", (0.0, (2.0, 1.0, 1.0), (0.75, 1.0, 1.25)), (0.0, car, o), expected=2.0 / 12.0),
        _scene("outside", (0.0, car, o), (0.0, (2.0, 1.0, 1.0), (0.75, 1.0, 1.25)), expected=2.0 / 12.0),
        # the footprint l x w turned a quarter is the footprint w x l: the axis-aligned answer
        _scene("quarter turn", (Q, car, o), (0.0, (2.0, 1.5, 4.0), o), expected=1.0),
        _scene("quarter turn, shifted", (Q, car, (1.0, 1.0, 1.5)), (0.0, car, o)),
        _scene("crossed bars", (0.0, bar, o), (Q, bar, o), expected=8.0 / (24.0 + 24.0 - 8.0)),
        _scene("octagon", (0.0, sq, o), (math.pi / 4, sq, o), expected=octagon / (2.0 - octagon)),
        _scene("half height", (0.0, car, o), (0.0, car, (0.5, 1.75, 1.0)), expected=1.0 / 3.0),
        _scene("no common height", (0.0, car, o), (0.0, car, (0.5, 2.5, 1.0)), zero=True),
        _scene("one above the other, touching", (0.0, car, o), (0.0, car, (0.5, 3.0, 1.0)), zero=True),
    ]


def moved(box, angle, dx, dz):
    """The box turned by `angle` about the camera's y axis through the origin, then moved by (dx, dz): applied to both boxes of a
    scene it leaves the IoU unchanged.  The turn is `Anno_Encoder.rad_to_matrix`: x' = x cos + z sin, z' = -x sin + z cos."""
    ry, dims, (x, y, z) = box
    c, s = math.cos(angle), math.sin(angle)
    return (ry + angle, dims, (x * c + z * s + dx, y, -x * s + z * c + dz))


def corners64(boxes):
    """(N, 8, 3) float64 corners of boxes (ry, (l, h, w), centre), restated from anno_encoder.py:93-128 -- what
    `Anno_Encoder.encode_box3d` rounds to fp32."""
    sx, sy, sz = (-1, -1, 1, 1, -1, -1, 1, 1), (1, 1, 1, 1, -1, -1, -1, -1), (-1, 1, 1, -1, -1, 1, 1, -1)
    out = np.empty((len(boxes), 8, 3))
    for i, (ry, (l, h, w), (x, y, z)) in enumerate(boxes):
        c, s = math.cos(ry), math.sin(ry)
        for k in range(8):
            px, py, pz = sx[k] * l / 2, sy[k] * h / 2, sz[k] * w / 2
            out[i, k] = (c * px + s * pz + x, py + y, -s * px + c * pz + z)
    return out


def encode(enc, boxes):
    """(N, 8, 3) fp32 corners from `Anno_Encoder.encode_box3d`, as the loss builds them."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    return enc.encode_box3d(f([b[0] for b in boxes]), f([b[1] for b in boxes]), f([b[2] for b in boxes])).contiguous()


def corner_rounding_bound(a, b, delta):
    """What moving every corner coordinate of both boxes by at most `delta` can do to their IoU, to first order.
    The symmetric difference of a footprint and its moved copy lies in a strip of width sqrt(2) delta along its perimeter P, so
    its area changes by at most sqrt(2) delta P, and the overlap of the two footprints by at most the sum of both strips; a height
    (a difference of two means of y) by at most 2 delta.  With V = area x height for the boxes and I for the overlap
    (area_I <= min area, h_I <= min h):  dV <= sqrt(2) delta P h + 2 delta area,  dI <= sqrt(2) delta (P_a + P_b) h_I + 2 delta
    area_I, and IoU = I / (V_a + V_b - I) moves by at most (2 dI + dV_a + dV_b) / union  (I <= union)."""
    r2 = math.sqrt(2.0)
    (la, ha, wa), (lb, hb, wb) = a[1], b[1]
    Pa, Pb, Aa, Ab = 2 * (la + wa), 2 * (lb + wb), la * wa, lb * wb
    dVa, dVb = r2 * delta * Pa * ha + 2 * delta * Aa, r2 * delta * Pb * hb + 2 * delta * Ab
    dI = r2 * delta * (Pa + Pb) * min(ha, hb) + 2 * delta * min(Aa, Ab)
    union_min = max(Aa * ha, Ab * hb)                  # the union holds the larger box
    return (2 * dI + dVa + dVb) / union_min


def oracle_iou3d(a, b):
    """`oracle/torch_ops.iou_3d` without its final rounding to fp32: the same statements on its own helpers, float64 out."""
    from oracle import torch_ops as TO
    A, B = a.detach().double().cpu(), b.detach().double().cpu()
    out = torch.zeros(A.shape[0], dtype=torch.float64)
    for i in range(A.shape[0]):
        lo_a, hi_a, lo_b, hi_b = -A[i, 0:4, 1].sum() / 4.0, -A[i, 4:8, 1].sum() / 4.0, -B[i, 0:4, 1].sum() / 4.0, -B[i, 4:8, 1].sum() / 4.0
        h = torch.clamp(torch.min(hi_a, hi_b) - torch.max(lo_a, lo_b), min=0)
        pa, pb = A[i, 0:4][:, [0, 2]], B[i, 0:4][:, [0, 2]]
        inter = TO._clip_convex(pa, pb)
        o3 = (TO._poly_area(inter) if inter.shape[0] >= 3 else torch.zeros((), dtype=torch.float64)) * h
        out[i] = o3 / (TO._poly_area(pa) * (hi_a - lo_a) + TO._poly_area(pb) * (hi_b - lo_b) - o3)
    return out


def iou3d_fp32(a, b, local=True):
    """The formula of `iou3d_kernel` with every operation rounded to fp32 (numpy scalars; no fused multiply-add), on footprints
    translated by the target's corner 0 (`local`) or as given.  local=True is the yardstick E_ref of the accuracy tests: what an
    honest fp32 evaluation of the formula in a local frame loses against float64."""
    f = np.float32
    A, B = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.zeros(A.shape[0], np.float32)

    def area(px, py):
        s = f(0)
        for i in range(len(px)):
            j = (i + 1) % len(px)
            s = f(s + f(f(px[i] * py[j]) - f(px[j] * py[i])))
        return f(f(0.5) * abs(s))

    for n in range(A.shape[0]):
        ox, oz = (B[n, 0, 0], B[n, 0, 2]) if local else (f(0), f(0))
        ax, az, bx, bz = A[n, :4, 0] - ox, A[n, :4, 2] - oz, B[n, :4, 0] - ox, B[n, :4, 2] - oz
        lo_a, hi_a, lo_b, hi_b = (f(-f(0.25) * v.sum(dtype=np.float32)) for v in (A[n, :4, 1], A[n, 4:, 1], B[n, :4, 1], B[n, 4:, 1]))
        h = max(f(0), f(min(hi_a, hi_b) - max(lo_a, lo_b)))
        orient = f(0)
        for k in range(4):
            j = (k + 1) % 4
            orient = f(orient + f(f(bx[k] * bz[j]) - f(bx[j] * bz[k])))
        sgn = f(1) if orient >= 0 else f(-1)
        px, py = list(ax), list(az)
        for e in range(4):
            if not px:
                break
            e2 = (e + 1) % 4
            ex, ez = f(bx[e2] - bx[e]), f(bz[e2] - bz[e])
            side = [f(sgn * f(f(ex * f(py[k] - bz[e])) - f(ez * f(px[k] - bx[e])))) for k in range(len(px))]
            qx, qy = [], []
            for k in range(len(px)):
                j = (k + 1) % len(px)
                if side[k] >= 0:
                    qx.append(px[k]), qy.append(py[k])
                if (side[k] >= 0) != (side[j] >= 0):
                    t = f(side[k] / f(side[k] - side[j]))
                    qx.append(f(px[k] + f(t * f(px[j] - px[k])))), qy.append(f(py[k] + f(t * f(py[j] - py[k]))))
            px, py = qx, qy
        o3 = f((area(px, py) if len(px) >= 3 else f(0)) * h)
        uni = f(f(f(area(ax, az) * f(hi_a - lo_a)) + f(area(bx, bz) * f(hi_b - lo_b))) - o3)
        out[n] = f(o3 / uni)
    return out


def random_pairs(depth, n, seed):
    """n car-sized box pairs at depth z: the second box is the first moved by N(0, 0.6 m) in x, y (a quarter of it) and z and
    turned by N(0, 0.3 rad), its dimensions 1.1 times the first's (the generator behind the figures of the kernel's comment)."""
    rng = np.random.RandomState(seed)
    a, b = [], []
    for _ in range(n):
        dims = tuple(np.abs(rng.normal([3.9, 1.5, 1.6], 0.2)))
        ry = rng.uniform(-math.pi, math.pi)
        loc = (rng.uniform(-0.3, 0.3) * depth, rng.uniform(0.8, 1.8), depth + rng.uniform(-1.0, 1.0))
        d = rng.normal(0, 0.6, 3)
        a.append((ry + rng.normal(0, 0.3), tuple(1.1 * v for v in dims), (loc[0] + d[0], loc[1] + 0.25 * d[1], loc[2] + d[2])))
        b.append((ry, dims, loc))
    return a, b


# ---- focal loss -------------------------------------------------------------------------------------------------------------
def focal_formula(p, tt, alpha, beta, q_neg=None, q_pos=None):
    """`focal_formula` of tests/test_gpu_heads.py for any exponents: the penalty-reduced focal loss per element
    (focal_loss.py:57-86) in p's dtype; a target outside [0, 1] contributes nothing.  q_neg / q_pos stand in for the logarithms'
    arguments."""
    pc = p.clamp(1e-10, 1 - 1e-10)
    qn = 1 - pc if q_neg is None else q_neg
    qp = pc if q_pos is None else q_pos
    zero = torch.zeros_like(pc)
    pos = torch.where(tt == 1, -(torch.log(qp) * (1 - qp) ** alpha), zero)
    neg = torch.where((tt < 1) & (tt >= 0), -torch.log(qn) * pc ** alpha * (1 - tt).clamp_min(0) ** beta, zero)
    return pos + neg, qn, qp


def focal_ref(pred, target, alpha, beta):
    """(loss, positives, g, bound) in float64 from fp32 arrays: the loss sum, the count of target == 1, g = d loss / d pred by
    autograd, and bound = 2^-24 |q dg/dq| -- what ONE fp32 rounding of a logarithm's argument does to g
    (`focal_gradient_reference` of tests/test_gpu_heads.py, any exponents)."""
    tt = torch.as_tensor(target).double()
    p = torch.as_tensor(pred).double().requires_grad_()
    loss = focal_formula(p, tt, alpha, beta)[0].sum()
    if p.numel() == 0:
        return 0.0, 0.0, torch.zeros_like(tt), torch.zeros_like(tt)
    g = torch.autograd.grad(loss, p)[0]
    pc = p.detach().clamp(1e-10, 1 - 1e-10)
    qn, qp = (1 - pc).requires_grad_(), pc.clone().requires_grad_()
    l, _, _ = focal_formula(p, tt, alpha, beta, qn, qp)
    gp, gn, gq = torch.autograd.grad(l.sum(), (p, qn, qp), create_graph=True)
    inside = (p.detach() >= 1e-10) & (p.detach() <= 1 - 1e-10)
    g_split = (gp - gn + gq) * inside                         # total derivative: d(1 - p)/dp = -1, dp/dp = 1
    assert (g_split.detach() - g).abs().max().item() <= 1e-12 * g.abs().max().item()
    dn, dq = torch.autograd.grad(g_split.sum(), (qn, qp))
    bound = U * ((qn * dn).abs() + (qp * dq).abs()).detach()
    return loss.item(), float((tt == 1).sum()), g, bound


def focal_fp32_rtol(pred, target, alpha, beta):
    """The rtol that the formula in fp32 torch on the CPU needs against float64, element by element, after `bound` is taken off:
    how FOCAL_RTOL of tests/test_gpu_heads.py was measured, for any exponents."""
    _, _, g, bound = focal_ref(pred, target, alpha, beta)
    p = torch.as_tensor(pred).float().requires_grad_()
    g32 = torch.autograd.grad(focal_formula(p, torch.as_tensor(target).float(), alpha, beta)[0].sum(), p)[0].double()
    over = ((g32 - g).abs() - bound).clamp_min(0)
    nz = g != 0
    return (over[nz] / g[nz].abs()).max().item()


# (alpha, beta) of the device test; the last pair runs `powf` in every power of the kernel
FOCAL_EXPONENTS = ((2, 4), (1, 4), (3, 2), (1.5, 2.5))
FOCAL_SHAPES = ((1, 5, 7), (2, 24, 80))
# rtol of the device test at non-integer exponents, fixed BEFORE any device run: `focal_fp32_rtol` at (1.5, 2.5) on the inputs of
# the test gives 8.35e-8 for (1, 5, 7) and 1.96e-7 for (2, 24, 80) (fp32 torch on the CPU against float64, `bound` taken off);
# times 4, the factor of FOCAL_RTOL, for a device `powf` / `logf` a few units in the last place from the host's.
# (The integer pairs need 1.90e-7, 2.12e-7 and 2.24e-7 on the same inputs and keep FOCAL_RTOL = 4 x 2.9e-7.)
FOCAL_POW_RTOL = 4 * 1.96e-7


def focal_inputs(shape):
    """`focal_inputs` of tests/test_gpu_heads.py (one prediction outside the clamp's pass band per branch) with three targets
    replaced: 1.5 and -0.1 lie outside [0, 1] -- no loss, no gradient, no positive -- and -0.0 is a plain 0.
    Returns (pred, tgt, outside cells (2), the -0.0 cell)."""
    import test_gpu_heads as TH
    pred, tgt, out_neg, out_pos = TH.focal_inputs(shape)
    free = [tuple(c) for c in np.argwhere((tgt < 0.9) & (tgt > 0)) if tuple(c) not in (out_neg, out_pos)]
    hi, lo, mz = free[0], free[len(free) // 2], free[-1]
    tgt[hi], tgt[lo], tgt[mz] = 1.5, -0.1, -0.0
    assert np.signbit(tgt[mz]) and tgt[mz] == 0
    return pred, tgt, (hi, lo), mz
