"""dcd_dcn_v2_forward / dcd_dcn_v2_backward through the C ABI on poisoned, guarded buffers (tests/arena.py): one case per route of
csrc/dcn_v2.hip, each taken from tests/test_gpu_dcn.py's own lists and pinned the way that file pins routes.

Every input lies between guard words of NaN, the output and all five gradients start as NaN, the workspace is exactly
dcd_dcn_v2_workspace_bytes of NaN, 256-byte aligned as include/dcd_hip.h asks.  After the call: no guard word changed, no input
changed, no output element left unwritten, and the values within the bounds of tests/test_gpu_dcn.py against the same oracle
(2e-5 forward, 5e-5 backward: test_forward_matches_oracle / test_backward_matches_oracle; BF16X3_TOL and BF16_TOL of that file in
the reduced precisions).  A missed zero-fill adds to NaN, a read past an input brings NaN in: both fail the comparison.

No bit comparison between two calls here: "grad_input and grad_weight are summed with fp32 atomics where work units overlap ...
order-nondeterministic sums" (include/dcd_hip.h, dcd_dcn_v2_backward)."""
import pytest
import torch

from arena import Arena
from test_gpu_dcn import BF16_TOL, BF16X3_TOL, CASES, DENSE_CASES, WIDE_SWEEP_CASES, close, make_case

pytestmark = pytest.mark.gpu

PREC = {"f32": 0, "bf16x3": 1, "bf16": 2}
TOL = {"f32": (2e-5, 5e-5), "bf16x3": (BF16X3_TOL, BF16X3_TOL), "bf16": (BF16_TOL, BF16_TOL)}
K3 = (3, 3, 1, 1, 1, 1, 1, 1)


@pytest.fixture(autouse=True)
def _fresh_launch_policy(cuda):
    """As in tests/test_gpu_dcn.py: the backward's launch policy is keyed by the weight's address; every test starts without history."""
    from dcd_amd import _lib
    _lib.lib().dcd_dcn_v2_forget(None)
    yield
    _lib.lib().dcd_dcn_v2_forget(None)


def _wide_case():
    B, C, Co, H, W, osc = min(WIDE_SWEEP_CASES, key=lambda c: c[0] * max(c[1], c[2]) * c[3] * c[4])
    x, w, b, off, m, gy = make_case(B, C, Co, H, W, off_scale=osc, seed=31)
    off[:, :, :, 1::4] += 1.4              # test_one_pass_backward_wide_outputs' quarter collisions
    off[:, :, :, 3::4] -= 1.4
    return (x, w, b, off, m, gy), K3 + (1,)


def _general_case(geo, B, C, Co, H, W, dg, osc, seed):
    """The tensors of test_dense_path_matches_oracle / test_general_geometry for one geometry."""
    kh, kw, sh, sw, ph, pw, dh, dw = geo
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    off = torch.randn(B, 2 * dg * kh * kw, Ho, Wo, generator=g) * osc
    m = torch.rand(B, dg * kh * kw, Ho, Wo, generator=g)
    w = torch.randn(Co, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    b = torch.randn(Co, generator=g)
    gy = torch.randn(B, Co, Ho, Wo, generator=g)
    return (x, w, b, off, m, gy), geo + (dg,)


def _listed(case, seed=1):
    B, C, Co, H, W, dg, osc = case
    return make_case(B, C, Co, H, W, dg, off_scale=osc, seed=seed), K3 + (dg,)


def _dense_case():
    B, C, Co, H, W, dg, osc, geo = min(DENSE_CASES, key=lambda c: c[0] * max(c[1], c[2]) * c[3] * c[4])
    return _general_case(geo, B, C, Co, H, W, dg, osc, 21)


# name, builder of ((x, w, b, off, m, gy), geometry), environment, precision
ROUTES = [
    ("register-gather", lambda: _listed(CASES[1]), {}, "f32"),
    ("far-outside-dg3", lambda: _listed(CASES[6]), {}, "f32"),
    ("tiled-one-pass", lambda: _listed(CASES[8]), {}, "f32"),
    ("tiled-one-pass", lambda: _listed(CASES[8]), {}, "bf16x3"),
    ("tiled-one-pass", lambda: _listed(CASES[8]), {}, "bf16"),
    ("ragged", lambda: _listed(CASES[9]), {}, "f32"),
    ("stand-down", lambda: _listed(CASES[11]), {}, "f32"),
    ("tiled-one-pass", lambda: _listed(CASES[8]), {"DCD_BWD_SWEEP": "0"}, "f32"),            # the three-pass backward
    ("wide-outputs", _wide_case, {"DCD_SWEEP_WIDE": "1"}, "f32"),
    ("column-buffer", _dense_case, {"DCD_DCN_DENSE": "1"}, "f32"),
    ("stride-2", lambda: _general_case((3, 3, 2, 2, 1, 1, 1, 1), 2, 8, 6, 11, 13, 1, 2.0, 5), {}, "f32"),
]


_PROBLEMS = {}


def test_the_cases_are_the_ones_the_routes_need():
    assert CASES[1] == (2, 5, 4, 7, 9, 1, 3.0) and CASES[6] == (1, 6, 3, 5, 6, 3, 6.0) and CASES[8] == (2, 64, 64, 24, 64, 1, 0.5)
    assert CASES[9] == (1, 12, 70, 17, 36, 1, 1.5) and CASES[11] == (2, 64, 64, 16, 64, 1, 12.0)


@pytest.mark.parametrize("name,build,env,prec", ROUTES,
                         ids=["%s-%s%s" % (r[0], r[3], "-three-pass" if "DCD_BWD_SWEEP" in r[2] else "") for r in ROUTES])
def test_dcn_on_poisoned_buffers(cuda, oracle_dcn, monkeypatch, name, build, env, prec):
    from dcd_amd import _lib
    L = _lib.lib()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _PROBLEMS:                     # one oracle run per case, shared by its precisions and routes; never modified
        tensors, geo = build()
        _PROBLEMS[name] = (tensors, geo, oracle_dcn.dcn_v2_forward(*tensors[:5], *geo), oracle_dcn.dcn_v2_backward(*tensors, *geo))
    (x, w, b, off, m, gy), geo, ref, refg = _PROBLEMS[name]
    B, C, H, W = x.shape
    Co = w.shape[0]
    geom = (B, C, H, W, Co) + geo
    nbytes = L.dcd_dcn_v2_workspace_bytes(*geom)
    assert nbytes > 0
    tol_f, tol_b = TOL[prec]

    ar = Arena(cuda)
    dx, dw, db, doff, dm = (ar.place(t, n) for t, n in ((x, "input"), (w, "weight"), (b, "bias"), (off, "offset"), (m, "mask")))
    y = ar.out(ref.shape, "output")
    ws = ar.scratch(nbytes, "workspace", align=256)
    st = _lib.stream_of(dx)
    assert L.dcd_dcn_v2_forward(st, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), doff.data_ptr(), dm.data_ptr(), y.data_ptr(), *geom,
                                PREC[prec], ar.ptr(ws), nbytes) == 0
    ar.check("%s %s forward" % (name, prec))
    close(y, ref, tol_f, "%s %s forward" % (name, prec))

    ar = Arena(cuda)
    dx, dw, db, doff, dm, dgy = (ar.place(t, n) for t, n in ((x, "input"), (w, "weight"), (b, "bias"), (off, "offset"), (m, "mask"),
                                                            (gy, "grad_output")))
    names = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
    grads = [ar.out(t.shape, n) for t, n in zip((x, off, m, w, b), names)]
    ws = ar.scratch(nbytes, "workspace", align=256)
    assert L.dcd_dcn_v2_backward(st, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), doff.data_ptr(), dm.data_ptr(), dgy.data_ptr(),
                                 *[g.data_ptr() for g in grads], *geom, PREC[prec], ar.ptr(ws), nbytes) == 0
    ar.check("%s %s backward" % (name, prec))
    for n, g_, r_ in zip(names, grads, refg):
        close(g_, r_, tol_b, "%s %s %s" % (name, prec, n))
