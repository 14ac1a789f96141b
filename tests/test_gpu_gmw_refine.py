"""GMW inference on the device, through the C ABI via `ops`: `dcd_gmw_refine` (csrc/gmw.hip), `dcd_context_norm_relu_add_forward`
(csrc/heads.hip) and `gmw.inference.refine / evaluate` on top of them.

The reference of the kernel tests is the stock chain of `refine(fused=False)` -- `F.normalize`, the diagonal of
`pairwise_l2_dist`, `compute_reg_loss`, the location rule -- in float64 on the host; the yardstick E_ref is the SAME chain in fp32
on the host against that float64, per output, as the maximum relative error over all elements.  Where the chain is accurate (random
features, d ~ 1.4) the kernel is held to max(4 E_ref, 8 * 2^-24): the margin covers another summation order, the floor is there
because E_ref of the depth outputs is itself one or two roundings.  Where the chain cancels (f6 = f4 + 0.05 randn: the expanded
||a||^2 + ||b||^2 - 2 a.b on unit vectors, d ~ 0.05) the kernel's difference form has to be at least 16 times better than it.

Measured (MI355X, generator seeds below; host fp32 = E_ref):
    random features       weights: kernel 1.0e-07 ... 4.0e-07 against E_ref 2.5e-07 ... 3.2e-07 (native shape: 4.0e-07 against
                          2.8e-07);  depth, location: kernel <= 9.2e-08 against E_ref 1.4e-08 ... 1.9e-07
    f6 = f4 + 0.05 randn  weights: kernel 4.6e-07 against E_ref 2.7e-04;  depth: kernel 3.5e-07 against E_ref 7.7e-05
    fused tail            kernel 5.3e-08 ... 1.0e-07 against E_ref 8.9e-08 ... 1.1e-07 (of max |y|)
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 8 * 2.0 ** -24
NATIVE = (3, 128, 2628, 1500)


def make_case(B, C, K, num_k, seed, near=None):
    g = torch.Generator().manual_seed(seed)
    f4 = torch.randn(B, C, K, generator=g)
    f6 = torch.randn(B, C, K, generator=g) if near is None else f4 + near * torch.randn(B, C, K, generator=g)
    depths = 5 + 40 * torch.rand(B, K, generator=g)
    idx = torch.stack([torch.randperm(K, generator=g)[:num_k] for _ in range(B)], 0)
    sign = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    loc = torch.stack([sign * (1 + 9 * torch.rand(B, generator=g)), 1.4 + 0.5 * torch.rand(B, generator=g),
                       8 + 40 * torch.rand(B, generator=g)], 1)
    dim = torch.stack([1.4 + 0.4 * torch.rand(B, generator=g), 1.5 + 0.4 * torch.rand(B, generator=g),
                       3 + 1.5 * torch.rand(B, generator=g)], 1)
    return f4, f6, depths, idx, loc, dim


def stock_chain(case, dtype):
    """The arithmetic of `refine(fused=False)` after the extractors, in `dtype` on the host."""
    from dcd_amd.gmw import compute_reg_loss, pairwise_l2_dist
    from dcd_amd.gmw.inference import relocate
    f4, f6, depths, idx, loc, dim = (t.to(dtype) if t.is_floating_point() else t for t in case)
    out = []
    for b in range(f4.shape[0]):                                    # one K x K matrix at a time
        a = F.normalize(f4[b:b + 1].transpose(-2, -1), p=2, dim=-1)
        c = F.normalize(f6[b:b + 1].transpose(-2, -1), p=2, dim=-1)
        out.append(1.0 / pairwise_l2_dist(a, c).diagonal(offset=0, dim1=-2, dim2=-1))
    weights = torch.cat(out, 0)
    _, z = compute_reg_loss(depths, weights, loc[:, -1], idx)
    return weights, z, relocate(loc, dim, z)


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    d = ((got - ref) / ref).abs()
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).max().item()


@functools.lru_cache(maxsize=None)
def reference(key):
    """(case, float64 outputs, E_ref per output) -- computed once per case and shared."""
    case = make_case(*key)
    ref = stock_chain(case, torch.float64)
    e_ref = [rel_err(o, r) for o, r in zip(stock_chain(case, torch.float32), ref)]
    return case, ref, e_ref


def run_kernel(case, cuda):
    from dcd_amd import ops
    return ops.gmw_refine(*(t.to(cuda) for t in case))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [NATIVE,                      # the native shape
                                   (2, 5, 37, 20),              # the remainders of every vector and block width
                                   (1, 128, 130, 130),          # all edges gathered, K % 4 != 0
                                   (2, 16, 4400, 4300)])        # more gathered edges than the softmax stage keeps in LDS
def test_refine_kernel_against_float64_where_the_stock_chain_is_accurate(cuda, shape):
    case, ref, e_ref = reference(shape + (21,))
    got = run_kernel(case, cuda)
    for name, g, r, e in zip(("weights", "pred_depth", "pred_location"), got, ref, e_ref):
        err = rel_err(g, r)
        print("gmw_refine %s %s: kernel %.2e, host fp32 (E_ref) %.2e, bar %.2e" % (shape, name, err, e, max(4 * e, FLOOR)))
        assert g.shape == r.shape
        assert err <= max(4 * e, FLOOR), (name, err, e)


@pytest.mark.gpu
def test_refine_kernel_is_accurate_where_the_stock_chain_cancels(cuda):
    case, ref, e_ref = reference(NATIVE + (22, 0.05))
    got = run_kernel(case, cuda)
    for name, g, r, e in list(zip(("weights", "pred_depth"), got, ref, e_ref)):
        err = rel_err(g, r)
        print("gmw_refine f6 = f4 + 0.05 randn, %s: kernel %.2e, host fp32 stock chain (E_ref) %.2e, ratio %.0f" % (
            name, err, e, e / max(err, 1e-300)))
        assert err <= e / 16, (name, err, e)


@pytest.mark.gpu
def test_refine_kernel_edges_of_the_arithmetic(cuda):
    from dcd_amd import ops
    B, C, K, num_k = 2, 128, 2628, 1500
    f4, f6, depths, idx, loc, dim = make_case(B, C, K, num_k, 23)
    f4[:, :, 5] = 0.0                                   # an all-zero column: normalised to 0, d = ||f6 / n6|| = 1
    f6[0, :, 77] = f4[0, :, 77]                         # identical columns: d = 1e-15, w = 1e15
    idx[0, 3] = 77
    idx[0, 4:][idx[0, 4:] == 77] = 78
    w, z, ploc = ops.gmw_refine(*(t.to(cuda) for t in (f4, f6, depths, idx, loc, dim)))
    w, z, ploc = w.cpu(), z.cpu(), ploc.cpu()
    # a sum of C squares of a unit vector's components, each step rounded once: |d^2 - 1| <= (C + 3) 2^-24, and w = d^-1
    assert (w[:, 5] - 1).abs().max().item() <= 0.5 * (C + 3) * 2.0 ** -24 + 2.0 ** -23
    assert torch.isfinite(w).all() and torch.isfinite(z).all() and torch.isfinite(ploc).all()
    assert w[0, 77].item() > 1e14
    assert abs(z[0].item() - depths[0, 77].item()) <= 1e-6 * depths[0, 77].item()       # a one-hot softmax, not a NaN
    with pytest.raises(RuntimeError):
        ops.gmw_refine(f4[:, :, :100].contiguous().to(cuda), f6[:, :, :100].contiguous().to(cuda), depths[:, :100].contiguous().to(cuda),
                       idx[:, :101].clamp(max=99).to(cuda), loc.to(cuda), dim.to(cuda))          # num_k = 101 > K = 100
    idx[1, 7] = K                                       # an index outside [0, K): that object is NaN, nothing is read there
    w, z, ploc = ops.gmw_refine(*(t.to(cuda) for t in (f4, f6, depths, idx, loc, dim)))
    assert torch.isnan(z[1]).item() and torch.isnan(ploc[1]).all() and torch.isfinite(z[0]).item()


@pytest.mark.gpu
def test_refine_kernel_rows_do_not_depend_on_the_batch_and_repeat_bit_for_bit(cuda):
    case, _, _ = reference(NATIVE + (21,))
    dev = [t.to(cuda) for t in case]
    first = run_kernel(case, cuda)
    second = run_kernel(case, cuda)
    from dcd_amd import ops
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for i in range(NATIVE[0]):
        alone = ops.gmw_refine(*(t[i:i + 1].contiguous() for t in dev))
        for a, b in zip(alone, first):
            assert torch.equal(a[0], b[i]), i


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 128, 2628),      # 2 * 128 rows, the row-in-registers kernel
                                   (1, 3, 37),          # the wave-per-row kernel, K % 64 != 0
                                   (1, 5, 4100)])       # K % 4 == 0 but past the 4096 a row of registers holds
def test_context_norm_relu_add_against_float64(cuda, shape):
    """y = relu(context_norm(x)) + residual against float64; the yardstick is the fp32 stock formula on the host on the same input,
    both as max |error| / max |y| (an element of y can be arbitrarily close to zero, so a per-element ratio measures nothing),
    the bar max(4 E_ref, 8 * 2^-24) as for the refinement kernel."""
    from dcd_amd import ops
    g = torch.Generator().manual_seed(31)
    x = torch.randn(*shape, generator=g) * 2 + 0.5
    r = torch.randn(*shape, generator=g)

    def stock(x, r):
        m = torch.mean(x, 2, keepdim=True)
        v = torch.var(x, 2, keepdim=True)
        return F.relu((x - m) * (1.0 / torch.sqrt(v + 1e-3))) + r
    ref = stock(x.double(), r.double())
    scale = ref.abs().max().item()
    e_ref = (stock(x, r).double() - ref).abs().max().item() / scale
    y = ops.context_norm_relu_add(x.to(cuda), r.to(cuda), 1e-3)
    err = (y.cpu().double() - ref).abs().max().item() / scale
    print("context_norm_relu_add %s: kernel %.2e, host fp32 (E_ref) %.2e" % (shape, err, e_ref))
    assert y.shape == x.shape and err <= max(4 * e_ref, FLOOR), (err, e_ref)
    with pytest.raises(RuntimeError):
        ops.context_norm_relu_add(x.to(cuda).requires_grad_(), r.to(cuda))


@pytest.fixture(scope="module")
def fixture_run():
    """The fixture's records, the seeded model, and the float64 stock chain on the host (shared by the end-to-end tests)."""
    from oracle import torch_ops
    from dcd_amd.gmw import GMW, load_infer_data, refine
    fx = np.load(os.path.join(HERE, "golden", "gmw_infer.npz"))
    data = load_infer_data(json.loads(str(fx["records_json"])))
    torch.manual_seed(0)
    model = GMW().eval()
    model64 = GMW().double().eval()
    model64.load_state_dict(model.state_dict())
    _, loc64 = refine(model64, data, "cpu", batch_size=3, fused=False, compute_z=torch_ops.compute_z)
    return fx, data, model, loc64


@pytest.mark.gpu
def test_refine_on_the_device_meets_the_reference_fixture(cuda, fixture_run):
    from dcd_amd.gmw import refine
    fx, data, model, loc64 = fixture_run
    model = model.to(cuda)
    z, loc = refine(model, data, cuda, batch_size=4)                 # 4 + 2: the last, shorter batch goes through as it is
    assert np.allclose(z.numpy(), fx["pred_depth"], rtol=2e-5, atol=0)
    assert np.allclose(loc.numpy(), fx["pred_location"], rtol=2e-5, atol=0)
    z1, loc1 = refine(model, data, cuda, batch_size=256)
    assert torch.equal(z, z1) and torch.equal(loc, loc1)               # the batch size does not change a result
    zs, locs = refine(model, data, cuda, batch_size=4, fused=False)  # the stock chain on the device
    assert np.allclose(zs.numpy(), fx["pred_depth"], rtol=2e-5, atol=0)


@pytest.mark.gpu
def test_evaluate_scores_the_refined_files_like_the_float64_chain(cuda, fixture_run, tmp_path):
    from dcd_amd.eval import kitti_ap
    from dcd_amd.gmw import evaluate, write_results
    fx, data, model, loc64 = fixture_run
    ids = [str(i) for i in fx["ids"]]
    root = tmp_path / "kitti"
    (root / "training" / "label_2").mkdir(parents=True)
    (root / "training" / "ImageSets").mkdir()
    (root / "training" / "ImageSets" / "val.txt").write_text("".join(i + "\n" for i in ids))
    for i, text in zip(ids, fx["label_texts"]):
        (root / "training" / "label_2" / (i + ".txt")).write_text(str(text))
    text, result, moderate = evaluate(model.to(cuda), data, str(root), None, str(tmp_path / "run"), device=cuda)
    ref_dir = write_results(data, loc64, str(tmp_path / "ref"), ids)
    want, _ = kitti_ap.evaluate(str(root / "training" / "label_2"), ref_dir, str(root / "training" / "ImageSets" / "val.txt"), 0, "R40",
                                device=cuda)
    print(text)
    assert text == want
    assert sorted(os.listdir(tmp_path / "run" / "kitti_results_for_eval")) == [i + ".txt" for i in ids]
    assert moderate == float(want.split("\n")[3].split(",")[1]) and "Car_3d_0.70/moderate" in result
