"""csrc/optim.hip through the C ABI (dcd_clip_grad_norm_scalars + dcd_adamw_apply) on poisoned, guarded buffers (tests/arena.py),
against the float64 reference of tests/optim_refs.py: at the element counts around a thread's four elements, an update block and a
norm block; with every pointer aligned and with the misaligned layouts that send the kernels down their scalar loops (the
data-parallel trainer packs its gradients back to back, so most of them sit at 4-byte alignment); with launch tables that fill
exactly, overflow by one and hold zero-element entries; with one parameter group and with two.

Layout of a case.  The tensors of one kind (p, g, m, v) are packed into ONE arena buffer: each tensor starts `offset` floats past a
16-byte boundary and is followed by 1..4 filler floats up to the next boundary.  Filler words are quiet NaNs with a payload of
their own: the arena guards the slab's ends, the test compares every filler word itself -- a store one element past a tensor's end
or before its start changes one, a load from there makes the norm NaN.  The workspace has exactly the advertised byte count and is
poisoned, `scal` is a poisoned 4-float output of which elements 0..2 must be written and element 3 must not.

Bounds.  Against float64 the kernels are held to the bounds tests/test_gpu_optim.py sets for the same quantities (2e-6 on the norm,
the coefficient and the clipped gradients; 2e-7 max|g| on the first moment; 2e-7 max|g|^2 on the second; 2e-4 of the largest update).
Those were set against the library, so the library calls (`trainer.clip_grad_norm`, `guard_nonfinite_step`, fused capturable
torch.optim.AdamW) run on the same inputs in the same layout, and the kernel may be at most TWICE as far from float64 as the library
is -- the margin covers a different order of the block sums and nothing more -- with a floor of one fp32 ulp of the quantity's scale
for where the library happens to be exact.  The scale is the one the bound above is relative to; for the update it is the larger of
the largest update and the largest parameter, because the update is read as a difference of stored fp32 parameters, whose
rounding unit is the parameter's ulp (parameters are drawn at 1e-4, below one update, so that this hides no wrong step size).
`pytest -s` prints both distances per case.

Measured on an MI355X, worst case of the module, distance from float64 relative to the quantity's scale (in ulps of it), kernel /
library in the case where the kernel is farthest, then the library's own worst anywhere:
  norm          5.3e-8 (0.66) / 2.7e-8 (0.34), one tensor of 3 elements;   library's worst 6.7e-8 (0.84)
  coefficient   9.1e-8 (1.13) / 1.0e-8 (0.13), the same case;              library's worst 1.0e-7 (1.25)
  gradient      1.1e-7 (1.71) / 3.2e-8 (0.53), 240 tensors;                library's worst 1.2e-7 (2.00)
  exp_avg       2.0e-8 (0.26) / 1.1e-8 (0.16), 240 tensors;                library's worst 1.9e-8 (0.31)
  exp_avg_sq    2.3e-9 (0.04) / 1.3e-9 (0.02), 240 tensors;                library's worst 2.9e-9 (0.04)
  update        1.9e-7 (2.41) / 1.9e-7 (2.41), two groups;                 largest kernel : library ratio 1.54 : 0.46 ulp (3 elements)
The comparison with the library is made over the case, not per tensor (see `Judge`): read per tensor, ONE one-element tensor of some
3 000 (tensor 42 of the 240-tensor case) had the kernel's update 2.07 ulp from float64 with the library's 0.07 ulp from it, in a case
where the library's own worst update is 2.21 ulp from float64 and the kernel's 2.28.
"""
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import optim_refs
from arena import Arena
from transport_refs import same_bits

pytestmark = pytest.mark.gpu

# csrc/optim.hip: OPT_CHUNK (elements per block of the update), OPT_NCHUNK (elements per block of the norm), OPT_MAXT (tensors per
# launch of the update), OPT_MAXG (gradients per launch of the norm), OPT_MAXS (step counters per launch); a thread takes four
# consecutive elements
OPT_CHUNK, OPT_NCHUNK, OPT_MAXT, OPT_MAXG, OPT_MAXS = 4096, 8192, 80, 240, 448
COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]
ALIGNMENTS = {                     # floats between a 16-byte boundary and the start of p, g, m, v
    "aligned": (0, 0, 0, 0),
    "g+1": (0, 1, 0, 0),           # the data-parallel layout: parameters and moments from the allocator, gradients packed
    "p+2": (2, 0, 0, 0),
    "pgmv+1231": (1, 2, 3, 1),
}
KINDS = "pgmv"
FILL_BITS = {k: 0x7FC0A5A5 ^ (i << 12) for i, k in enumerate(KINDS)}
BETAS, EPS, WD = (0.9, 0.99), 1e-8, 1e-2
LRS = (float(torch.tensor(3e-4, dtype=torch.float32)), float(torch.tensor(6e-4, dtype=torch.float32)))
STEP0, STEP_AHEAD = 2.0, 7.0


# ------------------------------------------------------------------------------------------------------------ problems
def make_problem(name, sizes, offsets, groups=None, ahead=(), gscale=1.0, seed=0):
    """Host data of one case (do not modify).  sizes: element count per tensor (0: an entry with null pointers); offsets: per tensor
    the floats (p, g, m, v) start past a 16-byte boundary; groups: parameter group per tensor; ahead: tensors whose step counter
    is STEP_AHEAD instead of STEP0."""
    gen = torch.Generator().manual_seed(seed)
    pr = SimpleNamespace(name=name, sizes=list(sizes), offsets=list(offsets), groups=list(groups or [0] * len(sizes)))
    assert len(pr.offsets) == len(pr.sizes) == len(pr.groups)
    pr.data = {k: [] for k in KINDS}
    pr.hist_max = []
    b1, b2 = BETAS
    for n in pr.sizes:
        pr.data["p"].append(1e-4 * torch.randn(n, generator=gen))
        g = gscale * torch.randn(n, generator=gen)
        pr.data["g"].append(g)
        # the moments are what two earlier steps left: sums of terms of the (clipped, ~0.37 x) gradients' size, which is what the
        # moment bounds are relative to.  In a tensor of a few elements the earlier gradients point the way of this one, so that
        # its largest update, the update bound's scale, cannot vanish by cancellation in a single element
        h = [0.37 * gscale * torch.randn(n, generator=gen) for _ in range(2)]
        if n < 64:
            h = [x.abs() * torch.where(g >= 0, 1.0, -1.0) for x in h]
        pr.data["m"].append(((1 - b1) * (b1 * h[0] + h[1])).float())
        pr.data["v"].append(((1 - b2) * (b2 * h[0] * h[0] + h[1] * h[1])).float())
        pr.hist_max.append(max(x.abs().max().item() for x in h) if n else 0.0)
    pr.steps = torch.tensor([STEP_AHEAD if i in ahead else STEP0 for i in range(len(pr.sizes))], dtype=torch.float32)
    return pack(pr)


def pack(pr):
    """The flat buffer of each kind: [offset filler words | the tensor | 1..4 filler words] per tensor, every such segment starting
    on a 16-byte boundary."""
    pr.flat, pr.start, pr.filler = {}, {}, {}
    for ki, k in enumerate(KINDS):
        cursor, starts = 0, []
        for n, off in zip(pr.sizes, pr.offsets):
            if n == 0:
                starts.append(None)
                continue
            assert cursor % 4 == 0 and 0 <= off[ki] < 4
            starts.append(cursor + off[ki])
            cursor += off[ki] + n
            cursor += 4 - cursor % 4
        flat = torch.full((cursor,), FILL_BITS[k], dtype=torch.int32).view(torch.float32)
        filler = torch.ones(cursor, dtype=torch.bool)
        for t, s in zip(pr.data[k], starts):
            if s is not None:
                flat[s:s + t.numel()] = t
                filler[s:s + t.numel()] = False
        assert int(filler.sum()) >= sum(1 for s in starts if s is not None)
        pr.flat[k], pr.start[k], pr.filler[k] = flat, starts, filler
    return pr


def views(pr, flats):
    """Per kind the list of per-tensor views into `flats[kind]` (None for a zero-element entry)."""
    return {k: [None if s is None else flats[k][s:s + n] for n, s in zip(pr.sizes, pr.start[k])] for k in KINDS}


def assert_alignment(pr, vs):
    """The pointers meant to be misaligned are, the others are not: a refactor of this file cannot fall back to the float4 path."""
    for i, (n, off) in enumerate(zip(pr.sizes, pr.offsets)):
        if n == 0:
            continue
        for ki, k in enumerate(KINDS):
            at = vs[k][i].data_ptr()
            if off[ki]:
                assert at % 16 != 0 and at % 16 == 4 * off[ki], (pr.name, i, k, hex(at))
            else:
                assert at % 16 == 0, (pr.name, i, k, hex(at))


# ------------------------------------------------------------------------------------------------------------ the three runs
def _table(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _counts(ns):
    return (ctypes.c_int64 * len(ns))(*ns)


def run_kernels(cuda, pr, max_norm, poison=True, apply=True):
    """One dcd_clip_grad_norm_scalars over all gradients, then one dcd_adamw_apply per parameter group.  Returns what the device
    holds afterwards, on the host: flat buffers per kind, step counters, scal."""
    from dcd_amd import _lib
    L = _lib.lib()
    st = torch._C._cuda_getCurrentRawStream(cuda.index if cuda.index is not None else torch.cuda.current_device())
    ar = Arena(cuda, poison=poison)
    flats = {k: ar.place(pr.flat[k], k, inplace=True) for k in KINDS}
    steps = ar.place(pr.steps, "steps", inplace=True)
    lr = ar.place(torch.tensor(LRS, dtype=torch.float32), "lr")
    vs = views(pr, flats)
    assert_alignment(pr, vs)
    n_all = _counts(pr.sizes)
    nbytes = L.dcd_clip_adamw_workspace_bytes(len(pr.sizes), n_all)
    assert nbytes == 8 * sum((n + OPT_NCHUNK - 1) // OPT_NCHUNK for n in pr.sizes) + 64
    ws = ar.scratch(nbytes, "workspace")
    scal = ar.out((4,), "scal", written=torch.tensor([True, True, True, False]))
    assert L.dcd_clip_grad_norm_scalars(st, len(pr.sizes), _table(vs["g"]), n_all, float(max_norm), ws.data_ptr(), nbytes,
                                        scal.data_ptr()) == 0
    if apply:
        for gi in sorted(set(pr.groups)):
            idx = [i for i, g in enumerate(pr.groups) if g == gi]
            pick = lambda k: _table([vs[k][i] for i in idx])
            step_ptrs = (ctypes.c_void_p * len(idx))(*[steps[i:i + 1].data_ptr() for i in idx])
            assert L.dcd_adamw_apply(st, len(idx), pick("p"), pick("g"), pick("m"), pick("v"), step_ptrs,
                                     _counts([pr.sizes[i] for i in idx]), lr[gi:gi + 1].data_ptr(), BETAS[0], BETAS[1], EPS, WD,
                                     scal.data_ptr()) == 0
    ar.check(pr.name)
    out = SimpleNamespace(flat={k: flats[k].cpu() for k in KINDS}, steps=steps.cpu(), scal=scal.cpu())
    for k in KINDS:                                            # the words before and after every tensor keep their bits
        moved = ~same_bits(out.flat[k], pr.flat[k]) & pr.filler[k]
        assert not moved.any(), "%s: %d filler words of %s changed, the first at float %d" % (
            pr.name, int(moved.sum()), k, int(torch.nonzero(moved)[0]))
    out.t = views(pr, out.flat)
    return out


def run_library(cuda, pr, max_norm):
    """The library calls on the same values in the same (mis)aligned layout."""
    from dcd_amd.engine import trainer
    flats = {k: pr.flat[k].to(cuda) for k in KINDS}
    vs = views(pr, flats)
    assert_alignment(pr, vs)
    params, groups = {}, []
    for gi in sorted(set(pr.groups)):
        ps = []
        for i, g in enumerate(pr.groups):
            if g == gi and pr.sizes[i]:
                params[i] = torch.nn.Parameter(vs["p"][i])
                assert params[i].data_ptr() == vs["p"][i].data_ptr()
                params[i].grad = vs["g"][i]
                ps.append(params[i])
        if ps:
            groups.append({"params": ps, "lr": torch.tensor(LRS[gi], dtype=torch.float32, device=cuda)})
    opt = torch.optim.AdamW(groups, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, fused=True, capturable=True)
    for i, p in params.items():
        opt.state[p] = {"step": torch.tensor(float(pr.steps[i]), dtype=torch.float32, device=cuda), "exp_avg": vs["m"][i],
                        "exp_avg_sq": vs["v"][i]}
    ordered = [params[i] for i in sorted(params)]
    total = trainer.clip_grad_norm(ordered, max_norm)
    coef = (max_norm / (total + 1e-6)).clamp(max=1.0)          # the coefficient clip_grad_norm multiplied with, from the same operations
    trainer.guard_nonfinite_step(opt, total)
    opt.step()
    out = SimpleNamespace(flat={k: flats[k].cpu() for k in KINDS}, total=float(total), coef=float(coef))
    out.steps = {i: float(opt.state[p]["step"]) for i, p in params.items()}
    out.t = views(pr, out.flat)
    return out


def reference(pr, max_norm):
    """Float64: norm, coefficient, and per tensor the clipped gradient and p, m, v after the step."""
    ref = SimpleNamespace()
    ref.total = optim_refs.total_norm64(pr.data["g"])
    ref.coef = optim_refs.clip_coef64(ref.total, max_norm)
    ref.g, ref.p, ref.m, ref.v = [], [], [], []
    for i, n in enumerate(pr.sizes):
        p, g, m, v = (pr.data[k][i] for k in KINDS)
        np_, nm, nv = optim_refs.adamw_step64(p, g, m, v, float(pr.steps[i]) + 1.0, LRS[pr.groups[i]], BETAS, EPS, WD, ref.coef)
        ref.g.append(g.double() * ref.coef)
        ref.p.append(np_)
        ref.m.append(nm)
        ref.v.append(nv)
    return ref


# ------------------------------------------------------------------------------------------------------------ the verdict
def ulp(x):
    """One unit in the last place of an fp32 number of magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 2.0 ** -126 else 2.0 ** -149


class Judge:
    """Holds every sample (one quantity of one tensor) to `bound` at once, and collects the kernel's and the library's distance from
    float64 in ulps of the sample's scale.  `verdict()` then compares the two over the case: the kernel's largest distance may be
    at most twice the library's largest, floor one ulp.  Over the case, not per tensor, because a distance from float64 is the
    maximum over a sample of rounding errors and the two maxima only compare over the same sample: both sides do the same
    operations on operands that differ in the last bit of the coefficient, so in a tensor of ONE element each side draws one
    rounding error of the same distribution -- a chain of seven fp32 roundings for the update, up to about three ulps -- and
    either may be the lucky one.  For the one-tensor cases the two readings are the same."""

    def __init__(self, case):
        self.case, self.samples = case, {}

    def __call__(self, what, d_kernel, d_lib, scale, bound, where=""):
        if scale <= 0.0:                                       # an all-zero quantity: must be exact
            assert d_kernel == 0.0, (self.case, what, where)
            return
        assert d_kernel <= bound, "%s %s %s: %.3e from float64, bound %.3e" % (self.case, what, where, d_kernel, bound)
        self.samples.setdefault(what, []).append((d_kernel / ulp(scale), None if d_lib is None else d_lib / ulp(scale), d_kernel / scale,
                                                  None if d_lib is None else d_lib / scale, where))

    def verdict(self):
        for what, rows in sorted(self.samples.items()):
            k = max(rows, key=lambda r: r[0])
            if k[1] is None:
                print("optim-edges %-28s %-12s kernel %.3e of the scale (%.2f ulp)" % (self.case, what, k[2], k[0]))
                continue
            l = max(rows, key=lambda r: r[1])
            print("optim-edges %-28s %-12s kernel %.3e of the scale (%.2f ulp)  library %.3e (%.2f ulp)" % (
                self.case, what, k[2], k[0], l[3], l[1]))
            assert k[0] <= 2.0 * max(l[1], 1.0), "%s %s: the kernel is %.2f ulp of the scale from float64 (%s), the library %.2f (%s)" % (
                self.case, what, k[0], k[4], l[1], l[4])


def _dist(a, ref):
    return (a.double() - ref).abs().max().item() if ref.numel() else 0.0


def check_step(cuda, pr, max_norm, with_library=True):
    """One call pair on the arena, the library on the same inputs, float64; every check of the module's docstring."""
    ker = run_kernels(cuda, pr, max_norm)
    lib = run_library(cuda, pr, max_norm) if with_library else None
    ref = reference(pr, max_norm)
    judge = Judge(pr.name)
    assert same_bits(ker.scal[2:3], torch.zeros(1)).all(), "scal[2] must be +0 for a finite norm"
    # bounds: tests/test_gpu_optim.py::test_clip_and_step_equals_the_library_calls (2e-6 norm and clipped gradients, 2e-7 max|g| and
    # 2e-7 max|g|^2 on the moments) and ::test_single_step_update_matches_to_rounding (2e-4 of the largest update)
    judge("norm", abs(float(ker.scal[0]) - ref.total), lib and abs(lib.total - ref.total), ref.total, 2e-6 * ref.total)
    judge("coefficient", abs(float(ker.scal[1]) - ref.coef), lib and abs(lib.coef - ref.coef), ref.coef, 2e-6 * ref.coef)
    if ref.coef == 1.0:
        assert float(ker.scal[1]) == 1.0
    assert torch.equal(ker.steps, pr.steps + 1.0), "every step counter advances by exactly 1"
    for i, n in enumerate(pr.sizes):
        if n == 0:
            continue
        if lib is not None:
            assert lib.steps[i] == float(pr.steps[i]) + 1.0
        where = "tensor %d (%d elements)" % (i, n)
        kt = {k: ker.t[k][i] for k in KINDS}
        lt = {k: lib.t[k][i] for k in KINDS} if lib is not None else None
        if ref.coef == 1.0:                                    # written back only when it clips
            assert same_bits(kt["g"], pr.data["g"][i]).all(), where
        else:
            assert ((kt["g"].double() - ref.g[i]).abs() <= 2e-6 * ref.g[i].abs()).all(), where
        gmax = ref.g[i].abs().max().item()
        judge("gradient", _dist(kt["g"], ref.g[i]), lt and _dist(lt["g"], ref.g[i]), gmax, 2e-6 * gmax, where)
        gmax = max(gmax, pr.hist_max[i])                       # the largest gradient the moments have seen, as in test_gpu_optim.py
        judge("exp_avg", _dist(kt["m"], ref.m[i]), lt and _dist(lt["m"], ref.m[i]), gmax, 2e-7 * gmax, where)
        judge("exp_avg_sq", _dist(kt["v"], ref.v[i]), lt and _dist(lt["v"], ref.v[i]), gmax * gmax, 2e-7 * gmax * gmax, where)
        p0 = pr.data["p"][i].double()
        upd = ref.p[i] - p0
        umax = upd.abs().max().item()
        # the update is read off stored fp32 parameters: its rounding unit is the parameter's
        scale = max(umax, ref.p[i].abs().max().item())
        assert scale <= 8.0 * umax, "parameters must stay small against an update (%s)" % where
        judge("update", _dist(kt["p"].double() - p0, upd), lt and _dist(lt["p"].double() - p0, upd), scale, 2e-4 * umax, where)
    judge.verdict()
    return ker, lib, ref


# ------------------------------------------------------------------------------------------------------------ the cases
def _max_norm_for(pr, fraction=0.37):
    """A clip threshold below the norm (as an fp32 number, what the entry point takes): the coefficient is ~`fraction`, every stored
    gradient is rewritten."""
    return float(torch.tensor(fraction * optim_refs.total_norm64(pr.data["g"]), dtype=torch.float32))


@pytest.mark.parametrize("layout", list(ALIGNMENTS))
@pytest.mark.parametrize("n", COUNTS)
def test_one_tensor_at_block_edges_and_alignments(cuda, n, layout):
    """One tensor of n elements, clip active, in each pointer layout."""
    off = ALIGNMENTS[layout]
    pr = make_problem("n=%d %s" % (n, layout), [n], [off], seed=n)
    vs = views(pr, pr.flat)
    assert all((vs[k][0].storage_offset() % 4 != 0) == bool(o) for k, o in zip(KINDS, off))
    ker, lib, ref = check_step(cuda, pr, _max_norm_for(pr))
    assert ref.coef < 0.5 and float(ker.scal[1]) < 0.5


def _small_sizes(count):
    return [1 + i % 7 for i in range(count)]


@pytest.mark.parametrize("count", [80, 81, 240, 241, 448, 449])
def test_launch_tables_filled_and_overflowing_by_one(cuda, count):
    """`count` tensors of 1 to 7 elements in ONE group: the update's table (OPT_MAXT = 80), the norm's (OPT_MAXG = 240) and the step
    counters' (OPT_MAXS = 448) each exactly full and one past full; every fourth gradient pointer at each misalignment."""
    assert {80, 81} == {OPT_MAXT, OPT_MAXT + 1} and {240, 241} == {OPT_MAXG, OPT_MAXG + 1} and {448, 449} == {OPT_MAXS, OPT_MAXS + 1}
    sizes = _small_sizes(count)
    pr = make_problem("%d tensors" % count, sizes, [(0, i % 4, 0, 0) for i in range(count)], ahead=(count - 1,), seed=count)
    check_step(cuda, pr, _max_norm_for(pr))


@functools.lru_cache(maxsize=None)
def five_hundred():
    """500 tensors of 1 to 7 elements; every 37th has 8193 (two blocks of the norm, three of the update), every 50th has zero
    elements and null pointers."""
    sizes = _small_sizes(500)
    for i in range(36, 500, 37):
        sizes[i] = OPT_NCHUNK + 1
    for i in range(49, 500, 50):
        sizes[i] = 0
    live = [n for n in sizes if n]                             # zero-element entries take no table slot
    multi = [j for j, n in enumerate(live) if n > OPT_NCHUNK]
    assert len(live) > 2 * OPT_MAXG and len(sizes) > OPT_MAXS
    assert any(j < OPT_MAXG for j in multi) and any(OPT_MAXG <= j < 2 * OPT_MAXG for j in multi), "a multi-block tensor on each side of entry 240"
    assert sizes.count(0) == 10 and len(multi) == 13
    return make_problem("500 tensors", sizes, [(0, i % 4, (i // 4) % 2, 0) for i in range(500)], ahead=(36, 258), seed=500)


def test_five_hundred_tensors_across_every_launch_edge(cuda):
    """Three launches of the norm (the second and third write their partials at `part0`), seven of the update, two of the step
    counters; multi-block tensors on both sides of the norm's launch edge, zero-element entries with null pointers skipped."""
    pr = five_hundred()
    check_step(cuda, pr, _max_norm_for(pr))


def test_zero_element_entries_at_the_norm_table_edge(cuda):
    """The 240th and 241st entries of the list are the zero-element ones: the launch edge of the norm falls two entries later."""
    sizes = _small_sizes(260)
    sizes[OPT_MAXG - 1] = sizes[OPT_MAXG] = 0
    sizes[OPT_MAXG + 1] = OPT_NCHUNK + 1                      # the 240th LIVE entry, the last of the first launch, has two blocks
    assert sum(1 for n in sizes[:OPT_MAXG + 2] if n) == OPT_MAXG and sum(1 for n in sizes if n) > OPT_MAXG
    pr = make_problem("zeros at 240/241", sizes, [(0, i % 4, 0, 0) for i in range(260)], seed=241)
    check_step(cuda, pr, _max_norm_for(pr))


@pytest.mark.parametrize("ngroups", [1, 2])
def test_one_parameter_group_against_two(cuda, ngroups):
    """The norm runs once over all gradients; the update runs per group with that group's device learning rate; one tensor's step
    counter is ahead of the others (its bias corrections differ)."""
    sizes = [5, 4097, 1, 8193, 1024, 3, 12289, 7, 4096, 2, 1025, 33]
    groups = [i % ngroups for i in range(len(sizes))]
    pr = make_problem("%d group(s)" % ngroups, sizes, [(0, i % 2, 0, 0) for i in range(len(sizes))], groups=groups, ahead=(3,), seed=12)
    assert LRS[0] != LRS[1] and len(set(groups)) == ngroups
    ker, lib, ref = check_step(cuda, pr, _max_norm_for(pr))
    if ngroups == 2:                                           # the two learning rates show: same tensors, another group, another update
        one = reference(make_problem("as one group", sizes, pr.offsets, ahead=(3,), seed=12), _max_norm_for(pr))
        assert (one.p[1] - ref.p[1]).abs().max().item() > 0.1 * (ref.p[1] - pr.data["p"][1].double()).abs().max().item()


def test_the_norm_does_not_depend_on_what_the_workspace_held(cuda):
    """`adam_finalize`: "fixed assignment, fixed tree: reproducible" -- the 500-tensor norm on a poisoned and on a zero-filled
    workspace gives the same bits in scal[0..2]."""
    pr = five_hundred()
    mn = _max_norm_for(pr)
    a = run_kernels(cuda, pr, mn, poison=True, apply=False)
    b = run_kernels(cuda, pr, mn, poison=False, apply=False)
    assert same_bits(a.scal[:3], b.scal[:3]).all(), (a.scal, b.scal)
    assert math.isfinite(float(a.scal[0])) and 0.0 < float(a.scal[1]) < 1.0 and float(a.scal[2]) == 0.0
    for k in KINDS:                                            # the norm alone writes no tensor
        assert same_bits(a.flat[k], pr.flat[k]).all()
    assert torch.equal(a.steps, pr.steps)


# ------------------------------------------------------------------------------------------------------------ nothing may move
def _frozen_problem(kind):
    pr = make_problem("frozen by " + kind, [5, 4097, 1025, 8193], [(0, 0, 0, 0), (0, 1, 0, 0), (1, 2, 3, 1), (0, 0, 0, 0)], ahead=(2,), seed=77)
    if kind == "inf":
        pr.data["g"][1][4096] = float("inf")                   # the scalar tail of an unaligned gradient's last block
    elif kind == "nan":
        pr.data["g"][3][8192] = float("nan")                   # the lone element of a second norm block
    else:
        for g in pr.data["g"]:                                 # finite, but 9e38 > FLT_MAX = 3.4e38: the fp32 square overflows
            g.copy_(torch.where(g >= 0, torch.full_like(g, 3e19), torch.full_like(g, -3e19)))
    return pack(pr)


@pytest.mark.parametrize("kind", ["inf", "nan", "overflow"])
def test_a_non_finite_norm_moves_nothing(cuda, kind):
    """+inf, NaN, and finite gradients of 3e19 whose squares overflow the per-thread fp32 sum: scal[2] == 1, every bit of p, g, m, v and
    every step counter as before.  The library reaches the same verdict (its norm is not finite either, its step is skipped); it
    does scale the gradients, which the kernels do not."""
    pr = _frozen_problem(kind)
    if kind == "overflow":
        assert all(torch.isfinite(g).all() for g in pr.data["g"]) and math.isfinite(optim_refs.total_norm64(pr.data["g"]))
    ker = run_kernels(cuda, pr, 15.0)
    assert float(ker.scal[2]) == 1.0 and float(ker.scal[1]) == 1.0 and not math.isfinite(float(ker.scal[0]))
    for k in KINDS:
        assert same_bits(ker.flat[k], pr.flat[k]).all(), "%s: %s moved" % (pr.name, k)
    assert torch.equal(ker.steps, pr.steps)
    lib = run_library(cuda, pr, 15.0)
    print("optim-edges %s: kernel norm %r, library norm %r" % (pr.name, float(ker.scal[0]), lib.total))
    assert not math.isfinite(lib.total), "the library's norm of the same gradients is finite: %r" % lib.total
    for k in "pmv":
        assert same_bits(lib.flat[k], pr.flat[k]).all(), "the library moved %s" % k
    assert all(s == float(pr.steps[i]) for i, s in lib.steps.items())


def _norm_problem(ratio, max_norm):
    """Gradients whose float64 norm is `ratio` x max_norm (to the fp32 rounding of the elements, ~1e-8)."""
    pr = make_problem("norm = %.3f max_norm" % ratio, [5, 4097, 1025], [(0, 0, 0, 0), (0, 1, 0, 0), (1, 2, 3, 1)], seed=5)
    total = optim_refs.total_norm64(pr.data["g"])
    s = ratio * max_norm / total
    for g, m, v in zip(pr.data["g"], pr.data["m"], pr.data["v"]):
        g.copy_((g.double() * s).float())
        m.mul_(s)
        v.mul_(s * s)
    pr.hist_max = [h * s for h in pr.hist_max]
    pack(pr)
    assert abs(optim_refs.total_norm64(pr.data["g"]) / max_norm - ratio) < 1e-6
    return pr


def test_max_norm_zero_means_no_clip(cuda):
    """max_norm = 0: the coefficient is exactly 1, g keeps its bits, the step still runs (no library twin: `trainer.clip_and_step`
    does not call the clip at all for a threshold of 0)."""
    pr = _norm_problem(3.0, 1.0)
    ker, _, ref = check_step(cuda, pr, 0.0, with_library=False)
    assert ref.coef == 1.0 and same_bits(ker.scal[1:2], torch.ones(1)).all()
    assert same_bits(ker.flat["g"], pr.flat["g"]).all()


def test_a_norm_just_below_max_norm_clamps_to_one(cuda):
    pr = _norm_problem(1.0 - 1e-3, 2.0)
    ker, lib, ref = check_step(cuda, pr, 2.0)
    assert ref.coef == 1.0 and same_bits(ker.scal[1:2], torch.ones(1)).all()
    assert same_bits(ker.flat["g"], pr.flat["g"]).all()


def test_a_norm_just_above_max_norm_rewrites_the_gradients(cuda):
    pr = _norm_problem(1.0 + 1e-3, 2.0)
    ker, lib, ref = check_step(cuda, pr, 2.0)
    assert 0.998 < ref.coef < 1.0 and 0.998 < float(ker.scal[1]) < 1.0
    for i in range(len(pr.sizes)):
        assert not same_bits(ker.t["g"][i], pr.data["g"][i]).any(), "every stored gradient is rewritten"
