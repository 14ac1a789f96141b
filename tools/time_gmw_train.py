"""Training GMW on the GPU: the device-side Sinkhorn against the stock loop, one iteration of `train_gmw`'s loop against a
hand-rolled `gmw_train_step` loop with `.item()` meters, and the kernels of csrc/transport.hip from traces of their own.

    python tools/time_gmw_train.py [--reps 5] [--out profiles/gmw_train.txt] [--no-trace]

Figures only, medians of alternating repetitions (the two routes of a comparison take turns inside one process):
  1. `ops.sinkhorn` and `RegularisedTransportFn.sinkhorn` on the same (B, 2628, 2628) distances at B = 8 and 16, for a seeded input
     the stock loop finishes in under 10 iterations and one it needs 30 or more for, with both iteration counts;
  2. one loop iteration (resident batch, `train_iteration`, the ring) against `gmw_train_step` + four `.item()`, B = 8 and 16;
  3. per kernel, from child processes under `rocprofv3 --kernel-trace` (started before this process opens the GPU): 30 working
     iterations (tolerance 0, cap 30) at B = 8 and B = 16 -- 221 MB of plans fit the 256 MiB Infinity Cache, 442 MB do not -- and
     a call whose 99 iterations after the first are empty launches (constant distances).
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

N_EDGES = 2628
LMBDA = 10.0
KERNELS = ("sinkhorn_gibbs", "sinkhorn_sweep", "sinkhorn_columns", "sinkhorn_scale", "dcd_zero_fill")


def distances(B, s, dev, seed=0):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(B, N_EDGES, 128, device=dev, generator=g), dim=-1)
    b = torch.nn.functional.normalize(a + s * torch.randn(B, N_EDGES, 128, device=dev, generator=g), dim=-1)
    return torch.cdist(a, b).contiguous()


def marginals(M):
    b, m, n = M.shape
    return M.new_full((b, m), 1.0 / m), M.new_full((b, n), 1.0 / n)


def stock_iterations(M, r, c, tolerance=1e-9, max_iterations=100):
    """The stock loop restated with a counter (the function itself does not return one)."""
    import torch
    K = torch.exp(-LMBDA * M.clamp_max(5.0))
    Kt = K.transpose(-2, -1)
    r, c = r.unsqueeze(-1), c.unsqueeze(-1)
    u, previous, it = r.clone(), torch.ones_like(r), 0
    for _ in range(max_iterations):
        if torch.all(torch.isclose(u, previous, atol=tolerance, rtol=0.0)):
            break
        previous = u
        u = r / K.matmul(c / Kt.matmul(u))
        it += 1
    return it


def alternate(routes, reps, inner):
    """[median seconds per call] of each route: `reps` rounds in which the routes take turns, `inner` calls per turn."""
    import torch
    times = [[] for _ in routes]
    for _ in range(reps):
        for i, fn in enumerate(routes):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t) / inner)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in times]


def time_sinkhorn(lines, reps, dev):
    import torch
    from dcd_amd import ops
    from dcd_amd.gmw.optimal_transport import RegularisedTransportFn as T
    lines.append("1. Sinkhorn forward on (B, %d, %d), lambda 10, tolerance 1e-9, cap 100: median ms per call (min, max)" % (N_EDGES, N_EDGES))
    for B in (8, 16):
        for label, s in (("fast", 1.0), ("slow", 0.05)):
            M = distances(B, s, dev)
            r, c = marginals(M)
            P, it = ops.sinkhorn(M, r, c, LMBDA, 1e-9, 100)
            stock = T.sinkhorn(M, r, c, LMBDA, 1e-9, 100)
            diff = ((P - stock).abs().max() / stock.max()).item()
            its = (int(it), stock_iterations(M, r, c))
            res = alternate((lambda: ops.sinkhorn(M, r, c, LMBDA, 1e-9, 100), lambda: T.sinkhorn(M, r, c, LMBDA, 1e-9, 100)), reps, 3)
            lines.append("  B %2d %s: ops.sinkhorn %7.3f (%.3f, %.3f) in %d iterations | stock %7.3f (%.3f, %.3f) in %d iterations | "
                         "%.2fx | plans differ by %.1e of their maximum"
                         % (B, label, res[0][0] * 1e3, res[0][1] * 1e3, res[0][2] * 1e3, its[0], res[1][0] * 1e3, res[1][1] * 1e3,
                            res[1][2] * 1e3, its[1], res[1][0] / res[0][0], diff))
            del M, P, stock
            torch.cuda.empty_cache()


def time_loop(lines, reps, dev):
    import torch
    from make_golden_gmw import inputs
    from dcd_amd.gmw import GMW, gmw_train_step
    from dcd_amd.gmw.data import ResidentRecords
    from dcd_amd.gmw.train import _Ring, build_gmw_optimizer, train_iteration
    lines.append("2. one training iteration at (cls 0.1, reg 1.0): median ms (min, max)")
    keys = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location")
    for B in (8, 16):
        data = dict(zip(keys, inputs(seed=11, B=4 * B)))
        torch.manual_seed(0)
        ours = GMW(device_sinkhorn=True).to(dev).train()
        opt_ours = build_gmw_optimizer(ours)
        rec, ring = ResidentRecords(data, dev), _Ring(10, dev)
        torch.manual_seed(0)
        theirs = GMW().to(dev).train()
        opt_theirs = torch.optim.AdamW(theirs.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-5)
        host = {k: torch.from_numpy(v) for k, v in data.items()}
        state = {"k": 0, "meters": [0.0] * 4}

        def next_index():
            state["k"] = (state["k"] + 1) % 4
            return list(range(state["k"] * B, (state["k"] + 1) * B))

        def loop_iteration():
            ring.append(train_iteration(ours, opt_ours, rec.batch(next_index()), 0.1, 1.0), B, 0.0)
            if ring.n == 10:
                ring.flush()

        def hand_rolled():
            idx = next_index()
            k2, k3, rot, loc = (host[k][idx].to(dev, non_blocking=True) for k in keys)
            loss, cls, reg, z = gmw_train_step(theirs, opt_theirs, k2, k3, rot, loc, 0.1, 1.0)
            mae = ((z - loc[:, 2]).abs() / loc[:, 2]).mean()
            for j, v in enumerate((loss, cls, reg, mae)):
                state["meters"][j] += v.item()

        for _ in range(3):
            loop_iteration()
            hand_rolled()
        res = alternate((loop_iteration, hand_rolled), reps, 10)
        lines.append("  B %2d: train_gmw's iteration %7.2f (%.2f, %.2f) | gmw_train_step + .item() meters %7.2f (%.2f, %.2f) | %.2fx"
                     % (B, res[0][0] * 1e3, res[0][1] * 1e3, res[0][2] * 1e3, res[1][0] * 1e3, res[1][1] * 1e3, res[1][2] * 1e3,
                        res[1][0] / res[0][0]))
        del ours, theirs, opt_ours, opt_theirs, rec
        torch.cuda.empty_cache()


def trace_child(what):
    import torch
    from dcd_amd import ops
    dev = torch.device("cuda:0")
    if what == "empty8":
        M, args = torch.full((8, N_EDGES, N_EDGES), 0.7, device=dev), (1e-3, 100)
    else:
        M, args = distances(int(what[4:]), 0.05, dev), (0.0, 30)
    r, c = marginals(M)
    for _ in range(4):
        ops.sinkhorn(M, r, c, LMBDA, *args)
    torch.cuda.synchronize()


def kernel_times(what):
    """{kernel family: [ns, ...]} from the child's kernel trace, or a reason."""
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not found"
    tmp = tempfile.mkdtemp()
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", tmp, "-o", "gmw_train", "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", what]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        if run.returncode != 0:                                              # nothing more is started on a device that may have faulted
            raise SystemExit("the traced child '%s' exited with %d: %s" % (what, run.returncode, run.stdout[-600:]))
        rows = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    for fam in KERNELS:
                        if fam in r["Kernel_Name"]:
                            rows.setdefault(fam, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        return rows, "ok" if rows else "no kernel of csrc/transport.hip in the trace"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def report_kernels(lines):
    lines.append("3. kernels of csrc/transport.hip (rocprofv3 --kernel-trace, 4 calls each; median us per launch, launches)")
    for what, title in (("work8", "B 8, 30 working iterations"), ("work16", "B 16, 30 working iterations"),
                        ("empty8", "B 8, constant distances: 1 working iteration, 99 empty")):
        rows, why = kernel_times(what)
        lines.append("  %s: %s" % (title, why))
        if not rows:
            continue
        B = 16 if what == "work16" else 8
        plan_bytes = B * N_EDGES * N_EDGES * 4
        for fam in KERNELS:
            ns = rows.get(fam)
            if not ns:
                continue
            us = statistics.median(ns) / 1e3
            note = ""
            if what != "empty8" and fam in ("sinkhorn_sweep", "sinkhorn_gibbs", "sinkhorn_scale"):
                moved = plan_bytes * (1 if fam == "sinkhorn_sweep" else 2)
                note = "   %d MB of plans %s = %.2f TB/s" % (plan_bytes // 1000000, "read once" if fam == "sinkhorn_sweep" else "read and written",
                                                             moved / (us * 1e-6) / 1e12)
            lines.append("    %-18s %9.1f us x %4d   (min %.1f, max %.1f, sum per call %.1f us)%s"
                         % (fam, us, len(ns), min(ns) / 1e3, max(ns) / 1e3, sum(ns) / 4e3, note))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmw_train.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", default=None)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.trace_child)
    lines = ["Training GMW on the GPU (MI355X): medians of %d alternating repetitions" % a.reps]
    trace = []
    if not a.no_trace:
        report_kernels(trace)                                              # children first: this process has not opened the GPU yet
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_gmw_train.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    time_sinkhorn(lines, a.reps, dev)
    time_loop(lines, a.reps, dev)
    text = "\n".join(lines + (trace or ["3. kernel trace skipped (--no-trace)"])) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
