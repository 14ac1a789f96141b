"""GMW inference on the GPU: objects/s of `gmw.inference.refine` against the training-loss route, and the two kernels' times.

    python tools/time_gmw_refine.py [--objects 2048] [--reps 3] [--out profiles/gmw_refine.txt] [--no-trace]

Three routes over the same 2048 seeded objects, end to end (host arrays in, refined locations back on the host):
  refine(fused=True) at batch 256 and at batch 8, and `gmw_val_step` at batch 8 -- the only way to refine without
  `gmw/inference.py`: it forms the 2628 x 2628 distance matrix and the transport plan per object, which ties it to about eight
  objects per call.
The repetitions alternate between the routes and the medians are reported.  The kernel times come from a run of their own: a
child process under `rocprofv3 --kernel-trace --stats` that refines 512 objects at batch 256 (started before this process opens
the GPU); `dcd_gmw_refine`'s two kernels stand beside the byte floor of the features they read (2 C K 4 bytes per object at
8 TB/s -- the kernel reads them twice, norms then differences).
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

HBM_BYTES_PER_S = 8e12
TRACE_OBJECTS, TRACE_BATCH = 512, 256
KERNELS = (("gmw_edge_weights", ("gmw_edge_weights",)), ("gmw_softmax_depth", ("gmw_softmax_depth",)),
           ("context_norm_fwd_row<true>", ("context_norm_fwd_row", "true")))


def seeded_data(n):
    import numpy as np
    from make_golden_gmw import inputs
    k2, k3, rot, loc = inputs(seed=11, B=n)
    rng = np.random.default_rng(12)
    dim = np.stack([rng.uniform(1.4, 1.8, n), rng.uniform(1.5, 1.9, n), rng.uniform(3.0, 4.5, n)], 1).astype(np.float32)
    return {"kpts_2d": k2, "kpts_3d": k3, "pred_rot": rot, "pred_location": loc, "dim": dim, "img_idx": [("0", i) for i in range(n)]}


def seeded_model(dev):
    import torch
    from dcd_amd.gmw import GMW
    torch.manual_seed(0)
    return GMW().to(dev).eval()


def val_step_route(model, data, dev, batch):
    """`gmw_val_step` over every record, with the same host <-> device traffic as `refine`."""
    import torch
    from dcd_amd.gmw import gmw_val_step
    out = []
    for s in range(0, len(data["img_idx"]), batch):
        k2, k3, rot, loc, dim = (torch.from_numpy(data[k][s:s + batch]).to(dev) for k in ("kpts_2d", "kpts_3d", "pred_rot",
                                                                                         "pred_location", "dim"))
        out.append(gmw_val_step(model, k2, k3, rot, loc, dim, 0.1, 1.0)[4].cpu())
    return torch.cat(out, 0)


def trace_child():
    import torch
    from dcd_amd.gmw import refine
    dev = torch.device("cuda:0")
    model, data = seeded_model(dev), seeded_data(TRACE_OBJECTS)
    for _ in range(3):
        refine(model, data, dev, batch_size=TRACE_BATCH)
    torch.cuda.synchronize()


def kernel_times(tmp):
    """{label: (calls, mean us)} from the child's kernel trace; {} with a reason when the profiler is not there."""
    if shutil.which("rocprofv3") is None:
        return {}, "rocprofv3 not found"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "gmw", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child"]
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    if run.returncode != 0:
        return {}, "rocprofv3 exited with %d: %s" % (run.returncode, run.stdout[-400:])
    rows = {}
    for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {}
    for label, parts in KERNELS:
        ns = [d for name, ds in rows.items() if all(p in name for p in parts) for d in ds]
        if ns:
            out[label] = (len(ns), statistics.median(ns) / 1e3)
    return out, "ok" if out else "no kernel of this project in the trace"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmw_refine.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        return trace_child()

    kernels, why = {}, "skipped (--no-trace)"
    if not a.no_trace:
        tmp = tempfile.mkdtemp()
        try:
            kernels, why = kernel_times(tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    import torch
    from dcd_amd.gmw import refine
    dev = torch.device("cuda:0")
    model, data = seeded_model(dev), seeded_data(a.objects)
    routes = (("refine(fused=True), batch 256", lambda d: refine(model, d, dev, batch_size=256)[1]),
              ("refine(fused=True), batch 8", lambda d: refine(model, d, dev, batch_size=8)[1]),
              ("gmw_val_step, batch 8", lambda d: val_step_route(model, d, dev, 8)))
    warm = {k: v[:512] for k, v in data.items()}
    first = [fn(warm) for _, fn in routes]                              # every shape the timed window uses, once
    torch.cuda.synchronize()
    times = [[] for _ in routes]
    for _ in range(a.reps):
        for i, (_, fn) in enumerate(routes):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(data)
            torch.cuda.synchronize()
            times[i].append(time.perf_counter() - t)

    C, K = 128, 2628
    lines = ["GMW inference, %d seeded objects, median of %d alternating repetitions (MI355X)" % (a.objects, a.reps)]
    for (name, _), ts in zip(routes, times):
        med = statistics.median(ts)
        lines.append("  %-32s %9.1f objects/s   (%.3f s; min %.3f, max %.3f)" % (name, a.objects / med, med, min(ts), max(ts)))
    base = statistics.median(times[2])
    lines.append("  speed-up over gmw_val_step: batch 256 %.1fx, batch 8 %.1fx" % (base / statistics.median(times[0]),
                                                                                base / statistics.median(times[1])))
    ref = first[2]
    for (name, _), got in zip(routes[:2], first[:2]):
        lines.append("  %-32s max relative difference of pred_location from gmw_val_step %.2e" % (
            name, ((got - ref) / ref).abs().max().item()))
    floor = 2 * C * K * 4 * TRACE_BATCH / HBM_BYTES_PER_S * 1e6
    lines.append("kernel trace (rocprofv3 --kernel-trace, %d objects at batch %d, median per launch): %s" % (TRACE_OBJECTS, TRACE_BATCH, why))
    for label, (calls, us) in kernels.items():
        note = ""
        if label == "gmw_edge_weights":
            note = "   byte floor %.1f us for one read of the features (%.0f MB at 8 TB/s); the kernel reads them twice" % (
                floor, 2 * C * K * 4 * TRACE_BATCH / 1e6)
        if label.startswith("context_norm"):
            moved = 3 * TRACE_BATCH * C * K * 4
            note = "   x, residual in and y out: %.0f MB = %.2f TB/s" % (moved / 1e6, moved / (us * 1e-6) / 1e12)
        lines.append("  %-28s %9.1f us x %d launches%s" % (label, us, calls, note))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
