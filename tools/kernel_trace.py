"""The traced child of the timing tools: a fresh process of a tool's own file under `rocprofv3 --kernel-trace --stats`, and its
kernel statistics."""
import csv
import glob
import os
import subprocess
import sys


def traced_child(script, mode, work, timeout):
    """{kernel name: (calls, total us)} of a child process running `python SCRIPT --once MODE`; its trace goes to
    `<work>/trace_<mode>`.  timeout: seconds the child may take."""
    tdir = os.path.join(work, "trace_" + mode)
    os.makedirs(tdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", mode, "--output-format", "csv", "--",
           sys.executable, os.path.abspath(script), "--once", mode]
    r = subprocess.run(cmd, cwd=tdir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
    found = {}
    for path in glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            calls, total = found.get(row["Name"], (0, 0.0))
            found[row["Name"]] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]) / 1e3)
    return found
