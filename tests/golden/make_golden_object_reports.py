"""Records what the two labelled-object reports (`engine.depth_report`, `engine.dis_iou_report`) do on the HOST, as
tests/golden/object_reports.json: `summarise` (every array by the SHA-256 of its bytes) and the exact `format_report` text (its
SHA-256; one case in full) on seeded tables, and the messages of the refusals that fire before any device work.  No GPU and no
built library are needed.

    python tests/golden/make_golden_object_reports.py

`record()` is what tests/test_object_report_host.py compares with the file, so re-running this on an unchanged host half
reproduces the file byte for byte.  The file was recorded on the commit BEFORE the two reports were given a shared module; it
holds results only."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "object_reports.json")
CLASSES = ["Car", "Pedestrian", "Cyclist"]
EDGES_3 = (0.0, 10.0, 30.0, 80.0)
CASES = (("ordinary", EDGES_3), ("a class without an object", EDGES_3), ("all zero", EDGES_3), ("non-finite only", EDGES_3),
         ("one bin", (0.0, 80.0)), ("sixteen bins", tuple(5.0 * i for i in range(17))))
FULL_TEXT = ("ordinary",)              # the printed table line by line; the other cases keep its digest only
# (statistics per cell, the index of the non-finite count) behind the (class, bin) axes
SHAPES = {"depth_report": ((10, 5), 4), "dis_iou_report": ((15, 2, 6), 5)}


def tables(report, case, edges, seed):
    """Seeded (table (3, n_bins) + the report's cell shape, float64; outside (3) int64): every cell an integer count, real sums
    and an integer non-finite count, as the accumulate kernels leave them."""
    cell, nonfinite = SHAPES[report]
    rng = np.random.RandomState(seed)
    n_bins = len(edges) - 1
    table = rng.uniform(-40.0, 40.0, (3, n_bins) + cell)
    table[..., 0] = rng.randint(1, 30, table.shape[:-1])
    table[..., nonfinite] = rng.randint(0, 3, table.shape[:-1])
    if report == "dis_iou_report":
        table[..., 1:3] = np.abs(table[..., 1:3]) / 40.0 * table[..., :1]                    # sums of IoU and IoU^2: at most the count
        table[..., 4] = rng.randint(0, 30, table.shape[:-1]) % (table[..., 0] + 1)           # loose hits <= count
        table[..., 3] = rng.randint(0, 30, table.shape[:-1]) % (table[..., 4] + 1)           # strict hits <= loose hits
    outside = rng.randint(0, 5, 3).astype(np.int64)
    if case == "a class without an object":
        table[1], outside[1] = 0.0, 0
    elif case == "all zero":
        table[:], outside[:] = 0.0, 0
    elif case == "non-finite only":
        table[0, :, 2], table[2, 1] = 0.0, 0.0                # one method / variant of a class in every bin; one bin of a class
        table[0, :, 2][..., nonfinite], table[2, 1][..., nonfinite] = 3.0, 1.0
        table[1] = 0.0                                        # a whole class: every object non-finite in every column
        table[1][..., nonfinite] = 2.0
    return table, outside


def plain(v):
    """A result value as one line: an array as its dtype, shape and the SHA-256 of its bytes (so NaN and -0.0 count by their
    bits), anything else as compact JSON."""
    if isinstance(v, np.ndarray):
        return "%s %s sha256 %s" % (v.dtype, list(v.shape), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    return json.dumps(v)


class _Stub:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def refusals(driver):
    """"<exception type>: <message>" of every refusal that fires before the model is looked at."""
    labelled, evaluation = _Stub(has_labels=True, split="val"), _Stub(is_train=False)
    calls = {"an unlabelled split": dict(files=_Stub(has_labels=False, split="test")),
             "is_train=True": dict(pipeline=_Stub(is_train=True)),
             "batch_size=0": dict(batch_size=0),
             "backbone_batch=0": dict(backbone_batch=0),
             "edges=(0, 20, 10)": dict(edges=(0, 20, 10)),
             "one edge": dict(edges=(5,)),
             "18 edges": dict(edges=tuple(range(18)))}
    out = {}
    for name, change in calls.items():
        args = dict(model=object(), files=labelled, pipeline=evaluation)
        args.update(change)
        try:
            driver(**args)
            out[name] = None
        except Exception as e:  # noqa: BLE001  (the record says which)
            out[name] = "%s: %s" % (type(e).__name__, e)
    return out


def record(full_text=FULL_TEXT):
    from dcd_amd.engine import depth_report as DR
    from dcd_amd.engine import dis_iou_report as DI
    thresholds = DI.default_thresholds(len(CLASSES))
    out = {}
    for report, module, driver in (("depth_report", DR, DR.depth_report), ("dis_iou_report", DI, DI.dis_iou_report)):
        cases = {}
        for seed, (case, edges) in enumerate(CASES):
            table, outside = tables(report, case, edges, seed)
            extra = (thresholds,) if report == "dis_iou_report" else ()
            result = module.summarise(table, outside, edges, CLASSES, *extra)
            text = module.format_report(result)
            cases[case] = {"result": {k: plain(v) for k, v in result.items()}, "text_sha256": hashlib.sha256(text.encode()).hexdigest(),
                           "text": text.split("\n") if case in full_text else None}
        out[report] = {"cases": cases, "refusals": refusals(driver),
                       "DEFAULT_EDGES": plain(list(module.DEFAULT_EDGES)), "MAX_SLOTS": module.MAX_SLOTS}
    return out


def dump(recorded):
    return json.dumps(recorded, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(dump(record()))
    print("%s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))
