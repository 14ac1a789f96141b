"""The host half of the two labelled-object reports, pinned without a GPU and without the built library: `summarise` (by bits)
and the `format_report` text (by digests) on seeded tables, and the refusals that fire before any device work, against
tests/golden/object_reports.json (recorded by tests/golden/make_golden_object_reports.py before the reports shared a module);
and the command lines' `--edges` / override splitting, by hand-written anchors, through each report's `main` with everything
behind the parser replaced."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_object_reports as G  # noqa: E402

REPORTS = ("depth_report", "dis_iou_report")


@pytest.fixture(scope="module")
def recorded():
    return G.record()


@pytest.fixture(scope="module")
def golden():
    with open(G.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("report", REPORTS)
@pytest.mark.parametrize("case", [name for name, _ in G.CASES])
def test_summarise_bits_and_report_text(recorded, golden, report, case):
    got, want = recorded[report]["cases"][case], golden[report]["cases"][case]
    assert sorted(got["result"]) == sorted(want["result"])
    for k in want["result"]:
        assert got["result"][k] == want["result"][k], k                          # arrays: dtype, shape and the digest of their bytes
    assert got["text"] == want["text"]                                           # line by line where the record keeps the lines
    assert got["text_sha256"] == want["text_sha256"]


@pytest.mark.parametrize("report", REPORTS)
def test_the_cases_are_the_ones_they_are_named_for(golden, report):
    full = G.record(full_text=[case for case, _ in G.CASES])[report]["cases"]
    assert all(full[case]["text_sha256"] == golden[report]["cases"][case]["text_sha256"] for case in full)
    text = {case: "\n".join(full[case]["text"]) for case in full}
    assert all(text["ordinary"].count(c) > 0 for c in G.CLASSES)
    assert "Pedestrian" not in text["a class without an object"] and "Car" in text["a class without an object"]
    assert all(c in text["all zero"] for c in G.CLASSES) and "0.000" not in text["all zero"]     # nothing skipped, every cell `-`
    assert "Pedestrian" in text["non-finite only"]
    assert "0-80" in text["one bin"] and "75-80" in text["sixteen bins"] and "0-5" in text["sixteen bins"]


@pytest.mark.parametrize("report", REPORTS)
def test_refusals_before_any_device_work(recorded, golden, report):
    want = golden[report]["refusals"]
    assert sorted(want) == ["18 edges", "an unlabelled split", "backbone_batch=0", "batch_size=0", "edges=(0, 20, 10)", "is_train=True",
                            "one edge"]
    assert all(v is not None and v.startswith("ValueError: ") for v in want.values())
    assert recorded[report]["refusals"] == want


def test_the_whole_record_is_reproduced_byte_for_byte(recorded):
    with open(G.GOLDEN) as f:
        assert G.dump(recorded) == f.read()


# ---- the command line ----------------------------------------------------------------------------------------------------------
class _Anything:
    """Stands for the detector, the split and the pipeline: `main` only hands them on."""

    def __init__(self, *a, **k):
        pass

    def to(self, device):
        return self


def _run_main(monkeypatch, report, argv):
    """`main(argv)` of a report with the configuration, the checkpoint, the split, the pipeline and the driver replaced:
    (the override list `get_cfg` was given, the driver's keyword arguments)."""
    import importlib
    module = importlib.import_module("dcd_amd.engine." + report)
    seen = {}

    def get_cfg(opts=None, **k):
        seen["opts"] = list(opts)
        return "cfg"

    def driver(model, files, pipeline, **kwargs):
        seen["kwargs"] = kwargs
        return "the table", {"edges": kwargs["edges"]}
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr("dcd_amd.config.get_cfg", get_cfg)
    monkeypatch.setattr("dcd_amd.engine.train.resume", lambda ckpt, model: {})
    monkeypatch.setattr("dcd_amd.model.detector.KeypointDetector", _Anything)
    monkeypatch.setattr("dcd_amd.data.kitti_files.KittiFiles", _Anything)
    monkeypatch.setattr("dcd_amd.data.input_pipeline.DeviceInputPipeline", _Anything)
    monkeypatch.setattr(module, report, driver)
    text, result = module.main(["--root", "R", "--ckpt", "C"] + argv)
    assert text == "the table"
    return seen["opts"], seen["kwargs"]


@pytest.mark.parametrize("report", REPORTS)
def test_edges_end_at_the_first_token_that_is_no_number(monkeypatch, capsys, report):
    opts, kwargs = _run_main(monkeypatch, report, ["--edges", "0", "10", "20", "TEST.DETECTIONS_THRESHOLD", "0.3", "A", "B"])
    assert kwargs["edges"] == [0.0, 10.0, 20.0] and opts == ["TEST.DETECTIONS_THRESHOLD", 0.3, "A", "B"]
    assert capsys.readouterr().out == "the table\n"
    # trailing positional overrides come after the ones the edge list swallowed
    opts, kwargs = _run_main(monkeypatch, report, ["X", "1", "--edges", "0", "10", "20", "TEST.DETECTIONS_THRESHOLD", "0.3"])
    assert kwargs["edges"] == [0.0, 10.0, 20.0] and opts == ["TEST.DETECTIONS_THRESHOLD", 0.3, "X", 1]


@pytest.mark.parametrize("report", REPORTS)
def test_defaults_of_the_command_line(monkeypatch, golden, report):
    opts, kwargs = _run_main(monkeypatch, report, [])
    assert kwargs["edges"] == json.loads(golden[report]["DEFAULT_EDGES"]) == [0, 10, 20, 30, 40, 50, 60, 80] and opts == []
    assert kwargs == dict(batch_size=8, edges=kwargs["edges"], gmw=None, gmw_batch=256, workers=None, backbone_batch=1)
    _, kwargs = _run_main(monkeypatch, report, ["--backbone-batch", "0", "--batch", "3"])
    assert kwargs["backbone_batch"] is None and kwargs["batch_size"] == 3


def test_the_parser_alone():
    """`object_report.parse_args`: argv -> (the parsed arguments, the edges, the override tokens), no GPU behind it."""
    from dcd_amd.engine import object_report as OR
    parse = lambda argv: OR.parse_args("DIR HELP", "GMW HELP", "DOC", ["--root", "R", "--ckpt", "C"] + argv)  # noqa: E731
    args, edges, tokens = parse(["--edges", "0", "10", "20", "TEST.DETECTIONS_THRESHOLD", "0.3", "A", "B"])
    assert edges == [0.0, 10.0, 20.0] and tokens == ["TEST.DETECTIONS_THRESHOLD", "0.3", "A", "B"]
    args, edges, tokens = parse(["X", "1", "--edges", "0", "1e1", "K", "V"])
    assert edges == [0.0, 10.0] and tokens == ["K", "V", "X", "1"]
    args, edges, tokens = parse(["--backbone-batch", "0"])
    assert edges == list(OR.DEFAULT_EDGES) and tokens == [] and args.backbone_batch == 0 and args.output_dir is None
    assert (args.root, args.split, args.ckpt, args.batch, args.workers, args.gmw_ckpt, args.gmw_batch) == ("R", "val", "C", 8, None, None, 256)
