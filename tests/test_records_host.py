"""GMW's training records from csrc/records_math.h compiled for the HOST (tests/host/host_records.cpp: the three launches of
csrc/records.hip in plain loops) against the reference's own `Loss_Computation.gen_data` fixture (tests/golden/gen_data.npz), the
compaction rules on hand-made masks, and the wire format of `TrainRecordCollector.gen_data` against the dict `Loss_Computation`
builds on the same batches.  The GPU build of the same header is checked in test_gpu_gmw_collect.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import records_refs as R  # noqa: E402
from test_host_golden import load  # noqa: E402

KEYS5 = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "pred_location")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("host_records"))


@pytest.fixture()
def host_collect(monkeypatch, host_lib):
    """`TrainRecordCollector` on host tensors: the host build in place of the library's entry point (test-only; the product
    module has no CPU path and raises on host tensors)."""
    from dcd_amd.gmw import collect
    monkeypatch.setattr(collect, "_entry", R.host_entry(host_lib))
    return collect


def test_the_product_module_has_no_cpu_path():
    from dcd_amd import _lib
    from dcd_amd.gmw import collect
    with pytest.raises(_lib.DcdHipError):
        collect._entry("cpu")


def test_host_build_matches_the_reference_fixture(host_collect):
    """The five arrays on the pinned loss inputs against the fixture the reference's `Loss_Computation` wrote: shapes and
    `img_idx` order equal, each key within 2e-5 * max(|ref|.max(), 1) (the bar test_host_golden holds the op-by-op CPU path to),
    kpts_3d bit-equal to the gathered channels."""
    g = load("gen_data")
    _, pois, targets = R.fixture_batch()
    col = host_collect.TrainRecordCollector(R.small_cfg(), "cpu", capacity=80, max_calls=1)
    col.add(pois, targets, torch.arange(2, dtype=torch.int32))
    gd = col.gen_data()
    assert list(gd.keys()) == list(g["keys"])
    assert gd["weight_img"] == [] and len(gd["kpts_2d"]) == 1
    assert list(gd["img_idx"][0]) == list(g["img_idx"])
    for k in KEYS5:
        got, ref = np.array(gd[k][0], np.float32), g[k]
        assert got.shape == ref.shape, k
        err = np.abs(got - ref).max()
        print("%s: %.3e of %.3e" % (k, err, 2e-5 * max(np.abs(ref).max(), 1.0)))
        assert err <= 2e-5 * max(np.abs(ref).max(), 1.0), k
    mask = torch.stack([t.get_field("reg_mask") for t in targets]).reshape(-1).bool()
    sl = slice(col.spec["ch_kpts3d"], col.spec["ch_kpts3d"] + 3 * 73)
    want = pois.reshape(-1, pois.shape[-1])[mask][:, sl].reshape(-1, 73, 3).numpy()
    assert R.bit_equal(col.finish().tables[1].numpy(), want)
    rec = col.finish()
    assert len(rec) == int(mask.sum()) and [tuple(t.shape[1:]) for t in rec.tables] == [(73, 2), (73, 3), (1,), (3,)]
    assert col.images().tolist() == [b for b in range(2) for _ in range(int(targets[b].get_field("reg_mask").sum()))]
    got = rec.batch([len(rec) - 1, 0])                                  # `ResidentRecords.batch` on adopted tables: the rows asked for
    assert all(torch.equal(g, t[[len(rec) - 1, 0]]) for g, t in zip(got, rec.tables))


# ---- compaction rules ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_runs(host_lib):
    """B -> (batch, records of ALL B * 40 slots in slot order): a record depends on its own slot and on image 0's intrinsics only,
    so every masked run below must reproduce a subset of these rows bit for bit."""
    out = {}
    entry = R.host_entry(host_lib)("cpu")
    for B in (2, 3):
        batch = R.seeded_batch(B, seed=B)
        tab = R.Tables(B * R.M, "cpu", n_calls=1)
        assert R.raw_call(entry, batch, tab, B * R.M, 0, "cpu") == 0
        got = tab.host()
        assert got["cursor"].tolist() == [0, B * R.M] and got["per_call"].tolist() == [B * R.M]
        assert all(np.isfinite(got[k]).all() and not (got[k] == R.POISON).any() for k in KEYS5)
        out[B] = (batch, got)
    return out


def expect_rows(full, mask, numbers):
    sel = np.flatnonzero(mask.reshape(-1).numpy())
    want = {k: full[k][sel] for k in KEYS5}
    want["image"] = numbers.numpy()[sel // R.M]
    return sel, want


@pytest.mark.parametrize("case", sorted(R.hand_masks()))
def test_compaction_on_hand_made_masks(host_lib, full_runs, case):
    mask = R.hand_masks()[case]
    B = mask.shape[0]
    batch, full = full_runs[B]
    batch = dict(batch, reg_mask=mask)
    rows = B * R.M
    tab = R.Tables(rows, "cpu", n_calls=1)
    assert R.raw_call(R.host_entry(host_lib)("cpu"), batch, tab, rows, 0, "cpu") == 0
    got = tab.host()
    sel, want = expect_rows(full, mask, batch["image_numbers"])
    n = len(sel)
    assert got["cursor"].tolist() == [0, n] and got["per_call"].tolist() == [n]
    for k in KEYS5:
        assert R.bit_equal(got[k][:n], want[k]), k                     # ascending (b, m) order, each record its slot's
        assert (got[k][n:] == R.POISON).all(), k
    assert got["image"][:n].tolist() == want["image"].tolist() and (got["image"][n:] == -1).all()
    # image 0's intrinsics normalise every object, whether image 0 owns one or not: back to pixels with row 0 of the table
    a = R.default_args(B)
    pois = batch["reg_pois"].reshape(-1, R.C)[sel].numpy()
    kp = pois[:, a.ch_kpts2d:a.ch_kpts2d + 2 * R.NK].reshape(n, R.NK, 2)
    centre = (batch["target_centers"].reshape(-1, 2)[sel].numpy().astype(np.float32) + batch["offset_3D"].reshape(-1, 2)[sel].numpy())
    pix = (kp + centre[:, None, :]) * np.float32(4) - batch["pad_size"].numpy()[sel // R.M].astype(np.float32)[:, None, :]
    c0 = batch["calib"][0].numpy()
    np.testing.assert_allclose(got["kpts_2d"][:n], (pix - c0[:2]) / c0[2:4], rtol=1e-6, atol=1e-6)


def test_second_call_appends_and_both_counts_are_kept(host_lib, full_runs):
    masks = R.hand_masks()
    first, second = masks["empty image in the middle"], masks["image 0 empty"]
    batch, full = full_runs[3]
    entry = R.host_entry(host_lib)("cpu")
    tab = R.Tables(32, "cpu", n_calls=2)
    assert R.raw_call(entry, dict(batch, reg_mask=first), tab, 32, 0, "cpu") == 0
    numbers2 = batch["image_numbers"] + 1000
    assert R.raw_call(entry, dict(batch, reg_mask=second, image_numbers=numbers2), tab, 32, 1, "cpu") == 0
    got = tab.host()
    _, w1 = expect_rows(full, first, batch["image_numbers"])
    _, w2 = expect_rows(full, second, numbers2)
    n1, n2 = len(w1["image"]), len(w2["image"])
    assert (n1, n2) == (6, 4)
    assert got["per_call"].tolist() == [n1, n2]
    assert got["cursor"].tolist() == [n1 + n2, n1]                     # call 1 read cursor[1] and wrote cursor[0]
    for k in KEYS5:
        assert R.bit_equal(got[k][:n1], w1[k]) and R.bit_equal(got[k][n1:n1 + n2], w2[k]), k
        assert (got[k][n1 + n2:] == R.POISON).all(), k
    assert got["image"][:n1 + n2].tolist() == w1["image"].tolist() + w2["image"].tolist()


def test_capacity_below_the_count(host_lib, full_runs):
    """cap = 5 of the 42 records: the first five are written, rows >= cap keep their poison, the cursor shows the true count."""
    mask = R.hand_masks()["all 40 slots of one image"]
    batch, full = full_runs[2]
    tab = R.Tables(12, "cpu", n_calls=1)
    assert R.raw_call(R.host_entry(host_lib)("cpu"), dict(batch, reg_mask=mask), tab, 5, 0, "cpu") == 0
    got = tab.host()
    _, want = expect_rows(full, mask, batch["image_numbers"])
    assert got["cursor"].tolist() == [0, 42] and got["per_call"].tolist() == [42]
    for k in KEYS5:
        assert R.bit_equal(got[k][:5], want[k][:5]), k
        assert (got[k][5:] == R.POISON).all(), k
    assert (got["image"][5:] == -1).all()


def test_argument_errors_of_the_host_build(host_lib, full_runs):
    batch, _ = full_runs[2]
    entry = R.host_entry(host_lib)("cpu")
    tab = R.Tables(8, "cpu", n_calls=1)
    bad = []
    for field, value in (("nk", 1), ("nk", 129), ("n_bins", 5), ("ch_kpts3d", R.C - 3 * R.NK + 1), ("ch_offset", -1), ("B", 0), ("M", 0)):
        a = R.default_args(2)
        setattr(a, field, value)
        bad.append(R.raw_call(entry, batch, tab, 8, 0, "cpu", args=a, workspace=torch.empty(1 << 22, dtype=torch.uint8)))
    bad.append(R.raw_call(entry, batch, tab, 0, 0, "cpu"))              # cap < 1
    bad.append(R.raw_call(entry, batch, tab, 8, 1, "cpu"))              # call outside [0, n_calls)
    assert bad == [1] * len(bad)
    assert R.raw_call(entry, batch, tab, 8, 0, "cpu", workspace=torch.empty(64, dtype=torch.uint8)) == 2
    got = tab.host()
    assert all((got[k] == R.POISON).all() for k in KEYS5) and got["per_call"].tolist() == [-1]


# ---- the wire format -------------------------------------------------------------------------------------------------------
def test_collector_refuses_what_the_header_does_not_cover():
    from dcd_amd.gmw.collect import records_spec
    with pytest.raises(NotImplementedError, match="multi-bin"):
        records_spec(R.small_cfg("cpu", "INPUT.ORIENTATION", "head-axis"))
    with pytest.raises(NotImplementedError, match="CORNER_LOSS_DEPTH"):
        records_spec(R.small_cfg("cpu", "MODEL.HEAD.CORNER_LOSS_DEPTH", "direct"))


def test_gen_data_of_two_calls_is_the_dict_of_the_loss(cpu_backend, host_collect, tmp_path):
    """`gen_data()` of a two-call collection against the dict `Loss_Computation` builds on the same two batches on the CPU: the
    same keys, the same nesting by iteration, the same `img_idx` strings, `weight_img` empty, values within the fixture bar."""
    import json
    from dcd_amd.engine.gen_data import dump_gen_data, dump_gen_data_train
    from dcd_amd.gmw.data import load_train_data
    from dcd_amd.model.head.detector_loss import Loss_Computation
    from dcd_amd.structures.params_3d import stack_field
    preds, pois, targets = R.fixture_batch()
    # the second batch: the two images in the other order, so image 0's intrinsics -- and with them every kpts_2d -- change
    cls2 = torch.from_numpy(preds["cls"]).flip(0).contiguous()
    reg2 = torch.from_numpy(preds["reg"]).flip(0).contiguous()
    targets2 = targets[::-1]
    pois2 = cpu_backend.select_point_of_interest(2, stack_field(targets2, "target_centers"), reg2)
    lc = Loss_Computation(R.small_cfg("cpu", "TEST.GENERATE_GMW", True))
    with torch.no_grad():
        lc({"cls": torch.from_numpy(preds["cls"]), "reg": torch.from_numpy(preds["reg"])}, list(targets))
        lc({"cls": cls2, "reg": reg2}, list(targets2))
    want = lc.gen_data
    col = host_collect.TrainRecordCollector(R.small_cfg(), "cpu", capacity=64, max_calls=2)
    col.add(pois, targets, torch.tensor([0, 1], dtype=torch.int32))
    col.add(pois2, targets2, torch.tensor([1, 0], dtype=torch.int32))
    got = col.gen_data()
    assert list(got.keys()) == list(want.keys()) and got["weight_img"] == want["weight_img"] == []
    assert got["img_idx"] == want["img_idx"] and len(got["img_idx"]) == 2
    for k in KEYS5:
        assert len(got[k]) == len(want[k]) == 2
        for it in range(2):
            a, b = np.array(got[k][it], np.float32), np.array(want[k][it], np.float32)
            assert a.shape == b.shape, (k, it)
            assert np.abs(a - b).max() <= 2e-5 * max(np.abs(b).max(), 1.0), (k, it)
    # the file, on request: the sibling of `dump_gen_data_train` writes the same layout, and GMW's reader takes it
    path = dump_gen_data(got, str(tmp_path / "a"))
    back = json.load(open(path))
    assert os.path.basename(path) == "gen_data_train.json" and list(back.keys()) == list(got.keys())
    ref_path = dump_gen_data_train(lc, str(tmp_path / "b"))
    a, b = load_train_data(path), load_train_data(ref_path)
    rec = col.finish()
    for i, k in enumerate(("kpts_2d", "kpts_3d", "pred_rot", "gt_location")):
        assert a[k].shape == b[k].shape
        assert R.bit_equal(a[k], rec.tables[i].numpy()), k             # float32 -> JSON -> float32 is the identity


def test_do_train_takes_the_keyword_with_generate_gmw_only(tmp_path):
    from dcd_amd.engine.train import do_train
    cfg = R.small_cfg("cpu", "SOLVER.LR_WARMUP", False)
    for value in (True, "json"):
        with pytest.raises(ValueError, match="gmw_records needs TEST.GENERATE_GMW"):
            do_train(cfg, torch.nn.Linear(1, 1), None, None, None, [], {"iteration": 0}, str(tmp_path), gmw_records=value)
    assert os.listdir(tmp_path) == []
