"""The host pieces of the one-pass two-stage evaluation (`engine.inference.inference(gmw=...)`): how `RecordRefiner.add` splits
a call at the buffers' capacity, and the writer's float64 fields taken straight from the detector's float32 rows."""
import json

import numpy as np
import pytest


def _brute(n_new, filled, cap):
    """One record at a time: (index in the call, position in the buffers, the buffers are full after it)."""
    out = []
    for i in range(n_new):
        out.append((i, filled, filled + 1 == cap))
        filled = (filled + 1) % cap
    return out


@pytest.mark.parametrize("cap", [1, 3, 64])
def test_plan_packs_against_one_record_at_a_time(cap):
    from dcd_amd.gmw.inference import plan_packs
    for filled in range(cap):
        for n_new in range(3 * cap + 2):
            pieces = plan_packs(n_new, filled, cap)
            want = _brute(n_new, filled, cap)
            at, pos, flat = 0, filled, []
            for start, count, flush in pieces:
                assert start == at and count >= 1                      # in order, nothing empty
                assert pos + count <= cap                              # no piece crosses the capacity
                assert flush == (pos + count == cap)                   # a flush exactly when the buffers become full
                flat += [(start + i, pos + i, flush and i == count - 1) for i in range(count)]
                at, pos = at + count, (pos + count) % cap
            assert at == n_new                                         # the pieces cover [0, n_new)
            assert flat == want, (n_new, filled, cap)
            assert sum(f for _, _, f in pieces) == (filled + n_new) // cap


def test_plan_packs_refuses_what_cannot_be():
    from dcd_amd.gmw.inference import plan_packs
    for args in ((1, 3, 3), (1, -1, 3), (-1, 0, 3), (1, 0, 0)):
        with pytest.raises(ValueError):
            plan_packs(*args)


def test_writer_fields_are_what_the_json_round_trip_gives():
    """A float32 written by `json.dumps` (through `tolist`, as `dump_gen_data_infer` does) and parsed back is the same float64,
    so `box`, `score`, `dim_out`, `rot_out` and `img_idx` from the rows equal `load_infer_data`'s from the file, exactly."""
    from dcd_amd.engine import gen_data
    from dcd_amd.engine.inference import _records
    from dcd_amd.gmw.inference import load_infer_data, writer_fields
    rng = np.random.RandomState(0)
    counts = {"000000": 3, "000001": 0, "000002": 5, "000003": 1}
    nk = 73
    infer, all_rows, all_ids = {}, [], []
    for img, n in counts.items():
        rows = (rng.randn(n, 14) * rng.choice([1e-3, 1.0, 1e3], size=(n, 14))).astype(np.float32)
        if n:
            rows[0, 13] = np.float32(1) / np.float32(3)                # digits a shorter repr would lose
        k2, k3 = rng.randn(n, nk, 2).astype(np.float32), rng.randn(n, nk, 3).astype(np.float32)
        infer[img] = _records(rows, k2, k3)
        all_rows.append(rows)
        all_ids += [img] * n
    want = load_infer_data(json.loads(json.dumps(infer, default=gen_data._json_default)))
    got = writer_fields(np.concatenate(all_rows, 0), all_ids)
    assert got["img_idx"] == want["img_idx"] and len(got["img_idx"]) == 9
    for k in ("box", "score", "dim_out", "rot_out"):
        assert got[k].dtype == np.float64 == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
    empty = writer_fields(np.zeros((0, 14), np.float32), [])
    assert empty["img_idx"] == [] and empty["box"].shape == (0, 4) and empty["rot_out"].shape == (0,)
