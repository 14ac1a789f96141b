"""GMW inference on the host (dcd_amd/gmw/inference.py) against tests/golden/gmw_infer.npz, which was produced by running the
reference's own loader, `validate` body and result writer (tests/golden/make_golden_gmw_infer.py) on six objects in three images
plus one image without detections."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "gmw_infer.npz"))


@pytest.fixture(scope="module")
def records(fx):
    return json.loads(str(fx["records_json"]))


def test_load_infer_data_returns_the_arrays_of_the_reference_loader(fx, records):
    from dcd_amd.gmw import load_infer_data
    data = load_infer_data(records)
    for ours, theirs in (("kpts_2d", "kpts_2d"), ("kpts_3d", "kpts_3d"), ("pred_rot", "pred_rot"), ("pred_location", "gt_location"),
                         ("dim", "dim")):
        ref = fx["loader_" + theirs]
        assert data[ours].dtype == np.float32 and data[ours].shape == ref.shape, ours
        assert np.array_equal(data[ours], ref), ours
    assert data["kpts_2d"].shape[1:] == (73, 2) and data["kpts_3d"].shape[1:] == (73, 3)
    assert [(float(img), float(i)) for img, i in data["img_idx"]] == [tuple(r) for r in fx["loader_img_idx"].tolist()]
    assert data["box"].shape == (6, 4) and data["score"].shape == (6,)


def test_load_infer_data_takes_a_path_numpy_views_and_longer_keypoint_lists(tmp_path, records):
    from dcd_amd.gmw import load_infer_data
    want = load_infer_data(records)
    path = tmp_path / "gen_data_infer.json"
    path.write_text(json.dumps(records, indent=4))
    views = {}
    for img, recs in records.items():                 # what engine.gen_data.infer_records_batch yields: float32 numpy views
        views[img] = []
        for r in recs:
            v = {k: (np.asarray(r[k], np.float32) if k != "cat" else r[k]) for k in r}
            v["kpts_2d"] = np.concatenate([v["kpts_2d"], np.full((5, 2), 9.0, np.float32)], 0)      # 78 keypoints: 73 are kept
            v["kpts_3d"] = np.concatenate([v["kpts_3d"], np.full((5, 3), 9.0, np.float32)], 0)
            views[img].append(v)
    for got in (load_infer_data(str(path)), load_infer_data(views)):
        assert got["img_idx"] == want["img_idx"]
        for k in want:
            if k != "img_idx":
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_write_results_reproduces_every_result_file(tmp_path, fx, records):
    from dcd_amd.gmw import load_infer_data, write_results
    ids = [str(i) for i in fx["ids"]]
    out = write_results(load_infer_data(records), torch.from_numpy(fx["pred_location"]), str(tmp_path / "results"), ids)
    texts = [str(t) for t in fx["result_texts"]]
    assert sorted(os.listdir(out)) == [i + ".txt" for i in ids]
    for i, text in zip(ids, texts):
        with open(os.path.join(out, i + ".txt")) as f:
            assert f.read() == text, i
    assert texts[3] == "" and [t.count("\n") for t in texts] == [3, 2, 1, 0]          # the image without detections
    yaws = [float(line.split(" ")[14]) for t in texts for line in t.splitlines()]
    assert abs(yaws[1] - 3 * np.pi) < 1e-6                  # the record's yaw is -pi - 0.3: the writer's rule makes it 3 pi
    assert abs(yaws[4] - (np.pi - 0.4)) < 1e-6              # pi + 0.4 is reflected to 2 pi - yaw


def test_refine_stock_chain_meets_the_reference_on_the_cpu(fx, records):
    """fused=False in fp32 on the CPU, edge depths from the oracle's compute_z, the model seeded like the reference's."""
    from oracle import torch_ops
    from dcd_amd.gmw import GMW, load_infer_data, refine
    torch.manual_seed(0)
    model = GMW().eval()
    z, loc = refine(model, load_infer_data(records), "cpu", batch_size=4, fused=False, compute_z=torch_ops.compute_z)
    assert z.shape == (6,) and loc.shape == (6, 3) and z.dtype == torch.float32
    assert np.allclose(z.numpy(), fx["pred_depth"], rtol=2e-5, atol=0)
    assert np.allclose(loc.numpy(), fx["pred_location"], rtol=2e-5, atol=0)


def test_device_ops_refuse_cpu_tensors_and_gradients():
    from dcd_amd import ops
    from dcd_amd._lib import DcdHipError
    x = torch.zeros(1, 2, 8)
    with pytest.raises(DcdHipError):
        ops.context_norm_relu_add(x, x)
    with pytest.raises(DcdHipError):
        ops.gmw_refine(x, x, torch.zeros(1, 8), torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 3), torch.ones(1, 3))
