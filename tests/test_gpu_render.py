"""The renderer on the device (csrc/render.hip, `ops.render_detections` / `ops.render_primitives`, `inference(render_dir=...)`):
bit for bit against the host build of the same header on the exact hand-made cases of tests/render_cases.py; on the seeded scenes
the integer table against the kernel's own float ends, the canvas against the restatement's raster of THAT table, the float
ends against float64 at four times the host build's recorded distance; the canvas in a poisoned, guarded buffer; two runs the
same bytes; and the public route, whose pictures must be the op's and whose result files must not change."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import render_cases as C  # noqa: E402
import render_refs as R  # noqa: E402
import test_render_host as H  # noqa: E402
from arena import Arena  # noqa: E402
from test_gpu_dcd_eval import world  # noqa: E402,F401  (the fixture directory and an initialised detector: module-scoped)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_render(tmp_path_factory):
    return H.build_host_render(tmp_path_factory.mktemp("host_render_gpu"))


def canvas_in(arena, B, in_h, in_w):
    nbytes = B * in_h * (in_w + in_h) * 3
    assert nbytes % 4 == 0
    return arena.scratch(nbytes, "canvas").view(B, in_h, in_w + in_h, 3)


def run_device(case, cuda, poison=True):
    """`ops.render_detections` on a case, the float inputs and the canvas between guards: (canvas, table, counts, ends) on the host."""
    from dcd_amd import ops
    arena = Arena(cuda, poison=poison)
    B = len(case["frames"])
    sizes = [f.shape[1::-1] for f in case["frames"]]
    rows = arena.place(torch.from_numpy(np.ascontiguousarray(case["rows"], np.float32)), "rows")
    aux = arena.place(torch.from_numpy(np.ascontiguousarray(case["aux"], np.float32)), "aux")
    tab = arena.place(torch.from_numpy(C.image_table(case["P"], sizes, case["in_h"], case["in_w"])), "image_table")
    k2 = arena.place(torch.from_numpy(case["k2"]), "k2") if case["k2"] is not None else None
    gt = None
    if case["gt"] is not None:
        d, l, r, m = case["gt"]
        gt = (arena.place(torch.from_numpy(d), "gt_dims"), arena.place(torch.from_numpy(l), "gt_locs"),
              arena.place(torch.from_numpy(r), "gt_rotys"), torch.from_numpy(m).to(cuda))
    staged = ops.stage_frames(case["frames"], cuda)
    canvas = canvas_in(arena, B, case["in_h"], case["in_w"])
    out, (table, counts, ends) = ops.render_detections(staged, rows, aux, k2, None, tab, gt, case["K"], case["det"], case["vis"],
                                                       keypoints=case["keypoints"], want_table=True, canvas=canvas)
    assert out.data_ptr() == canvas.data_ptr()
    arena.check("render_detections")
    return canvas.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy(), ends.cpu().numpy()


@pytest.mark.parametrize("name", sorted(C.HAND_MADE))
def test_device_equals_the_host_build_on_exact_cases(cuda, host_render, name):
    case = C.HAND_MADE[name]()
    canvas, table, counts, ends = run_device(case, cuda)
    want_canvas, want_table, want_counts, want_ends = H.run_host(host_render, case)
    assert np.array_equal(table, want_table), "integer table: first difference at %s" % (np.argwhere(table != want_table)[:1],)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(canvas, want_canvas), "%d canvas bytes differ" % (canvas != want_canvas).sum()
    assert np.array_equal(ends, want_ends, equal_nan=True), "the exact cases' float ends are the host build's"
    again = run_device(case, cuda, poison=False)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((canvas, table, counts, ends), again)), "two runs differ"


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_seeded_scenes(cuda, name):
    case = C.SCENES[name]()
    canvas, table, counts, ends = run_device(case, cuda)
    want_table, want_counts, want = H.run_ref(case)[1:]
    # every slot of every image takes part in each comparison
    assert np.array_equal(table[:, :, 1], want_table[:, :, 1]), "drawn / not drawn differs from the restatement"
    assert (table[:, :, 1] >= 0).sum() > 3000
    assert np.array_equal(counts, want_counts)
    segments = table[:, :, 1] == 0
    assert np.array_equal(table[:, :, 2:6][segments], np.trunc(ends[segments]).astype(np.int32)), "table != trunc(the kernel's own ends)"
    assert np.array_equal(table[~segments], want_table[~segments]), "glyphs and empty slots are integer from the start"
    assert np.array_equal(table[:, :, [0, 6, 7, 8, 9, 10, 11]], want_table[:, :, [0, 6, 7, 8, 9, 10, 11]])
    assert np.array_equal(canvas, R.raster(case["frames"], table, counts, case["in_h"], case["in_w"])), "canvas != the raster of the kernel's table"
    assert np.isfinite(ends).all()
    worst = float(np.abs(ends.astype(np.float64) - want).max())
    bar = 4 * C.HOST_ENDS_DISTANCE[name]
    print("device, %s scene, float ends: worst distance from float64 %.4e px (bar %.4e = 4 x the host build's)" % (name, worst, bar))
    assert worst <= bar
    again = run_device(case, cuda, poison=False)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((canvas, table, counts, ends), again)), "two runs differ"


@pytest.mark.parametrize("name", sorted(C.TABLES) + ["octants reversed"])
def test_render_primitives(cuda, host_render, name):
    from dcd_amd import ops
    table, counts = C.table_octants(True) if name == "octants reversed" else C.TABLES[name]()
    frames = C.frames_of(C.SIZES, seed=1)
    arena = Arena(cuda)
    dev_table = arena.place(torch.from_numpy(table), "table")
    dev_counts = arena.place(torch.from_numpy(counts), "counts")
    canvas = canvas_in(arena, len(frames), C.IN_H, C.IN_W)
    ops.render_primitives(ops.stage_frames(frames, cuda), dev_table, dev_counts, C.IN_H, C.IN_W, canvas=canvas)
    arena.check("render_primitives")
    got = canvas.cpu().numpy()
    assert np.array_equal(got, H.run_host_primitives(host_render, frames, table, counts))
    assert np.array_equal(got, R.raster(frames, table, counts, C.IN_H, C.IN_W))
    if name == "octants reversed":
        assert np.array_equal(got, H.run_host_primitives(host_render, frames, *C.table_octants(False))), "a -> b must equal b -> a"


def test_a_table_that_does_not_fit_is_refused(cuda):
    from dcd_amd import _lib, ops
    assert ops.render_slots(40, 50, 73) == 17 * 40 + 50 * 101 and ops.render_slots(40, 128, 128) == -1
    K, nk = 128, 128
    frames = C.frames_of(((150, 33),))
    rows, aux = torch.zeros((K, 14), device=cuda), torch.zeros((K, 4), device=cuda)
    tab = torch.from_numpy(C.image_table(C.intrinsics(1), [(150, 33)])).to(cuda)
    with pytest.raises(_lib.DcdHipError, match="status 1"):
        ops.render_detections(ops.stage_frames(frames, cuda), rows, aux, torch.zeros((K, nk, 2), device=cuda), None, tab, None, K, 0.2, 0.25,
                              keypoints=True, in_h=C.IN_H, in_w=C.IN_W)
    with pytest.raises(ValueError, match="records=True"):
        ops.render_detections(ops.stage_frames(frames, cuda), rows, aux, None, None, tab, None, K, 0.2, 0.25, keypoints=True,
                              in_h=C.IN_H, in_w=C.IN_W)


def test_a_record_outside_the_buffer_draws_nothing(cuda):
    """A frame record that points past the staged buffer (or past the canvas) is an all-zero picture, not a read."""
    from dcd_amd import ops
    table, counts = C.table_thickness()
    frames = C.frames_of(C.SIZES, seed=1)
    staged = ops.stage_frames(frames, cuda)
    rec = staged[:80].view(torch.int64).view(2, 5)
    rec[0, 0] = staged.numel() - 100                                       # offset + h * pitch runs past the end
    rec[1, 3] = C.IN_W + 1                                                 # wider than the canvas
    got = ops.render_primitives(staged, torch.from_numpy(table).to(cuda), torch.from_numpy(counts).to(cuda), C.IN_H, C.IN_W).cpu().numpy()
    assert not got.any()


# ---- the public route ------------------------------------------------------------------------------------------------------
def _pictures(folder, ids):
    from PIL import Image
    assert sorted(os.listdir(folder)) == [i + ".png" for i in ids]
    return {i: np.asarray(Image.open(os.path.join(folder, i + ".png"))) for i in ids}


def _results(folder, ids):
    assert sorted(os.listdir(folder)) == [i + ".txt" for i in ids]
    return {i: open(os.path.join(folder, i + ".txt"), "rb").read() for i in ids}


class _Spy:
    """`ops.render_detections` with every call's inputs and canvas kept (clones: the pass lets its tensors go)."""

    def __init__(self, ops):
        self.original, self.calls = ops.render_detections, []

    def __call__(self, frames, rows, aux, k2, k3, table, gt, K, det, vis, **kw):
        canvas, _ = self.original(frames, rows, aux, k2, k3, table, gt, K, det, vis, **kw)
        keep = lambda t: None if t is None else t.clone()  # noqa: E731
        self.calls.append(dict(frames=keep(frames), rows=keep(rows), aux=keep(aux), k2=keep(k2), table=keep(table),
                               gt=None if gt is None else tuple(keep(t) for t in gt), K=K, det=det, vis=vis, kw=dict(kw),
                               canvas=canvas.cpu().numpy()))
        return canvas, None


def _same_tables(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same_tables(a[k], b[k])
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("keypoints", [False, True])
def test_inference_leaves_the_ops_pictures_and_the_same_files(world, tmp_path, monkeypatch, keypoints):  # noqa: F811
    from dcd_amd import ops
    from dcd_amd.engine.inference import inference
    ids = world["ids"]
    monkeypatch.setitem(world["model"].cfg.TEST, "VISUALIZE_THRESHOLD", -1.0)   # a fresh detector's confidences are ~0: draw every kept row
    plain = inference(world["model"], world["files"], world["pipe"], str(tmp_path / "plain"), batch_size=3)
    spy = _Spy(ops)
    monkeypatch.setattr(ops, "render_detections", spy)
    drawn = inference(world["model"], world["files"], world["pipe"], str(tmp_path / "drawn"), batch_size=3, render_dir=str(tmp_path / "png"),
                      render_keypoints=keypoints)
    monkeypatch.setattr(ops, "render_detections", spy.original)
    assert _results(str(tmp_path / "drawn" / "data"), ids) == _results(str(tmp_path / "plain" / "data"), ids)
    _same_tables(drawn, plain)
    pictures = _pictures(str(tmp_path / "png"), ids)
    assert [c["rows"].shape[0] for c in spy.calls] == [150, 50], "batches of 3 and 1 images"
    n = 0
    for call in spy.calls:
        assert call["kw"].get("keypoints", False) is keypoints and (call["k2"] is not None or not keypoints) and call["gt"] is not None
        canvas, (table, _, _) = spy.original(call["frames"], call["rows"], call["aux"], call["k2"], None, call["table"], call["gt"], call["K"],
                                             call["det"], call["vis"], want_table=True, **call["kw"])
        assert np.array_equal(canvas.cpu().numpy(), call["canvas"])
        rec = call["frames"][:40 * canvas.shape[0]].view(torch.int64).view(-1, 5).cpu().numpy()
        for b in range(canvas.shape[0]):
            h, w = int(rec[b, 2]), int(rec[b, 3])
            picture = pictures[ids[n]]
            assert picture.shape == (h, w + h, 3) and np.array_equal(picture, call["canvas"][b, :h, :w + h]), ids[n]
            kinds = table[b, :, 1].cpu().numpy()
            print("%s: %d x %d, %d primitives drawn, %d pixels of the frame changed" % (
                ids[n], w, h, (kinds >= 0).sum(), (picture[:, :w] != np.asarray(world["files"].frame(n))).any(-1).sum()))
            assert (kinds >= 0).sum() >= 50 * (28 + (73 if keypoints else 0)) - 50 * 19, "every kept row draws (its far box may miss the panel)"
            n += 1
    assert n == len(ids)


def test_suppressed_rows_leave_no_pixel(world, tmp_path, monkeypatch):  # noqa: F811
    from dcd_amd import ops
    from dcd_amd.engine.inference import inference
    from test_gpu_nms import _nms
    monkeypatch.setitem(world["model"].cfg.TEST, "VISUALIZE_THRESHOLD", -1.0)
    spy = _Spy(ops)
    monkeypatch.setattr(ops, "render_detections", spy)
    with _nms(world, "3d", 0.42, False):
        inference(world["model"], world["files"], world["pipe"], str(tmp_path / "out"), batch_size=3, render_dir=str(tmp_path / "png"))
    monkeypatch.setattr(ops, "render_detections", spy.original)
    suppressed = 0
    for call in spy.calls:
        aux, K = call["aux"], call["K"]
        gone = torch.isinf(aux[:, 0]) & (aux[:, 0] < 0)
        suppressed += int(gone.sum())
        _, (table, _, _) = spy.original(call["frames"], call["rows"], call["aux"], None, None, call["table"], call["gt"], K, call["det"],
                                        call["vis"], want_table=True, **call["kw"])
        B, M = call["rows"].shape[0] // K, call["gt"][0].shape[1]
        kinds = table[:, 17 * M:, 1].reshape(B, K, 28).flip(1).reshape(B * K, 28)        # (image, rank) order
        assert (kinds[gone] < 0).all() and (kinds[~gone & (aux[:, 0] >= call["det"])] >= 0).any(1).all()
        only = call["aux"].clone()
        only[gone, 0] = float("nan")                                       # the same batch without the suppressed rows at all
        rows = call["rows"].clone()
        rows[gone] = float("nan")
        canvas, _ = spy.original(call["frames"], rows, only, None, None, call["table"], call["gt"], K, call["det"], call["vis"], **call["kw"])
        assert np.array_equal(canvas.cpu().numpy(), call["canvas"])
    assert suppressed > 0, "the NMS of the fixture suppresses rows (test_gpu_nms.py)"


def test_without_a_render_dir_nothing_is_rendered_or_kept(world, tmp_path, monkeypatch):  # noqa: F811
    from dcd_amd import ops
    from dcd_amd.data import batches
    from dcd_amd.engine.inference import inference
    calls = []
    monkeypatch.setattr(ops, "render_detections", lambda *a, **k: calls.append("render_detections"))
    monkeypatch.setattr(ops, "render_primitives", lambda *a, **k: calls.append("render_primitives"))
    pipe = world["pipe"]
    seen = []
    original = type(pipe).__call__

    def watched(self, *a, **k):
        images, targets = original(self, *a, **k)
        seen.append((k.get("keep_frames", False), any(t.has_field("frames") for t in targets)))
        return images, targets
    monkeypatch.setattr(type(pipe), "__call__", watched)
    inference(world["model"], world["files"], pipe, str(tmp_path / "plain"), batch_size=3)
    assert calls == [] and seen and not any(k or f for k, f in seen)
    assert not os.path.exists(str(tmp_path / "png"))
    del seen[:]
    monkeypatch.undo()
    with batches.eval_batches(world["files"], pipe, 3, keep_frames=True) as walk:
        for k, indices, images, targets in walk:
            staged, rec = targets[0].get_field("frames"), targets[0].get_field("frame_records")
            assert staged.dtype == torch.uint8 and tuple(rec.shape) == (len(indices), 5) and rec.data_ptr() == staged.data_ptr()
            for b, i in enumerate(indices):
                frame = np.asarray(world["files"].frame(i))
                off, pitch, h, w, flip = (int(v) for v in rec[b].tolist())
                assert (h, w, flip) == (frame.shape[0], frame.shape[1], 0) and tuple(targets[b].get_field("frame_size").tolist()) == (w, h)
                got = staged[off:off + h * pitch].view(h, w, 3).cpu().numpy()
                assert np.array_equal(got, frame)


def test_render_dir_needs_the_fused_decode(world, tmp_path, monkeypatch):  # noqa: F811
    from dcd_amd.engine.inference import inference
    pp = world["model"].heads.post_processor

    def refuse():
        raise NotImplementedError("decode_fused: refused for the test")
    monkeypatch.setattr(pp, "decode_spec", refuse)
    with pytest.raises(NotImplementedError, match="render_dir"):
        inference(world["model"], world["files"], world["pipe"], str(tmp_path / "out"), batch_size=3, render_dir=str(tmp_path / "png"))
