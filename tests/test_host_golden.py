"""Host-side logic (cfg, registries, anno encoder, predictor, loss, post-processor, whole KeypointDetector) against
fixtures produced by the reference's own Python (tests/golden/make_golden.py).  Runs on the CPU by patching the
oracle in for the HIP entry points (conftest.cpu_backend) -- the product code itself has no CPU path."""
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi

G = os.path.join(os.path.dirname(__file__), "golden")
LOSS_KEYS = ['hm_loss', 'bbox_loss', 'dims_loss', 'orien_loss', 'offset_loss', 'trunc_offset_loss', 'corner_loss',
             'depth_loss', 'keypoint_loss', 'extra_kpts_2d_loss', 'extra_kpts_3d_loss', 'extra_kpts_depth_loss',
             'keypoint_depth_loss']


def load(name):
    return np.load(os.path.join(G, name + ".npz"), allow_pickle=False)


def small_cfg(device="cpu"):
    from dcd_amd.config import get_cfg
    return get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", device, "MODEL.USE_SYNC_BN", False,
                         "INPUT.WIDTH_TRAIN", 320, "INPUT.HEIGHT_TRAIN", 96])


def check_anno_encoder(device):
    from dcd_amd.model.anno_encoder import Anno_Encoder
    g = load("anno_encoder")
    enc = Anno_Encoder(small_cfg(str(device)))
    d = gi.anno_inputs()
    t = {k: torch.from_numpy(v).to(device) for k, v in d.items() if k != "P_img"}
    calibs = gi.ref_like_calibs(d["P_img"])
    def close(a, key, tol=1e-5):
        np.testing.assert_allclose(a.detach().cpu().numpy(), g[key], rtol=tol, atol=tol, err_msg=key)
    close(enc.encode_box3d(t["rotys"], t["dims"], t["locs"]), "encode_box3d")
    close(enc.decode_depth(t["depth_off"], None), "decode_depth")
    close(enc.decode_dimension(t["cls"], t["dims_off"]), "decode_dimension")
    close(enc.decode_location_flatten(t["points"], t["offsets"], t["depths"], calibs, t["pad"], t["batch_idxs"]),
          "decode_location", 2e-5)
    close(enc.decode_depth_from_keypoints_batch(t["kp10"], t["dims"], calibs, t["batch_idxs"]), "kp_depths", 2e-5)
    ro, al = enc.decode_axes_orientation(t["ori"].clone(), t["locs"])
    close(ro, "rotys")
    close(al, "alphas")
    close(enc.decode_kpts_2d_img(t["kp73"], t["points"], t["offsets"],
                                 t["pad"][t["batch_idxs"]].unsqueeze(1).expand_as(t["kp73"])), "kpts_2d_img")


def check_loss_computation(device, tol, through_row_kernel=False):
    """The reference's Loss_Computation fixture (13 losses, log dict, gradients w.r.t. both head maps).
    through_row_kernel: hand the loss what the predictor hands it in training -- the regression map gathered at the object
    centres, `reg_pois` (B, M, 415) -- so that the per-object rows run through csrc/loss_rows.hip (GPU only) instead of the
    op-by-op rows; the gradient flows back through the gather into the dense map and is compared with the same fixture."""
    from dcd_amd.model.head.detector_loss import Loss_Computation
    g = load("loss_computation")
    preds, targets = gi.loss_inputs()
    cls = torch.from_numpy(preds["cls"]).to(device).requires_grad_()
    reg = torch.from_numpy(preds["reg"]).to(device).requires_grad_()
    targets = [t.to(device) for t in targets]
    loss = Loss_Computation(small_cfg(str(device)))
    if through_row_kernel:
        assert loss.fused_rows, "the row kernel is switched off (DCD_LOSS_ROWS)"
        cx = torch.stack([t.get_field("target_centers") for t in targets]).long()
        bidx = torch.arange(cx.shape[0], device=cx.device).view(-1, 1).expand(-1, cx.shape[1])
        predictions = {"cls": cls, "reg": None, "reg_pois": reg[bidx, :, cx[:, :, 1], cx[:, :, 0]]}      # B x M x 415
    else:
        predictions = {"cls": cls, "reg": reg}
    loss_dict, log = loss(predictions, targets)
    assert list(loss_dict.keys()) == LOSS_KEYS
    for k in LOSS_KEYS:
        ref = float(g["loss_" + k])
        assert abs(float(loss_dict[k]) - ref) <= tol * max(abs(ref), 1e-3), (k, float(loss_dict[k]), ref)
    for k in log:
        if k == "3D_IoU":      # the fixture's value comes through a stand-in for shapely: not reference-pinned
            continue
        ref = float(g["log_" + k])
        assert abs(log[k] - ref) <= tol * max(abs(ref), 1e-3), ("log " + k, log[k], ref)
    assert set("log_" + k for k in log) == set(k for k in g.files if k.startswith("log_"))
    sum(loss_dict.values()).backward()
    def rel(a, ref):
        return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-12)
    assert rel(cls.grad.cpu().numpy(), g["grad_cls"]) <= tol
    assert rel(reg.grad.sum(1).cpu().numpy(), g["grad_reg_sum_c"]) <= tol
    assert rel(reg.grad.abs().sum((0, 2, 3)).cpu().numpy(), g["grad_reg_abs_per_channel"]) <= tol
    # ... and on each value's own scale.  The per-channel sums span 8.1e-4 (a 2d_dim channel) to 1.57 (corner_uncertainty) and
    # 42 % of the heat-map gradient's cells lie below 1e-4 of its maximum: one scale per tensor lets a 7-20 % error in the box
    # regression gradient and any error in those cells pass.  The op-by-op rows on the CPU deviate by at most 2.2e-7 per channel
    # and are bit-equal in grad_cls.  The figures of a run are printed below (pytest -s).
    from grad_scales import assert_close_by_element
    ref_c = torch.from_numpy(g["grad_reg_abs_per_channel"])
    ref_cls = torch.from_numpy(g["grad_cls"])
    assert (ref_c != 0).all() and (ref_cls != 0).all()
    w_c = assert_close_by_element(reg.grad.abs().sum((0, 2, 3)), ref_c, tol, torch.zeros_like(ref_c), "grad_reg_abs_per_channel, each channel")
    w_cls = assert_close_by_element(cls.grad, ref_cls, tol, torch.zeros_like(ref_cls), "grad_cls, each cell")
    print("check_loss_computation(%s): worst per-channel %.2e, worst grad_cls cell %.2e (of |ref|)" % (device, w_c * tol, w_cls * tol))


def check_model(device, tol, gtol, truth="model_96x320", loss_tol=None, decode_tol=2e-2, decode_min_match=0.8, sparse_tol=1e-4,
                grads_out=None):
    """Whole KeypointDetector vs a fixture of the reference's run: `truth` = "model_96x320" (the reference in fp32 on the CPU)
    or "model_96x320_f64" (the reference in float64: the exact result up to ~1e-12).  tol: activations; loss_tol: the 13
    losses (default tol); gtol: per-parameter gradient norms, relative to the norm (floored at 1e-4 of the largest)."""
    from dcd_amd.model.detector import KeypointDetector
    g = load(truth)
    loss_tol = tol if loss_tol is None else loss_tol
    model = KeypointDetector(small_cfg(str(device))).to(device)
    assert list(model.state_dict().keys()) == list(load("model_96x320")["state_keys"]), "state_dict keys / order must equal the reference's"
    gi.name_hashed_init(model)
    model.train()
    images, targets = gi.model_inputs()
    images = images.to(device)
    targets = [t.to(device) for t in targets]
    feats = model.backbone(images)
    model.heads.predictor.sparse_training_heads = False      # the reference's dense training output, for the map slices
    pred = model.heads.predictor(feats, targets)
    model.heads.predictor.sparse_training_heads = True       # default: heads evaluated at the object centres only
    sparse = model.heads.predictor(feats, targets)
    assert sparse["reg"] is None
    cx = torch.stack([t.get_field("target_centers") for t in targets]).long()
    bidx = torch.arange(cx.shape[0], device=cx.device).view(-1, 1).expand(-1, cx.shape[1])
    dense_at = pred["reg"][bidx, :, cx[:, :, 1], cx[:, :, 0]]                       # B x M x 415
    # (sparse_tol: in mixed precision the dense trunks run their 3x3 products in bf16, the trunks at listed positions in fp32)
    assert (sparse["reg_pois"] - dense_at).abs().max().item() <= sparse_tol * max(dense_at.abs().max().item(), 1.0)
    assert (sparse["cls"] - pred["cls"]).abs().max().item() <= max(1e-5, sparse_tol * 0.1)
    def rel(a, key):
        a = a.detach().cpu().numpy()
        return np.abs(a - g[key]).max() / (np.abs(g[key]).max() + 1e-12)
    assert rel(feats[:, :4, ::6, ::16], "feat_slice") <= tol
    assert rel(pred["cls"][:, :, ::4, ::8], "cls_slice") <= tol
    assert rel(pred["reg"][:, ::25, ::6, ::16], "reg_slice") <= tol
    assert rel(pred["reg"].abs().mean((0, 2, 3)), "reg_abs") <= tol
    gi.name_hashed_init(model)
    model.zero_grad()
    loss_dict, log = model(images, targets)
    for k in LOSS_KEYS:
        ref = float(g["loss_" + k])
        assert abs(float(loss_dict[k]) - ref) <= loss_tol * max(abs(ref), 1e-3), (k, float(loss_dict[k]), ref)
    sum(loss_dict.values()).backward()
    names = list(g["param_names"])
    norms = dict(zip(names, g["grad_norms"]))
    worst, worst_name = 0.0, None
    for n, p in model.named_parameters():
        ref = norms[n]
        got = 0.0 if p.grad is None else float(p.grad.double().norm())
        # norms below 1e-4 of the largest are compared on that absolute scale: the biases that sit in front of a BatchNorm have
        # an exactly zero gradient, and what fp32 leaves there (1e-7 .. 4e-6 here) is summation-order noise, different every run
        dev_ = abs(got - ref) / max(ref, 1e-4 * max(norms.values()))
        if dev_ > worst:
            worst, worst_name = dev_, n
    if grads_out is not None:                                  # name -> gradient, for comparisons between two runs of this check
        grads_out.update({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    if os.environ.get("DCD_TEST_PRINT_GRAD_DEV"):
        print("worst gradient-norm deviation %.3e at %s" % (worst, worst_name))
    assert worst <= gtol, "per-parameter gradient norms deviate by %.3e (%s)" % (worst, worst_name)
    g = load("model_96x320")                                   # BN buffers and the eval decode: fp32 fixture only
    np.testing.assert_allclose(model.backbone.base.base_layer[1].running_mean.cpu().numpy(), g["bn_running_mean_sample"],
                               rtol=1e-4, atol=1e-6)
    # eval decode
    model.eval()
    model.heads.post_processor.det_threshold = 0.0
    with torch.no_grad():
        result, eval_utils, _ = model(images[:1], targets[:1])
    ref = g["eval_result"]
    assert tuple(result.shape) == ref.shape
    got = result.cpu().numpy()
    # This is the MODEL-level decode: the heat map comes out of ~90 layers, rows are sorted by score and at random initialisation
    # many scores are nearly equal, so the order (and the last few members) of the top-50 move with fp32 round-off of the conv
    # back end: rows are matched by their 2-D box and compared at `decode_tol` of each column's range (the fused depth divides by
    # exp(uncertainty) of a random net: round-off in the maps is amplified).  The decode itself is pinned exactly -- row order,
    # every column at 1e-4 -- on fixed predictor maps by check_post_processor (CPU and GPU).
    scale = np.abs(ref).max(0) + 1e-6
    matched = 0
    for row in got:
        d = np.abs(ref[:, 2:6] - row[None, 2:6]).max(1)
        j = int(d.argmin())
        if d[j] <= 0.5 and (np.abs(row - ref[j]) / scale).max() <= decode_tol:
            matched += 1
    # 80 %: on the GPU 44-46 of the 50 rows match depending on the run (which of the nearly-equal scores make the cut)
    assert matched >= decode_min_match * len(ref), "only %d of %d decoded rows match the reference" % (matched, len(ref))
    # TEST.GENERATE_GMW eval pass -> gen_data_infer.json records (DGDE/engine/inference.py:59-84)
    from dcd_amd.engine.gen_data import infer_records
    model.heads.post_processor.generate_data = True
    with torch.no_grad():
        result_g, _, vis_g = model(images[:1], targets[:1])
    recs = infer_records(result_g, vis_g)
    assert len(recs) == g["gen_result"].shape[0]
    assert set(recs[0]) == {'kpts_2d', 'kpts_3d', 'pred_rot', 'box', 'dim', 'pred_location', 'score', 'cat'}
    ref_box, matched = g["gen_result"][:, 2:6], 0
    for r in recs:
        d = np.abs(ref_box - np.array(r['box'])[None]).max(1)
        j = int(d.argmin())
        k2, k3 = g["gen_kpts_2d"][j], g["gen_kpts_3d"][j]
        if (d[j] <= 0.5 and np.abs(np.array(r['kpts_2d']) - k2).max() <= decode_tol * (np.abs(k2).max() + 1e-6)
                and np.abs(np.array(r['kpts_3d']) - k3).max() <= decode_tol * (np.abs(k3).max() + 1e-6)):
            matched += 1
    assert matched >= decode_min_match * len(recs), "only %d of %d GMW inference records match the reference" % (matched, len(recs))


def check_post_processor(device, tol=1e-4):
    """`PostProcessor.forward` (detector_infer.py:86-213) fed with PINNED predictor outputs (image 0 of the loss_inputs() maps)
    against the reference's own output on them: row for row in the reference's order (scores are continuous random values --
    no ties among the top-50), every KITTI column, the raw scores, the fused-depth diagnostics, the decoded key-points and
    the GMW inference records.  `tol` is relative to each column's range in the reference."""
    from dcd_amd.engine.gen_data import infer_records
    from dcd_amd.model.head.detector_infer import make_post_processor
    g = load("post_processor")
    preds, targets = gi.loss_inputs()
    pp = make_post_processor(small_cfg(str(device)))
    assert pp.det_threshold == float(g["threshold"])
    cls = torch.from_numpy(preds["cls"][:1]).to(device)
    reg = torch.from_numpy(preds["reg"][:1]).to(device)
    tg = [targets[0].to(device)]
    with torch.no_grad():
        rows, info, vis = pp({"cls": cls, "reg": reg}, tg)
    ref = g["result"]
    assert tuple(rows.shape) == ref.shape
    got = rows.cpu().numpy()
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])                       # class ids (fractional, utils.py:91)
    scale = np.abs(ref).max(0) + 1e-6
    err = np.abs(got - ref) / scale
    assert err.max() <= tol, "decoded rows deviate: column %d by %.3e" % (int(err.max(0).argmax()), err.max())

    def close(a, key, t=tol):
        a = a.detach().cpu().numpy().reshape(g[key].shape)
        assert np.abs(a - g[key]).max() <= t * (np.abs(g[key]).max() + 1e-6), key
    close(info["vis_scores"], "vis_scores", 1e-6)
    close(info["uncertainty_conf"], "uncertainty_conf")
    close(info["estimated_depth_error"], "estimated_depth_error")
    close(vis["keypoints"], "keypoints", 1e-6)
    close(vis["proj_center"], "proj_center", 1e-6)
    close(vis["pred_extra_kpts_2d"], "pred_extra_kpts_2d", 1e-6)
    close(vis["pred_extra_kpts_3d"], "pred_extra_kpts_3d", 1e-6)
    np.testing.assert_array_equal(vis["min_uncertainty"].cpu().numpy(), g["min_uncertainty"])
    pp.generate_data = True
    with torch.no_grad():
        rows_g, _, vis_g = pp({"cls": cls, "reg": reg}, tg)
    assert torch.equal(rows_g, rows)
    close(vis_g["gen_pred_extra_kpts_2d"], "gen_kpts_2d", 1e-6)
    close(vis_g["gen_pred_extra_kpts_3d"], "gen_kpts_3d", 1e-6)
    recs = infer_records(rows_g, vis_g)
    assert len(recs) == ref.shape[0]
    for j in (0, 7, 49):
        assert np.abs(np.array(recs[j]["box"]) - ref[j, 2:6]).max() <= tol * scale[2:6].max()
        assert np.abs(np.array(recs[j]["kpts_2d"]) - g["gen_kpts_2d"][j]).max() <= 1e-6 * np.abs(g["gen_kpts_2d"]).max()


def check_gen_data(device, tol):
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.gen_data import dump_gen_data_train
    from dcd_amd.model.head.detector_loss import Loss_Computation
    g = load("gen_data")
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(device), "INPUT.WIDTH_TRAIN", 320, "INPUT.HEIGHT_TRAIN", 96,
                        "TEST.GENERATE_GMW", True])
    preds, targets = gi.loss_inputs()
    lc = Loss_Computation(cfg)
    with torch.no_grad():
        lc({"cls": torch.from_numpy(preds["cls"]).to(device), "reg": torch.from_numpy(preds["reg"]).to(device)},
           [t.to(device) for t in targets])
    gd = lc.gen_data
    assert list(gd.keys()) == list(g["keys"])
    for k in ("kpts_2d", "kpts_3d", "pred_rot", "gt_location", "pred_location"):
        got, ref = np.array(gd[k][0], np.float32), g[k]
        assert got.shape == ref.shape, k
        assert np.abs(got - ref).max() <= tol * max(np.abs(ref).max(), 1.0), k
    assert list(gd["img_idx"][0]) == list(g["img_idx"])
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = dump_gen_data_train(lc, d)
        back = json.load(open(path))
        assert set(back.keys()) == set(gd.keys()) and len(back["kpts_2d"][0][0]) == 73


def test_cfg_and_registry():
    from dcd_amd.config import get_cfg
    from dcd_amd.model import registry
    import dcd_amd.model.head.detector_predictor  # noqa: F401  (registers Base_Predictor)
    cfg = get_cfg()
    assert cfg.MODEL.HEAD.PREDICTOR in registry.PREDICTOR
    assert sum(c for grp in cfg.MODEL.HEAD.REGRESSION_CHANNELS for c in grp) == 415
    assert cfg.DATASETS.MAX_OBJECTS == 40 and cfg.TEST.DETECTIONS_PER_IMG == 50 and cfg.MODEL.BATCH_WEIGHT_FACTOR == 18
    with pytest.raises(KeyError):
        cfg.merge_from_list(["MODEL.NOT_A_KEY", 1])


def test_anno_encoder_matches_reference(cpu_backend):
    check_anno_encoder(torch.device("cpu"))


def test_loss_computation_matches_reference(cpu_backend):
    check_loss_computation(torch.device("cpu"), 2e-5)


def test_nonfinite_logging_metric_does_not_poison_the_losses(cpu_backend, monkeypatch):
    """Advisor r2: the 13 losses leave as M (rc * columns); a NaN in a logging-only column (3-D IoU of a degenerate box) has a zero
    row in M, but 0 * NaN = NaN -- the metric columns are zeroed out of the product, the losses stay those of the fixture."""
    from dcd_amd.model.head import detector_loss
    from dcd_amd.model.head.detector_loss import Loss_Computation
    g = load("loss_computation")
    preds, targets = gi.loss_inputs()
    real = detector_loss.get_iou_3d
    monkeypatch.setattr(detector_loss, "get_iou_3d", lambda a, b: real(a, b) * float("nan"))
    loss_dict, log = Loss_Computation(small_cfg("cpu"))({"cls": torch.from_numpy(preds["cls"]), "reg": torch.from_numpy(preds["reg"])},
                                                        list(targets))
    for k in LOSS_KEYS:
        ref = float(g["loss_" + k])
        assert abs(float(loss_dict[k]) - ref) <= 2e-5 * max(abs(ref), 1e-3), (k, float(loss_dict[k]), ref)
    assert bool(torch.isfinite(loss_dict.total))


def test_gen_data_for_gmw_matches_reference(cpu_backend):
    check_gen_data(torch.device("cpu"), 2e-5)


def test_post_processor_matches_reference(cpu_backend):
    check_post_processor(torch.device("cpu"), 1e-5)


def test_solver_schedule_and_step_match_reference(tmp_path):
    """learning-rate trace over 3000 iterations (cosine warm-up, then step decay, stepped with the absolute
    iteration like the reference's loop), bias parameters at twice the rate, three AdamW steps, checkpoint round trip."""
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, checkpoint_state, load_checkpoint_state, step_schedulers
    g = load("solver")
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "SOLVER.LR_WARMUP", True, "SOLVER.WARMUP_STEPS", 200,
                        "SOLVER.MAX_ITERATION", 3000, "SOLVER.STEPS", (2000, 2600)])
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    opt = build_optimizer(net, cfg)
    sched, warm = build_scheduler(opt, cfg)
    x = torch.linspace(-1, 1, 24).reshape(4, 6)
    lw, lb = [], []
    for it in range(3000):
        if it < 3:
            opt.zero_grad()
            net(x).square().sum().backward()
            opt.step()
        step_schedulers(sched, warm, it, cfg)
        lw.append(opt.param_groups[0]["lr"])       # ours: group 0 = weights, group 1 = biases
        lb.append(opt.param_groups[1]["lr"])
    np.testing.assert_allclose(np.array(lw), g["lr_weight"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.array(lb), g["lr_bias"], rtol=1e-12, atol=0)
    got = np.concatenate([p.detach().numpy().ravel() for p in net.parameters()])
    np.testing.assert_allclose(got, g["params_after_3_steps"], rtol=2e-6, atol=1e-7)
    # checkpoint layout round trip
    path = tmp_path / "model_checkpoint.pth"
    live = {id(st): dict(st) for st in opt.state.values()}
    ck = checkpoint_state(net, opt, sched, iteration=2999, iter_per_epoch=100)
    for st in opt.state.values():                          # the running optimizer's state objects are not replaced ...
        assert all(v is live[id(st)][k] for k, v in st.items())
    for i, st in ck["optimizer"]["state"].items():         # ... and the checkpoint holds copies, not the live tensors
        assert all(not any(v is w for w in l.values()) for l in live.values() for v in st.values() if torch.is_tensor(v))
    torch.save(ck, path)
    data = torch.load(path, weights_only=False)
    assert set(data) == {"model", "optimizer", "scheduler", "iteration", "iter_per_epoch"}
    net2 = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    opt2 = build_optimizer(net2, cfg)
    sched2, _ = build_scheduler(opt2, cfg)
    extra = load_checkpoint_state(data, net2, opt2, sched2)
    assert extra == {"iteration": 2999, "iter_per_epoch": 100}
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]


def _reference_checkpoint_from_fixture(g, net):
    """The 'optimizer' / 'scheduler' entries a reference checkpoint holds after iteration 2 (one group per parameter), rebuilt
    from tests/golden/solver.npz -- the values were saved by the reference's own solver package (make_golden.golden_solver)."""
    n = int(g["n_groups"])
    groups = [{"lr": float(g["ckpt_group_lr"][i]), "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": float(g["ckpt_group_wd"][i]),
               "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
               "decoupled_weight_decay": True, "initial_lr": float(g["ckpt_group_initial_lr"][i]),
               "params": [int(v) for v in g["ckpt_group_params"][i]]} for i in range(n)]
    state = {i: {"step": torch.tensor(float(g["ckpt_step"][i])), "exp_avg": torch.from_numpy(g["ckpt_exp_avg_%d" % i].copy()),
                 "exp_avg_sq": torch.from_numpy(g["ckpt_exp_avg_sq_%d" % i].copy())} for i in range(n)}
    sched = {"base_lrs": list(map(float, g["ckpt_sched_base_lrs"])), "last_epoch": int(g["ckpt_sched_last_epoch"]),
             "_last_lr": list(map(float, g["ckpt_sched_last_lr"])), "_step_count": 1, "_is_initial": False, "lr_lambdas": [None] * n}
    flat = torch.from_numpy(g["params_after_3_steps"].copy())
    model_sd, o = {}, 0
    for k, v in net.state_dict().items():
        model_sd[k] = flat[o:o + v.numel()].reshape(v.shape).clone()
        o += v.numel()
    return {"model": model_sd, "optimizer": {"state": state, "param_groups": groups}, "scheduler": sched, "iteration": 2,
            "iter_per_epoch": 100}


def test_reference_checkpoint_resumes_here_and_ours_resumes_there():
    """the reference saves one optimizer group per parameter (solver/__init__.py:10-25); ours pools weights and
    biases.  A reference checkpoint must load (SOLVER.LOAD_OPTIMIZER_SCHEDULER path of utils/check_point.py) and continue to
    the same weights, and what we write must have the reference's layout, value for value."""
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, checkpoint_state, load_checkpoint_state
    g = load("solver")
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "SOLVER.LR_WARMUP", True, "SOLVER.WARMUP_STEPS", 200,
                        "SOLVER.MAX_ITERATION", 3000, "SOLVER.STEPS", (2000, 2600)])
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    opt = build_optimizer(net, cfg)
    sched, _ = build_scheduler(opt, cfg)
    ref_ckpt = _reference_checkpoint_from_fixture(g, net)
    extra = load_checkpoint_state(ref_ckpt, net, opt, sched)
    assert extra == {"iteration": 2, "iter_per_epoch": 100}
    assert len(opt.param_groups) == 2 and [len(gr["params"]) for gr in opt.param_groups] == [2, 2]
    assert opt.param_groups[0]["lr"] == float(g["ckpt_group_lr"][0]) and opt.param_groups[1]["lr"] == float(g["ckpt_group_lr"][1])
    # (a) the reference's 4th step, taken by our optimizer from the loaded state
    x = torch.linspace(-1, 1, 24).reshape(4, 6)
    opt.zero_grad()
    net(x).square().sum().backward()
    opt.step()
    got = np.concatenate([p.detach().numpy().ravel() for p in net.parameters()])
    np.testing.assert_allclose(got, g["params_after_4_steps"], rtol=2e-6, atol=1e-7)
    # (b) what we write has the reference's layout: reload the fixture state, write it back out, compare entry by entry
    net2 = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    opt2 = build_optimizer(net2, cfg)
    sched2, _ = build_scheduler(opt2, cfg)
    load_checkpoint_state(_reference_checkpoint_from_fixture(g, net2), net2, opt2, sched2)
    out = checkpoint_state(net2, opt2, sched2, iteration=2, iter_per_epoch=100)
    n = int(g["n_groups"])
    assert len(out["optimizer"]["param_groups"]) == n
    for i, gr in enumerate(out["optimizer"]["param_groups"]):
        assert gr["params"] == [int(v) for v in g["ckpt_group_params"][i]]
        assert gr["lr"] == float(g["ckpt_group_lr"][i]) and gr["initial_lr"] == float(g["ckpt_group_initial_lr"][i])
        assert gr["weight_decay"] == float(g["ckpt_group_wd"][i]) and tuple(gr["betas"]) == (0.9, 0.99)
        st = out["optimizer"]["state"][i]
        assert float(st["step"]) == float(g["ckpt_step"][i])
        np.testing.assert_array_equal(st["exp_avg"].numpy(), g["ckpt_exp_avg_%d" % i])
        np.testing.assert_array_equal(st["exp_avg_sq"].numpy(), g["ckpt_exp_avg_sq_%d" % i])
    assert out["scheduler"]["base_lrs"] == list(map(float, g["ckpt_sched_base_lrs"]))
    assert out["scheduler"]["_last_lr"] == list(map(float, g["ckpt_sched_last_lr"]))
    # (c) a stock per-parameter AdamW (the reference's construction) loads our 'optimizer' entry as it is
    ref_like = torch.optim.AdamW([{"params": [p], "lr": 1.0} for p in net2.parameters()], betas=(0.9, 0.99))
    ref_like.load_state_dict(out["optimizer"])
    assert [gr["lr"] for gr in ref_like.param_groups] == [float(v) for v in g["ckpt_group_lr"]]


def test_calibration_table_follows_values_not_object_identity():
    """a loader builds new Calibration objects per batch and CPython recycles their addresses; the cached device
    table must follow the intrinsics."""
    from dcd_amd.config import get_cfg
    from dcd_amd.model.anno_encoder import Anno_Encoder

    class Calib:
        def __init__(self, f):
            self.c_u, self.c_v, self.f_u, self.f_v, self.b_x, self.b_y = 600.0, 170.0, f, f, 0.06, 0.0003
    enc = Anno_Encoder(get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu"]))
    seen = []
    for f in (700.0, 710.0, 720.0, 730.0):
        batch = [Calib(f)]
        seen.append(float(enc._calib_table(batch, torch.device("cpu"))[0, 2]))
        del batch
    assert seen == [700.0, 710.0, 720.0, 730.0]


def test_float64_model_equals_reference_float64(cpu_backend):
    """The reference model run in float64 (tests/golden/model_96x320_f64.npz: stock convs in double + the f64 build of the
    oracle as `_ext`; make_golden.golden_model_f64) against OUR model shell run the same way: with round-off out of the
    picture the two must agree to ~1e-12 -- the tightest pin of the DLA-34 / IDAUp / predictor wiring there is.  It is also
    the ground truth that the fp32 tolerances of the GPU test are measured against (tests/test_gpu_golden.py)."""
    from dcd_amd.model.detector import KeypointDetector
    g = load("model_96x320_f64")
    model = KeypointDetector(small_cfg("cpu"))
    gi.name_hashed_init(model)
    model = model.double().train()
    images, targets = gi.model_inputs()
    feats = model.backbone(images.double())
    model.heads.predictor.sparse_training_heads = False
    pred = model.heads.predictor(feats, targets)

    def rel(a, key):
        return np.abs(a.detach().numpy() - g[key]).max() / (np.abs(g[key]).max() + 1e-300)
    assert rel(feats[:, :4, ::6, ::16], "feat_slice") <= 1e-12
    assert rel(pred["cls"][:, :, ::4, ::8], "cls_slice") <= 1e-6          # float32 outputs (detector_predictor.py:203)
    assert rel(pred["reg"][:, ::25, ::6, ::16], "reg_slice") <= 1e-6
    # how far the reference's own fp32 run (model_96x320.npz) sits from the exact result: the yardstick for the GPU bars
    f32 = load("model_96x320")
    d = {k: np.abs(f32[k] - g[k]).max() / np.abs(g[k]).max() for k in ("feat_slice", "cls_slice", "reg_slice")}
    assert max(d.values()) <= 5e-5, d


def test_whole_model_matches_reference(cpu_backend):
    check_model(torch.device("cpu"), 2e-4, 2e-3)


def test_product_ops_refuse_cpu_tensors():
    """No silent CPU fallback: every HIP-backed entry point raises on CPU tensors."""
    from dcd_amd import ops, _ext, _lib
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(_lib.DcdHipError):
        ops.focal_loss(x, x)
    with pytest.raises(_lib.DcdHipError):
        ops.nms_hm(x)
    with pytest.raises(RuntimeError):
        _ext.dcn_v2_forward(x, torch.zeros(1, 1, 3, 3), torch.zeros(1), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4),
                            3, 3, 1, 1, 1, 1, 1, 1, 1)


def test_config_tree_equals_the_reference(tmp_path=None):
    """dcd_amd/config (defaults + the DGDE run tables of dgde_run.py) against the reference's merged tree, key by key
    (tests/golden/cfg.json, written by make_golden.golden_config from config/defaults.py + runs/DGDE.yaml)."""
    import json
    import os
    from dcd_amd.config import get_cfg
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg.json")))

    def flat(node, prefix=""):
        out = {}
        for k, v in node.items():
            if isinstance(v, dict):
                out.update(flat(v, prefix + k + "."))
            else:
                out[prefix + k] = list(v) if isinstance(v, tuple) else v
        return out
    def plain(v):                                    # JSON has no tuples
        return [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    ours = {k: plain(v) for k, v in flat(get_cfg()).items()}
    assert set(ours) == set(ref), (sorted(set(ours) ^ set(ref))[:10])
    diff = {k: (ours[k], ref[k]) for k in ref if ours[k] != ref[k] and k != "PATHS_CATALOG"}      # a machine-specific path
    assert not diff, diff


def test_stack_field_is_zero_copy_for_collated_targets():
    """structures.params_3d.stack_field: consecutive slices of one batched tensor come back as that tensor (no copy); anything
    else is stacked as before."""
    from dcd_amd.structures.params_3d import ParamsList, collate_fields, stack_field
    ts = []
    for i in range(3):
        t = ParamsList((1280, 384))
        t.add_field("a", torch.full((4, 2), float(i)))
        t.add_field("n", torch.tensor(i))
        t.add_field("name", "img%d" % i)
        ts.append(t)
    plain = stack_field(ts, "a")
    assert plain.shape == (3, 4, 2) and plain.data_ptr() != ts[0].get_field("a").data_ptr()
    collate_fields(ts)
    for name in ("a", "n"):
        s1 = stack_field(ts, name)
        assert s1.data_ptr() == ts[0].get_field(name).data_ptr() and s1.shape[0] == 3
        assert torch.equal(s1, torch.stack([t.get_field(name) for t in ts]))
    assert ts[2].get_field("name") == "img2"
    # a reordered list is not one tensor's consecutive slices: copy
    rev = stack_field(ts[::-1], "a")
    assert rev.data_ptr() != ts[2].get_field("a").data_ptr() and torch.equal(rev[0], ts[2].get_field("a"))
