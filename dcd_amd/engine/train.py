"""The training loop: the counterpart of the reference's `do_train` (DGDE/engine/trainer.py:69-232) over the pieces in
engine/trainer.py (step, schedule, checkpoint layout), data/batches.py (batch sources) and engine/inference.py (evaluation).

    arguments = resume(path, model, optimizer, scheduler)            # or {"iteration": 0}
    arguments = do_train(cfg, model, optimizer, scheduler, warmup_scheduler, batches, arguments, output_dir,
                         step=None, log_every=10, val=None, val_batch_size=1)

What it keeps of the reference: the iteration range, `step_schedulers` with the iteration number BEFORE the increment (:152-155),
the meters of DGDE/utils/metric_logger.py (window 20: median and global average) and the log line (:177-195), the checkpoint
names and the `last_checkpoint` file of `Checkpointer.save` (DGDE/utils/check_point.py:31-49, :132-135), written by rank 0
only, and the collection pass of `TEST.GENERATE_GMW` (:97-98, :114-116, :127-129, :208-221).

What it does differently:
  * no synchronisation per iteration.  The reference's `meters.update(**log_loss_dict)` reads every logged value on the host in
    every iteration.  Here the values of an iteration are appended, device to device, to a small ring (under a graphed step:
    before the next replay overwrites them); every `log_every` iterations and at the last one ONE copy brings the ring to the
    host and the meters receive every iteration's values in order, so medians and averages are those of the reference.  A
    non-finite loss is reported then (`FloatingPointError`, as `LazyLogDict` raises it); the weights are protected by the
    step's own guard in the meantime.
  * `batches.get(iteration)` instead of a data loader: batch k is a function of k (data/batches.py), so a resumed run goes on
    with the batches an uninterrupted one would have had.
  * it returns `arguments` instead of calling `exit()` (:232); no tensorboard writer."""
import datetime
import logging
import os
import time
from collections import deque

import torch

from dcd_amd.engine import gen_data
from dcd_amd.engine.passes import parse_overrides, restored_modes
from dcd_amd.engine.trainer import checkpoint_state, load_checkpoint_state, step_schedulers, train_step
from dcd_amd.utils import comm


class SmoothedValue:
    """A series of values: the last `window_size` of them for `value` / `median` / `avg`, all of them for `global_avg`
    (metric_logger.py:8-42)."""

    def __init__(self, window_size=20):
        self.deque = deque(maxlen=window_size)
        self.total = 0.0
        self.count = 0

    def update(self, value):
        self.deque.append(value)
        self.count += 1
        self.total += value

    @property
    def value(self):
        return self.deque[-1]

    @property
    def median(self):
        return torch.tensor(list(self.deque)).median().item()

    @property
    def avg(self):
        return torch.tensor(list(self.deque)).mean().item()

    @property
    def global_avg(self):
        return self.total / self.count


class MetricLogger:
    def __init__(self, delimiter=" ", window_size=20):
        self.meters, self.delimiter, self.window_size = {}, delimiter, window_size

    def __getitem__(self, name):
        if name not in self.meters:
            self.meters[name] = SmoothedValue(self.window_size)
        return self.meters[name]

    def update(self, **kwargs):
        for k, v in kwargs.items():
            self[k].update(v.item() if torch.is_tensor(v) else v)

    def update_block(self, names, rows):
        """Several iterations at once, oldest first: `rows[i][j]` is the value of `names[j]` in the block's i-th iteration."""
        for row in rows:
            for k, v in zip(names, row):
                self[k].update(v)

    def __str__(self):
        return self.delimiter.join("%s: %.4f (%.4f)" % (name, m.median, m.global_avg) for name, m in self.meters.items())


class _LogRing:
    """`log_every` rows of logged values, kept where the step left them until `flush` copies them to the host in one go.
    What an iteration costs: ONE device-to-device copy of the step's packed log values into the ring's row, and one more of
    the learning rate where that is a device tensor (`build_optimizer` on the GPU: the schedulers fill it in place, the value
    lives there); a learning rate that is a Python float stays in a host list."""

    def __init__(self, rows):
        self.rows, self.names, self.loss_keys, self.buf, self.n = rows, None, (), None, 0
        self.host_lr = []

    def append(self, log_loss_dict, lr):
        unread = log_loss_dict.unread() if hasattr(log_loss_dict, "unread") else None
        if unread is not None:
            names, row, loss_keys = unread
        else:
            names, loss_keys = list(log_loss_dict), ()
            vals = [log_loss_dict[k] for k in names]
            like = next((v for v in vals if torch.is_tensor(v)), torch.zeros(()))
            row = torch.stack([v.detach().to(like.device, torch.float32).reshape(()) if torch.is_tensor(v)
                               else torch.tensor(float(v), dtype=torch.float32, device=like.device) for v in vals])
        if self.buf is None:
            self.names, self.loss_keys = list(names), tuple(loss_keys)
            self.buf = torch.zeros((self.rows, len(self.names) + 1), dtype=torch.float32, device=row.device)
        elif list(names) != self.names:
            raise ValueError("the logged names changed during the run: %s -> %s" % (self.names, list(names)))
        self.buf[self.n, :-1].copy_(row.detach(), non_blocking=True)
        if torch.is_tensor(lr):
            self.buf[self.n, -1:].copy_(lr.detach().reshape(1).to(torch.float32), non_blocking=True)
            self.host_lr.append(None)
        else:
            self.host_lr.append(float(lr))
        self.n += 1

    def full(self):
        return self.n == self.rows

    def flush(self, meters):
        """The ring's rows -> the meters, oldest first; returns the last learning rate (None if the ring was empty)."""
        if self.n == 0:
            return None
        host = self.buf[:self.n].cpu()                                 # the ONE device-to-host copy of these iterations
        last_lr = self.host_lr[-1] if self.host_lr[-1] is not None else float(host[-1, -1])
        self.n, self.host_lr = 0, []
        names = self.names
        loss_cols = [j for j, k in enumerate(names) if k.find('loss') >= 0]
        rows = []
        for r in host.tolist():
            for k in self.loss_keys:
                v = r[names.index(k)]
                if v != v or v in (float('inf'), float('-inf')):
                    raise FloatingPointError("non-finite loss %s: %s" % (k, dict(zip(names, r))))
            rows.append([sum(r[j] for j in loss_cols)] + r[:-1])       # `loss`: the sum of the entries named *loss* (:134)
        meters.update_block(["loss"] + names, rows)
        return last_lr


def save_checkpoint(output_dir, name, model, optimizer, scheduler, arguments):
    """`Checkpointer.save` (check_point.py:31-49): <output_dir>/<name>.pth in the reference's layout, and `last_checkpoint`."""
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "%s.pth" % name)
    logging.getLogger("dcd_amd.trainer").info("Saving checkpoint to %s", path)
    torch.save(checkpoint_state(model, optimizer, scheduler, **arguments), path)
    with open(os.path.join(output_dir, "last_checkpoint"), "w") as f:
        f.write(path)
    return path


def resume(path, model, optimizer=None, scheduler=None):
    """Load a checkpoint file -- or, given a directory, the file its `last_checkpoint` names -- and return the trainer's
    arguments it carries ('iteration', 'iter_per_epoch', ...), ready for `do_train`."""
    if os.path.isdir(path):
        with open(os.path.join(path, "last_checkpoint"), "r") as f:
            path = f.read().strip()
    data = torch.load(path, map_location=torch.device("cpu"), weights_only=False)
    return load_checkpoint_state(data, model, optimizer, scheduler)


def freeze_bn(model):
    """Every BatchNorm layer to eval inside a model that stays in train mode (trainer.py:62-67)."""
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()


def generate_infer_data(model, files, pipeline, out_dir):
    """`gen_data_infer.json` of the collection pass (DGDE/engine/inference.py:59-84): one image per model call."""
    infer_data = {}
    with restored_modes(model), torch.no_grad():
        model.eval()
        for i in range(len(files)):
            img_id = files.img_id(i)
            images, targets = pipeline([files.frame(i)], [files.sample(i)], img_ids=[img_id])
            feats = model.backbone(images)
            preds = model.heads.predictor(feats, targets)
            rows, _, vis, image_of = model.heads.post_processor.forward_batch(preds, targets, test=model.test, features=feats)
            infer_data[img_id] = gen_data.infer_records_batch(rows, vis, image_of, 1)[0]
    return gen_data.dump_gen_data_infer(infer_data, out_dir)


def _pass_plan(batches):
    """(plan, files) of a batch source of data/batches.py, through a `Prefetcher` as well; None where the source has none.  The
    plan is a twin of the source's: asking it for a batch moves neither of the source's two streams."""
    import copy
    source = getattr(batches, "source", batches)
    plan = getattr(source, "plan", None)
    files = getattr(source, "files", None) or getattr(getattr(source, "split", None), "files", None)
    if plan is not None:
        plan = copy.copy(plan)
        plan._next = None
    return plan, files


def _precision(model, tensor):
    """The bf16 scope `KeypointDetector.forward` and the head open under MODEL.FP16 in training."""
    import contextlib
    if not getattr(model, "fp16", False):
        return contextlib.nullcontext()
    if tensor.is_cuda:
        from dcd_amd import _ext
        return _ext.precision_scope("bf16")
    return torch.autocast(device_type=tensor.device.type, dtype=torch.bfloat16)


def collect_step(model, collector, images, targets, image_numbers):
    """The body of the collection loop: backbone -> predictor -> `collector.add`.  No loss, no host read."""
    from dcd_amd.structures.image_list import to_image_list
    pixels = to_image_list(images).tensors
    with _precision(model, pixels):
        features = model.backbone(pixels)
    with _precision(model.heads, features):
        predictions = model.heads.predictor(features, targets)
    reg_pois = predictions.get("reg_pois")
    if reg_pois is None:
        raise RuntimeError("the predictor did not evaluate the heads at the objects' centres (`reg_pois`)")
    collector.add(reg_pois, targets, image_numbers)


def collect_gmw_records(model, batches, iterations, start=0, capacity=None, cfg=None):
    """GMW's training records of batches start .. start + iterations - 1, collected on the device (gmw/collect.py): the model in
    train mode with its BatchNorm layers frozen and no gradients, as the reference's collection pass runs it
    (DGDE/engine/trainer.py:97-98, :114-116), but backbone -> predictor -> `dcd_gmw_train_records` only -- the loss is not
    called.  Returns the `ResidentRecords`; its `collector` attribute is the `TrainRecordCollector` (`gen_data()` for the file).
    capacity: rows of the tables; by default the number of labelled objects of the images the pass will see, which the host
    knows from `files.sample`.  Raises NotImplementedError before the first batch for a configuration the kernel refuses."""
    from dcd_amd.gmw.collect import TrainRecordCollector
    cfg = cfg if cfg is not None else model.cfg
    if iterations < 1:
        raise ValueError("iterations %d" % iterations)
    device = next(model.parameters()).device
    B, M = int(batches.batch_size), int(cfg.DATASETS.MAX_OBJECTS)
    plan, files = _pass_plan(batches)
    if plan is not None:
        rows = [plan(k)[0] for k in range(start, start + iterations)]
    else:
        rows = [list(range(k * B, (k + 1) * B)) for k in range(start, start + iterations)]
    if capacity is None:
        if plan is not None and files is not None:
            counts = {}
            for i in {i for r in rows for i in r}:
                counts[i] = min(len(files.sample(i)["cls"]), M)
            capacity = max(1, sum(counts[i] for r in rows for i in r))
        else:
            capacity = iterations * B * M
    collector = TrainRecordCollector(cfg, device, capacity, iterations)
    numbers = torch.tensor(rows, dtype=torch.int32).to(device)          # every iteration's image numbers, one copy before the loop
    with restored_modes(model), torch.no_grad():
        model.train()
        freeze_bn(model)
        for it in range(iterations):
            images, targets = batches.get(start + it)
            collect_step(model, collector, images, targets, numbers[it])
    records = collector.finish()
    records.collector = collector
    return records


def do_train(cfg, model, optimizer, scheduler, warmup_scheduler, batches, arguments, output_dir, step=None, log_every=10, val=None,
             val_batch_size=1, val_gmw=None, gmw_records=False, val_render_dir=None, val_render_keypoints=False, val_tta=None):
    """batches: a source of data/batches.py (or a `Prefetcher` around one).  step: `step(images, targets) -> (loss_dict,
    log_loss_dict)`, e.g. a `GraphedTrainStep`; by default `train_step` with SOLVER.GRAD_NORM_CLIP.  val: (files, pipeline) of
    `engine.inference.inference`, run after the final checkpoint; its result comes back as arguments["eval"].
    With TEST.GENERATE_GMW and `val` the validation split is walked TWICE, on purpose: once by `generate_infer_data` for
    `gen_data_infer.json` (backbone, predictor and `forward_batch`, which hands out the key points the records need) and once by
    `inference`, which writes the result files and scores them.  The reference's `do_eval` does both in one loop over its
    data loader; here the two are separate functions with separate outputs, and the collection pass runs once per trained model.
    val_batch_size > 1: the evaluation runs in batches of that many images (`inference(batch_size=...)`), and with
    TEST.GENERATE_GMW the validation split is walked ONCE: the records and the result files come out of the same pass.
    val_gmw: a `gmw.GMW` model; the evaluation is then the batched pass of the whole two-stage system (`inference(gmw=...)`),
    whatever val_batch_size is, and arguments["eval"]["gmw"] holds the refined detections' tables.
    gmw_records (with TEST.GENERATE_GMW only): True collects GMW's training records on the device (`collect_gmw_records`) instead
    of running the loss over the split; arguments["gmw_records"] is then the `ResidentRecords` that `gmw.train.train_gmw` takes,
    and `gen_data_train.json` is not written.  "json" writes the file as well, from one bulk copy.  A configuration the record
    kernel refuses raises NotImplementedError before the first batch.  False (the default): the pass and the file as before.
    val_render_dir: the evaluation also leaves one picture per validation image there (`inference(render_dir=...)`, the batched
    pass whatever val_batch_size is); val_render_keypoints draws the dense key points too.
    val_tta: an `engine.inference.TTASpec`, handed to `inference(tta=...)`: the evaluation merges every image's detections with its
    mirrored view's (the batched pass whatever val_batch_size is); None leaves DATASETS.USE_TTA to decide."""
    logger = logging.getLogger("dcd_amd.trainer")
    is_gen = bool(cfg.TEST.GENERATE_GMW)
    if cfg.SOLVER.LR_WARMUP and warmup_scheduler is None:
        raise ValueError("SOLVER.LR_WARMUP needs a warmup_scheduler")
    if log_every < 1:
        raise ValueError("log_every %d" % log_every)
    start_iter = int(arguments["iteration"])
    max_iter = cfg.SOLVER.MAX_ITERATION
    arguments.setdefault("iter_per_epoch", max(1, len(batches) // cfg.SOLVER.IMS_PER_BATCH))
    rank0 = comm.get_rank() == 0
    model.train()
    if is_gen:
        freeze_bn(model)
        logger.info("Start collecting the data for GMW")
        max_iter = start_iter + len(batches) // cfg.SOLVER.IMS_PER_BATCH
    elif step is None:
        def step(images, targets):
            return train_step(model, optimizer, images, targets, cfg.SOLVER.GRAD_NORM_CLIP)
    if gmw_records and not is_gen:
        raise ValueError("gmw_records needs TEST.GENERATE_GMW: it replaces the collection pass, not the training")
    if gmw_records not in (False, True, "json"):
        raise ValueError("gmw_records is False, True or 'json', not %r" % (gmw_records,))
    logger.info("Start training")
    meters, ring = MetricLogger(delimiter=" "), _LogRing(log_every)
    start_time = end = time.time()
    loop = range(start_iter, max_iter)
    if gmw_records:
        # the collection on the device: backbone -> predictor -> record kernels, no loss, no read-back per iteration
        records = collect_gmw_records(model, batches, max_iter - start_iter, start=start_iter, cfg=cfg)
        freeze_bn(model)
        arguments["gmw_records"], arguments["iteration"] = records, max_iter
        logger.info("collected %d records for GMW in %.1f s", len(records), time.time() - start_time)
        loop = range(0)
    for iteration in loop:
        images, targets = batches.get(iteration)
        data_time = time.time() - end
        if is_gen:
            with torch.no_grad():
                log_loss_dict = model(images, targets)[1]
        else:
            log_loss_dict = step(images, targets)[1]                   # the loss dict, and with it the autograd graph, is let go here
        ring.append(log_loss_dict, optimizer.param_groups[0]["lr"])     # the rate this step used, before the schedule moves it
        if not is_gen:
            step_schedulers(scheduler, warmup_scheduler, iteration, cfg)
        now = time.time()
        meters.update(time=now - end, data=data_time)
        end = now
        iteration += 1
        arguments["iteration"] = iteration
        if ring.full() or iteration == max_iter:
            lr = ring.flush(meters)
            eta = datetime.timedelta(seconds=int(meters["time"].global_avg * (max_iter - iteration)))
            logger.info(meters.delimiter.join(["eta: %s" % eta, "iter: %d" % iteration, str(meters), "lr: %.8f" % lr]))
        if not is_gen and rank0:
            if iteration % cfg.SOLVER.SAVE_CHECKPOINT_INTERVAL == 0:
                logger.info("iteration = %d, saving checkpoint ...", iteration)
                save_checkpoint(output_dir, "model_checkpoint_%d" % (iteration // arguments["iter_per_epoch"]), model, optimizer,
                                scheduler, arguments)
            if iteration == max_iter:
                save_checkpoint(output_dir, "model_final", model, optimizer, scheduler, arguments)
    if is_gen:
        out_dir = os.path.join(output_dir, "gen_data")
        if not gmw_records:
            logger.info("Start generate Train data for GMW")
            gen_data.dump_gen_data_train(model.heads.loss_evaluator, out_dir)
        elif gmw_records == "json":
            logger.info("Start generate Train data for GMW")
            gen_data.dump_gen_data(arguments["gmw_records"].collector.gen_data(), out_dir)
        if val is not None and val_batch_size <= 1 and val_gmw is None:
            logger.info("Start generate Infer data for GMW")
            generate_infer_data(model, val[0], val[1], out_dir)
    else:
        total = time.time() - start_time
        logger.info("Total training time: %s (%.4f s / it)", datetime.timedelta(seconds=int(total)),
                    total / max(1, max_iter - start_iter))
    if val is not None:
        from dcd_amd.engine.inference import inference
        render = {"render_dir": val_render_dir, "render_keypoints": val_render_keypoints} if val_render_dir is not None else {}
        if val_tta is not None:
            render["tta"] = val_tta
        if val_batch_size > 1 or val_gmw is not None:
            gen_out_dir = os.path.join(output_dir, "gen_data") if is_gen else None
            if is_gen:
                logger.info("Start generate Infer data for GMW (same pass as the evaluation)")
            arguments["eval"] = inference(model, val[0], val[1], os.path.join(output_dir, "inference"), batch_size=val_batch_size,
                                          gen_out_dir=gen_out_dir, gmw=val_gmw, **render)
        else:
            arguments["eval"] = inference(model, val[0], val[1], os.path.join(output_dir, "inference"), **render)
    return arguments


def main(argv=None):
    """`python -m dcd_amd.engine.train --root KITTI_DIR --output-dir OUT [KEY VALUE ...]`: one process, one GPU (rank and world
    size are taken from the process group when one is initialised)."""
    import argparse
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import Prefetcher, ResidentBatches, StreamingBatches
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    from dcd_amd.model.detector import KeypointDetector
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--root", required=True, help="KITTI directory: ImageSets, image_2, label_2, calib, kpts_ann (and image_3 for "
                    "`DATASETS.USE_RIGHT_IMAGE True`, which trains on both cameras' views)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--batch", type=int, default=None, help="images per step on this GPU (default SOLVER.IMS_PER_BATCH / world size)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--streaming", action="store_true", help="decode every batch in a thread pool instead of keeping the split in HBM")
    ap.add_argument("--no-prefetch", action="store_true")
    ap.add_argument("--eval-split", default=None, help="evaluate this split after the final checkpoint")
    ap.add_argument("--eval-batch", type=int, default=1, help="images per model call of that evaluation (1: one image per call)")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("opts", nargs="*", help="configuration overrides: KEY VALUE ...")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(message)s")
    cfg = get_cfg(opts=parse_overrides(args.opts))
    device = torch.device("cuda", torch.cuda.current_device())
    rank, world = comm.get_rank(), comm.get_world_size()
    batch = args.batch if args.batch is not None else max(1, cfg.SOLVER.IMS_PER_BATCH // world)
    files = KittiFiles(args.root, cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    torch.manual_seed(args.seed)
    model = KeypointDetector(cfg).to(device)
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    arguments = {"iteration": 0}
    if os.path.exists(os.path.join(args.output_dir, "last_checkpoint")):
        arguments = resume(args.output_dir, model, optimizer, scheduler)
    if args.streaming:
        source = StreamingBatches(files, DeviceInputPipeline(cfg, device, is_train=True), batch, args.seed, rank, world)
    else:
        source = ResidentBatches(ResidentSplit(files, cfg, device), batch, args.seed, rank, world)
    val = None
    if args.eval_split:
        val = (KittiFiles(args.root, args.eval_split, cfg, is_train=False), DeviceInputPipeline(cfg, device, is_train=False))
    batches = source if args.no_prefetch else Prefetcher(source, device)
    arguments = do_train(cfg, model, optimizer, scheduler, warmup, batches, arguments, args.output_dir, log_every=args.log_every, val=val,
                         val_batch_size=args.eval_batch)
    if hasattr(source, "close"):
        source.close()
    return arguments


if __name__ == "__main__":
    main()
