"""Training GMW from the detector's generated records: the epoch loop of GMW/main.py:231-341, 418-484.

    python -m dcd_amd.gmw.train --train_data_path gen_data/gen_data_train.json --log-dir runs/gmw \\
        [--val_data_path gen_data/gen_data_infer.json --kitti_path /data/kitti]
    python -m dcd_amd.gmw.train --detector-ckpt runs/dgde/model_final.pth --root /data/kitti/training [--split train] --log-dir runs/gmw

The second form replaces the file: the detector's collection pass writes its records into device tables (gmw/collect.py) and GMW
trains on them in the same process.

What the reference does per epoch, kept: AdamW(lr, betas (0.9, 0.999), weight decay) at a CONSTANT rate (a `CosineAnnealingLR` is
built and saved, `scheduler.step()` is never called, main.py:272); from `reg_loss_start_epoch` on the loss weights switch to
(cls 0.1, reg 1.0) unless `no_weight_change` (main.py:313-315); `checkpoint_epoch_N.pth.tar` every 5 epochs and at the last one with
the keys `epoch, state_dict, best_mAP, optimizer, scheduler`; at the last epoch the KITTI evaluation of the refined detections, its
table appended to `log.txt`, the checkpoint copied to `model_best.pth.tar` when the moderate AP improved; `ProgressMeter`'s line on
stdout and in `log.txt` every `print_freq` batches.

What differs is execution.  The records stay in device memory (`gmw.data.ResidentRecords`), the batches of an epoch are
`epoch_order`'s, cut to whole batches (drop_last).  On the GPU nothing inside an iteration reads the device:
  * the transport layer stops its Sinkhorn iteration on a device flag (`device_sinkhorn`, csrc/transport.hip);
  * the reference's `if not torch.isnan(loss).any(): loss.backward()` becomes the optimiser kernel's non-finite guard: the backward
    is seeded with `0 * loss + 1` -- exactly 1 for a finite loss, NaN otherwise -- so a non-finite loss gives non-finite gradients,
    their norm is not finite, and `ClipAdamW.clip_and_step(0)` (no clipping) leaves parameters, moments and step counters as they
    were -- what the reference's `zero_grad(); step()` without a backward does as well.  (Without the seed a NaN in `gt_location`
    gives a NaN loss and FINITE gradients: it enters through |z - gt|, whose derivative sign(NaN) is 0.);
  * `loss, cls_loss, reg_loss, Depth_MAE` go device to device into a ring of `print_freq` rows, and ONE copy per `print_freq`
    iterations feeds the meters in order (the reference: four `.item()` per iteration).
On the CPU the same loop drives `gmw_train_step`, the stock step, so it can be tested without a device.
"""
import argparse
import os
import shutil
import time

import torch

from dcd_amd.engine.passes import load_gmw_state
from dcd_amd.engine.trainer import ClipAdamW, _host_state_value, guard_nonfinite_step
from .data import ResidentRecords, epoch_order, load_train_data
from .step import gmw_losses, gmw_train_step

METER_NAMES = ("Loss", "cls Loss", "reg Loss", "Depth_MAE")


class AverageMeter:
    """main.py:571-589."""

    def __init__(self, name, fmt=":f"):
        self.name, self.fmt = name, fmt
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def __str__(self):
        return ("{name} {val" + self.fmt + "} ({avg" + self.fmt + "})").format(**self.__dict__)


class ProgressMeter:
    """main.py:591-606, its two separators included: tabs on stdout, none in log.txt."""

    def __init__(self, num_batches, meters, prefix="", log_dir=""):
        digits = len(str(num_batches))
        self.batch_fmtstr = "[{:" + str(digits) + "d}/" + ("{:" + str(digits) + "d}").format(num_batches) + "]"
        self.meters, self.prefix = meters, prefix
        self.log_path = os.path.join(log_dir, "log.txt")

    def display(self, batch):
        entries = [self.prefix + self.batch_fmtstr.format(batch)] + [str(m) for m in self.meters]
        print("\t".join(entries))
        with open(self.log_path, "a") as f:
            f.write("".join(entries) + "\n")


def build_gmw_optimizer(model, lr=1e-4, weight_decay=1e-5):
    """AdamW as main.py:255-259, one group in `model.parameters()` order.  On the device: fused + capturable with the learning rate
    as a device tensor, which is what `ClipAdamW`'s own kernels need; on the host the library's default."""
    params = list(model.parameters())
    if params and all(p.is_cuda for p in params):
        group = {"params": params, "lr": torch.tensor(float(lr), dtype=torch.float32, device=params[0].device)}
        return ClipAdamW([group], lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, fused=True, capturable=True)
    return ClipAdamW(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay)


def portable_optimizer_state(optimizer):
    """`optimizer.state_dict()` as the reference's plain AdamW loads it after `torch.load`: host copies of the moments, float step
    counters brought over in ONE stacked copy, plain-float learning rates, none of this optimiser's fused / capturable flags."""
    sd = optimizer.state_dict()
    state = {i: {k: _host_state_value(k, v) for k, v in st.items()} for i, st in sd["state"].items()}
    dev_steps = [(i, st["step"]) for i, st in state.items() if torch.is_tensor(st.get("step")) and st["step"].is_cuda]
    if dev_steps:
        host = torch.stack([t.detach().reshape(()).to(torch.float32) for _, t in dev_steps]).cpu()
        for (i, _), v in zip(dev_steps, host):
            state[i]["step"] = v.clone()
    groups = []
    for g in sd["param_groups"]:
        g = dict(g)
        g["fused"], g["foreach"], g["capturable"] = None, None, False
        for k in ("lr", "initial_lr", "weight_decay", "eps"):
            if torch.is_tensor(g.get(k)):
                g[k] = float(g[k])
        groups.append(g)
    return {"state": state, "param_groups": groups}


def load_optimizer_state(optimizer, saved):
    """Inverse of `portable_optimizer_state` (or a reference checkpoint's entry): the state and the hyper-parameters' VALUES are
    taken, how this optimiser runs (fused, capturable, learning rate as a device tensor) stays."""
    ours = optimizer.state_dict()
    if len(saved["param_groups"]) != len(ours["param_groups"]):
        raise ValueError("the checkpoint's optimiser has %d parameter groups, this one %d"
                         % (len(saved["param_groups"]), len(ours["param_groups"])))
    keep = [{k: v for k, v in g.items() if torch.is_tensor(v) and k != "params"} for g in optimizer.param_groups]
    for og, sg in zip(ours["param_groups"], saved["param_groups"]):
        for k, v in sg.items():
            if k in ("params", "fused", "foreach", "capturable"):
                continue
            og[k] = float(v) if torch.is_tensor(v) else v
    ours["state"] = saved["state"]
    optimizer.load_state_dict(ours)
    for g, old in zip(optimizer.param_groups, keep):            # the same tensor objects, the loaded values
        for k, t in old.items():
            t.fill_(float(g[k]))
            g[k] = t


def _portable_scheduler_state(scheduler):
    def plain(v):
        if torch.is_tensor(v):
            return float(v)
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v
    return {k: plain(v) for k, v in scheduler.state_dict().items()}


def save_checkpoint(state, is_best, log_dir, filename):
    path = os.path.join(log_dir, filename + ".pth.tar")
    torch.save(state, path)
    if is_best:
        shutil.copyfile(path, os.path.join(log_dir, "model_best.pth.tar"))
    return path


def _step_without_clipping(optimizer):
    """The optimiser step with the non-finite guard and no clipping, without a host read."""
    if optimizer.own_kernels_ok():
        return optimizer.clip_and_step(0)
    grads = [p.grad for g in optimizer.param_groups for p in g["params"] if p.grad is not None]
    total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
    guard_nonfinite_step(optimizer, total)
    optimizer.step()
    optimizer.found_inf = None
    return total


def train_iteration(model, optimizer, batch, cls_weight, reg_weight, compute_z=None):
    """One iteration on (kpts_2d, kpts_3d, pred_rot, gt_location) -> the four logged values as one (4,) tensor on the batch's device:
    loss, cls_loss, reg_loss, Depth_MAE (main.py:447-476)."""
    kpts_2d, kpts_3d, pred_rot, gt_location = batch
    if kpts_2d.is_cuda:
        optimizer.zero_grad(set_to_none=True)
        loss, cls_loss, reg_loss, pred_depth = gmw_losses(model, kpts_2d, kpts_3d, pred_rot, gt_location, cls_weight, reg_weight,
                                                          compute_z)
        # the seed is 1 for a finite loss and NaN otherwise (0 * NaN, 0 * inf): a NaN target reaches the loss through |z - gt|, whose
        # derivative sign(NaN) is 0 in torch, so the gradients of a NaN loss would be FINITE and the guard would let them through
        loss.backward(gradient=loss.detach() * 0.0 + 1.0)
        _step_without_clipping(optimizer)
        loss, cls_loss, reg_loss, pred_depth = loss.detach(), cls_loss.detach(), reg_loss.detach(), pred_depth.detach()
    else:
        loss, cls_loss, reg_loss, pred_depth = gmw_train_step(model, optimizer, kpts_2d, kpts_3d, pred_rot, gt_location, cls_weight,
                                                              reg_weight, compute_z)
    gt_depth = gt_location[:, 2]
    depth_mae = ((pred_depth - gt_depth).abs() / gt_depth).mean()
    return torch.stack([loss.reshape(()), cls_loss.reshape(()), reg_loss.reshape(()), depth_mae.reshape(())])


class _Ring:
    """`rows` iterations' logged values where the step left them; `flush` is the one copy to the host."""

    def __init__(self, rows, device):
        self.buf = torch.zeros((rows, len(METER_NAMES)), dtype=torch.float32, device=device)
        self.n, self.host = 0, []

    def append(self, values, batch_size, seconds):
        self.buf[self.n].copy_(values, non_blocking=True)
        self.host.append((batch_size, seconds))
        self.n += 1

    def flush(self):
        rows = self.buf[:self.n].cpu().tolist() if self.n else []
        out = [(r, b, s) for r, (b, s) in zip(rows, self.host)]
        self.n, self.host = 0, []
        return out


def train_gmw(model, records, log_dir, epochs=100, batch_size=16, lr=1e-4, weight_decay=1e-5, cls_weight=1.0, reg_weight=0.0,
              reg_loss_start_epoch=50, no_weight_change=False, print_freq=10, seed=0, resume=None, val_data=None, kitti_root=None,
              compute_z=None, rank=0, world_size=1):
    """Trains `model` (a `GMW` already on its device) on `records` (a path, the parsed JSON, `load_train_data`'s arrays or a
    `ResidentRecords`).  Returns {'epoch', 'best_mAP', 'history': [(epoch, batch, loss, cls_loss, reg_loss, Depth_MAE), ...],
    'optimizer', 'scheduler'}.  A model on the GPU gets its transport layer's `device_sinkhorn` switched on.  `rank` and
    `world_size` reach the sampler only (no DDP wrapping here)."""
    if print_freq < 1 or batch_size < 1:
        raise ValueError("print_freq %d, batch_size %d" % (print_freq, batch_size))
    device = next(model.parameters()).device
    os.makedirs(log_dir, exist_ok=True)
    if not isinstance(records, ResidentRecords):
        if not (isinstance(records, dict) and hasattr(records.get("kpts_2d"), "shape")):
            records = load_train_data(records)
        records = ResidentRecords(records, device)
    if device.type == "cuda":
        model.sinkhorn.device_sinkhorn = True
    optimizer = build_gmw_optimizer(model, lr, weight_decay)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, epochs, eta_min=0, last_epoch=-1)   # saved, never stepped
    start_epoch, best_mAP = 0, 0.0
    if resume:
        checkpoint = torch.load(resume, map_location="cpu", weights_only=False)
        start_epoch, best_mAP = int(checkpoint["epoch"]), checkpoint["best_mAP"]
        load_gmw_state(model, checkpoint["state_dict"])
        load_optimizer_state(optimizer, checkpoint["optimizer"])
        scheduler.load_state_dict(checkpoint["scheduler"])
        print("=> loaded checkpoint '{}' (epoch {})".format(resume, checkpoint["epoch"]))

    n_batches = len(epoch_order(len(records), 0, seed, rank, world_size)) // batch_size
    if n_batches < 1:
        raise ValueError("%d records per rank give no whole batch of %d" % (len(records) // world_size, batch_size))
    history = []
    for epoch in range(start_epoch + 1, epochs + 1):
        if epoch >= reg_loss_start_epoch and not no_weight_change:
            reg_weight, cls_weight = 1.0, 0.1
        model.train()
        order = epoch_order(len(records), epoch, seed, rank, world_size)
        time_meter = AverageMeter("Time", ":6.4f")
        meters = [AverageMeter(name, ":6.4f") for name in METER_NAMES]
        progress = ProgressMeter(n_batches, [time_meter] + meters, prefix="Epoch: [{}]".format(epoch), log_dir=log_dir)
        ring = _Ring(print_freq, device)
        begin = time.time()
        for k in range(n_batches):
            batch = records.batch(order[k * batch_size:(k + 1) * batch_size])
            values = train_iteration(model, optimizer, batch, cls_weight, reg_weight, compute_z)
            ring.append(values, batch_size, time.time() - begin)          # the reference never moves `end`: time since the epoch began
            if k % print_freq == 0 or k == n_batches - 1:
                first = k - ring.n + 1
                for j, (row, b, seconds) in enumerate(ring.flush()):
                    time_meter.update(seconds)
                    for m, v in zip(meters, row):
                        m.update(v, b)
                    history.append((epoch, first + j) + tuple(row))
                if k % print_freq == 0:
                    progress.display(k)

        last = epoch == epochs
        if last and val_data is not None:
            from .inference import evaluate, load_infer_data
            if not (isinstance(val_data, dict) and "img_idx" in val_data):
                val_data = load_infer_data(val_data)
            model.eval()
            text, _, mAP_now = evaluate(model, val_data, kitti_root, out_dir=log_dir, device=device, fused=device.type == "cuda",
                                        compute_z=compute_z)
            print(text)
            is_best, best_mAP = mAP_now > best_mAP, max(mAP_now, best_mAP)
            with open(os.path.join(log_dir, "log.txt"), "a") as f:
                f.write("\n{}\n\n".format(text))
        else:
            is_best = False
        if (epoch > 0 and epoch % 5 == 0) or last:
            save_checkpoint({"epoch": epoch, "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                             "best_mAP": best_mAP, "optimizer": portable_optimizer_state(optimizer),
                             "scheduler": _portable_scheduler_state(scheduler)},
                            is_best, log_dir, "checkpoint_epoch_" + str(epoch))
    return {"epoch": max(start_epoch, epochs), "best_mAP": best_mAP, "history": history, "optimizer": optimizer,
            "scheduler": scheduler}


def build_parser():
    p = argparse.ArgumentParser(description="Train GMW on the records a trained detector generated")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--train_data_path", default=None, type=str, help="gen_data_train.json of a detector's collection pass")
    src.add_argument("--detector-ckpt", dest="detector_ckpt", default=None, type=str,
                     help="a detector checkpoint: its records are collected on the device and GMW trains on them, no file in between")
    p.add_argument("--root", default=None, type=str, help="KITTI directory of the collection pass (with --detector-ckpt)")
    p.add_argument("--split", default="train", type=str, help="the split the detector's records are collected from")
    p.add_argument("--detector-batch", dest="detector_batch", default=8, type=int, help="images per detector call of that pass")
    p.add_argument("--detector-opts", dest="detector_opts", nargs="*", default=[], help="detector configuration overrides: KEY VALUE ...")
    p.add_argument("--val_data_path", default=None, type=str)
    p.add_argument("--kitti_path", default=None, type=str)
    p.add_argument("--log-dir", dest="log_dir", default="", type=str)
    p.add_argument("--epochs", default=100, type=int)
    p.add_argument("-b", "--batch-size", dest="batch_size", default=16, type=int)
    p.add_argument("--lr", "--learning-rate", dest="lr", default=1e-4, type=float)
    p.add_argument("--wd", "--weight-decay", dest="weight_decay", default=1e-5, type=float)
    p.add_argument("-p", "--print-freq", dest="print_freq", default=10, type=int)
    p.add_argument("--resume", default="", type=str)
    p.add_argument("--seed", default=None, type=int)
    p.add_argument("--reg_loss_start_epoch", default=50, type=int)
    p.add_argument("--no_weight_change", action="store_true")
    p.add_argument("--cls_weight", default=1.0, type=float)
    p.add_argument("--reg_weight", default=0.0, type=float)
    return p


def records_from_detector(ckpt, root, split="train", batch=8, opts=(), device="cuda:0"):
    """The collection pass of a trained detector over a KITTI split (`engine.train.collect_gmw_records`): loads the checkpoint, walks
    the split's labelled images in file order without flips, in whole batches, releases the detector and returns the
    `ResidentRecords`."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.passes import load_detector, parse_overrides
    from dcd_amd.engine.train import collect_gmw_records
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "TEST.GENERATE_GMW", True] + parse_overrides(opts))
    device = torch.device(device)
    files = KittiFiles(root, split, cfg, is_train=True)
    model, _ = load_detector(cfg, ckpt, device)
    batch = max(1, min(int(batch), len(files)))
    source = ResidentBatches(ResidentSplit(files, cfg, device), batch, seed=0, is_train=False)
    iterations = len(files) // batch                            # whole batches, as the reference's pass (trainer.py:97-98)
    records = collect_gmw_records(model, source, iterations, cfg=cfg)
    del model, source
    torch.cuda.empty_cache()
    return records


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    if args.val_data_path and not args.kitti_path:
        raise SystemExit("--val_data_path needs --kitti_path (labels and ImageSets/val.txt)")
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if not torch.cuda.is_available():
        raise SystemExit("training GMW needs a GPU: the edge-depth solver (dcd_amd.ops.compute_z) has no CPU path")
    from .model import GMW
    records = args.train_data_path
    if args.detector_ckpt:
        if not args.root:
            raise SystemExit("--detector-ckpt needs --root (the KITTI directory of the collection pass)")
        records = records_from_detector(args.detector_ckpt, args.root, args.split, args.detector_batch, args.detector_opts)
        print("collected %d records from %s" % (len(records), args.detector_ckpt))
    model = GMW(device_sinkhorn=True).to(torch.device("cuda:0"))
    train_gmw(model, records, args.log_dir or ".", epochs=args.epochs, batch_size=args.batch_size, lr=args.lr,
              weight_decay=args.weight_decay, cls_weight=args.cls_weight, reg_weight=args.reg_weight,
              reg_loss_start_epoch=args.reg_loss_start_epoch, no_weight_change=args.no_weight_change, print_freq=args.print_freq,
              seed=args.seed or 0, resume=args.resume or None, val_data=args.val_data_path, kitti_root=args.kitti_path)


if __name__ == "__main__":
    main()
