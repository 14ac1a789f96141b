"""What every pass over a split shares on the host: the `training` flags put back, and the command lines' preamble (the
`KEY VALUE ...` overrides, the detector and the GMW model from their checkpoints).  The walk over the split itself is
`data.batches.eval_batches`.  Nothing here needs the built library to be imported."""
import ast
import contextlib


@contextlib.contextmanager
def restored_modes(*modules):
    """The `training` flag of every module (a None is skipped) as it was, once the body is left -- by its end or by an exception.
    The body sets the modes it wants itself."""
    before = [(m, m.training) for m in modules if m is not None]
    try:
        yield
    finally:
        for m, training in before:
            m.train(training)


def parse_overrides(tokens):
    """`KEY VALUE ...` tokens -> the `opts` list of `get_cfg`: a string value that is a Python literal becomes that literal, any
    other string stays, a value that is no string passes through, and a key without a value is dropped."""
    tokens = list(tokens)
    opts = []
    for k, v in zip(tokens[0::2], tokens[1::2]):
        try:
            v = ast.literal_eval(v) if isinstance(v, str) else v
        except (ValueError, SyntaxError):
            pass
        opts += [k, v]
    return opts


def load_detector(cfg, ckpt, device):
    """(a `KeypointDetector` of `cfg` on `device` with the weights of `ckpt` -- a file, or a directory with `last_checkpoint` --,
    the trainer's arguments the checkpoint carries)."""
    from dcd_amd.engine.train import resume
    from dcd_amd.model.detector import KeypointDetector
    model = KeypointDetector(cfg).to(device)
    return model, resume(ckpt, model)


def load_gmw_state(model, state_dict):
    """A GMW `state_dict` into `model`, saved from the bare model or from a wrapper that prefixes every name with "module."."""
    return model.load_state_dict({k.replace("module.", ""): v for k, v in state_dict.items()})


def load_gmw(ckpt, device):
    """A `GMW` on `device` with the weights of a checkpoint of `dcd_amd.gmw.train` (checkpoint_epoch_N.pth.tar)."""
    import torch
    from dcd_amd.gmw import GMW
    model = GMW().to(device)
    load_gmw_state(model, torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"])
    return model
