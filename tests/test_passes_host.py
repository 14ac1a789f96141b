"""The host pieces the passes over a split share (`engine.passes`, `gmw.inference.PackBuffers`): the override parser against the
loops it replaced, the mode restorer, the GMW state loader and the refusals of the pack buffers.  No device, no library."""
import ast

import pytest
import torch


def _loop_of_the_mains(tokens):
    """The loop `engine.inference.main`, `engine.depth_report.main` and `engine.train.main` each had, verbatim."""
    opts = []
    for k, v in zip(tokens[0::2], tokens[1::2]):
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        opts += [k, v]
    return opts


def _loop_of_gmw_train(opts):
    """The loop `gmw.train.records_from_detector` had, verbatim: the one with the guard for values that are no strings."""
    parsed = []
    for k, v in zip(list(opts)[0::2], list(opts)[1::2]):
        try:
            v = ast.literal_eval(v) if isinstance(v, str) else v
        except (ValueError, SyntaxError):
            pass
        parsed += [k, v]
    return parsed


OVERRIDES = [
    ([], []),
    (["SOLVER.IMS_PER_BATCH", "8"], ["SOLVER.IMS_PER_BATCH", 8]),
    (["SOLVER.BASE_LR", "3e-4", "TEST.DETECTIONS_THRESHOLD", "0.0"], ["SOLVER.BASE_LR", 3e-4, "TEST.DETECTIONS_THRESHOLD", 0.0]),
    (["MODEL.PRETRAIN", "False", "MODEL.USE_SYNC_BN", "True"], ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", True]),
    (["INPUT.AUG_PARAMS", "((0.5,), (0.3, 0.4))", "SOLVER.STEPS", "(1, 2)"], ["INPUT.AUG_PARAMS", ((0.5,), (0.3, 0.4)), "SOLVER.STEPS", (1, 2)]),
    (["DATASETS.DETECT_CLASSES", "['Car', 'Cyclist']"], ["DATASETS.DETECT_CLASSES", ["Car", "Cyclist"]]),
    (["INPUT.ORIENTATION", "multi-bin", "DATASETS.TRAIN_SPLIT", "trainval"], ["INPUT.ORIENTATION", "multi-bin", "DATASETS.TRAIN_SPLIT", "trainval"]),
    (["DATASETS.TRAIN_SPLIT", "'val'", "OUTPUT_DIR", '"runs/a b"'], ["DATASETS.TRAIN_SPLIT", "val", "OUTPUT_DIR", "runs/a b"]),
    (["MODEL.PRETRAIN", False, "SOLVER.IMS_PER_BATCH", 8, "SOLVER.STEPS", (1, 2), "X", None], ["MODEL.PRETRAIN", False, "SOLVER.IMS_PER_BATCH", 8,
                                                                                             "SOLVER.STEPS", (1, 2), "X", None]),
    (["SOLVER.IMS_PER_BATCH", "8", "MODEL.PRETRAIN"], ["SOLVER.IMS_PER_BATCH", 8]),
    (["MODEL.PRETRAIN"], []),
    (["A", "1 +", "B", "None", "C", "-3", "D", "1e400", "E", ""], ["A", "1 +", "B", None, "C", -3, "D", float("inf"), "E", ""]),
]


@pytest.mark.parametrize("tokens, want", OVERRIDES)
def test_parse_overrides_is_the_loop_it_replaces(tokens, want):
    from dcd_amd.engine.passes import parse_overrides
    got = parse_overrides(tokens)
    assert got == want and [type(v) for v in got] == [type(v) for v in want]
    for old in (_loop_of_the_mains, _loop_of_gmw_train):
        assert got == old(tokens) and [type(v) for v in got] == [type(v) for v in old(tokens)], old.__name__
    assert parse_overrides(tuple(tokens)) == want                      # `records_from_detector` takes a tuple by default
    assert parse_overrides(iter(tokens)) == want


def _children_modes(m):
    return [c.training for c in m.modules()]


def test_restored_modes_puts_every_flag_back_and_sets_none():
    from dcd_amd.engine.passes import restored_modes
    a, b = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.BatchNorm1d(2)).train(), torch.nn.Linear(2, 2).eval()
    with restored_modes(a, None, b):
        assert a.training is True and b.training is False              # the body chooses the modes, not the context manager
        assert _children_modes(a) == [True, True, True]
        a.eval()
        b.train()
        assert a.training is False and b.training is True
    assert a.training is True and b.training is False
    assert _children_modes(a) == [True, True, True]                    # as `model.train(was_training)` put them back

    class Stop(Exception):
        pass
    with pytest.raises(Stop):
        with restored_modes(a, b, None):
            a.eval()
            b.train()
            raise Stop()
    assert a.training is True and b.training is False
    with restored_modes(a, b):                                         # a body that changes nothing changes nothing
        pass
    assert a.training is True and b.training is False
    with restored_modes():
        pass
    with restored_modes(None):
        pass


def test_restored_modes_refuses_what_has_no_flag_before_the_body_runs():
    """An argument without a `training` flag is an error at entry, before the body runs."""
    from dcd_amd.engine.passes import restored_modes
    ran = []
    with pytest.raises(AttributeError):
        with restored_modes(torch.nn.Linear(1, 1), object()):
            ran.append(1)
    assert ran == []


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)


def test_load_gmw_state_strips_the_wrapper_prefix():
    from dcd_amd.engine.passes import load_gmw_state
    torch.manual_seed(0)
    src = _Toy()
    state = src.state_dict()
    assert sorted(state) == ["fc.bias", "fc.weight"]
    for prefixed in ({"module." + k: v for k, v in state.items()}, dict(state),
                     {"module.fc.weight": state["fc.weight"], "fc.bias": state["fc.bias"]}):
        dst = _Toy()
        assert not torch.equal(dst.fc.weight, src.fc.weight)
        load_gmw_state(dst, prefixed)
        assert torch.equal(dst.fc.weight, src.fc.weight) and torch.equal(dst.fc.bias, src.fc.bias)
    with pytest.raises(RuntimeError):                                  # strict, as `load_state_dict` is: a missing name is an error
        load_gmw_state(_Toy(), {"module.fc.weight": state["fc.weight"]})


class _StubGmw:
    """What `PackBuffers` reads of a GMW model."""

    def __init__(self, num_kpts=73, dtype=torch.float32):
        self.num_kpts = num_kpts
        self._p = torch.zeros(1, dtype=dtype)
        i, j = torch.triu_indices(73, 73, offset=1)
        self.pair_i, self.pair_j = i, j

    def parameters(self):
        return iter([self._p])


def test_pack_buffers_refuse_before_anything_is_allocated():
    """Each refusal is a ValueError that starts with the caller's name.  The device is one this machine may not have: a refusal
    that came after an allocation would be another error."""
    from dcd_amd.gmw.inference import NUM_KPTS, PackBuffers
    assert NUM_KPTS == 73
    nowhere = torch.device("cuda", 0)
    for who in ("RecordRefiner", "depth_report(gmw=...)"):
        with pytest.raises(ValueError, match="72 key points") as e:
            PackBuffers(_StubGmw(), nowhere, 4, 72, who)
        assert str(e.value).startswith(who)
        with pytest.raises(ValueError, match="model: 72") as e:
            PackBuffers(_StubGmw(num_kpts=72), nowhere, 4, 73, who)
        assert str(e.value).startswith(who)
        for cap in (0, -1):
            with pytest.raises(ValueError) as e:
                PackBuffers(_StubGmw(), nowhere, cap, 73, who)
            assert str(e.value).startswith(who) and str(cap) in str(e.value)
        with pytest.raises(ValueError, match="float32") as e:
            PackBuffers(_StubGmw(dtype=torch.float64), nowhere, 4, 73, who)
        assert str(e.value).startswith(who) and "float64" in str(e.value)


def test_pack_buffers_layout():
    from dcd_amd.gmw.inference import PackBuffers
    stub = _StubGmw()
    packs = PackBuffers(stub, torch.device("cpu"), 3, 73, "test")
    P = 73 * 72 // 2
    assert packs.cap == 3 and packs.model is stub
    assert [tuple(b.shape) for b in packs.buffers] == [(3, 4, P), (3, 6, P), (3, 73, 2), (3, 73, 3), (3, 1), (3, 3), (3, 3)]
    assert all(b.dtype == torch.float32 and b.is_contiguous() and not b.any() for b in packs.buffers)
    assert packs.pair_i.dtype == packs.pair_j.dtype == torch.int32 and packs.pair_i.numel() == P
    assert torch.equal(packs.pair_i.long(), stub.pair_i) and torch.equal(packs.pair_j.long(), stub.pair_j)
