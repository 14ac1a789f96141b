"""Which entry point a convolution layer takes (host only: no GPU, no library).

`layers.conv.Conv2d.forward` / `forward_with_skip` and `DCN.forward` choose between our kernels' entry points and the stock op from
the layer's configuration, the input's device / dtype / shape and a handful of process switches.  A wrong choice is still a
correct convolution -- it shows only as lost speed, or as a whole-step capture that silently falls back to eager -- so this
test pins the choice itself: every entry point is replaced by a stub that returns its own name, the input is a stand-in
object (the predicates read `is_cuda`, `dtype`, `shape`, `requires_grad`, `dim()`), the layers live on the meta device.

tests/golden/conv_routes.json holds one line per (layer, input): the routes of all state combinations, one letter each
(`CODE` below; `X`: raises inside a stream capture).  `python tests/test_conv_routes.py --record` rewrites it -- from a
checkout whose routing is known to be right, never to make a failing test pass.  The anchors further down spell out by hand
what a reader should expect to find in it."""
import itertools
import json
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")

CODE = {"conv3x3": "w", "conv3x3_with_skip": "k", "conv3x3_stock_forward": "f", "conv3x3_stride2_native": "n",
        "conv3x3_stride2": "d", "conv_stem": "m", "conv2d_bias": "b", "stock": "s", "raises": "X", "dcn_one_node": "D"}
ENTRY_POINTS = ("conv3x3", "conv3x3_stock_forward", "conv3x3_stride2_native", "conv3x3_stride2", "conv_stem", "conv2d_bias",
                "conv3x3_with_skip")

# name -> (constructor arguments, forward_with_skip is recorded too); "dcn ..." layers are DCN modules: `D` one node, else the
# route of their offset convolution
LAYERS = {
    "stem 3>16 k7": (dict(cin=3, cout=16, k=7, padding=3), False),
    "stem 16>16": (dict(cin=16, cout=16), True),
    "s2 16>32": (dict(cin=16, cout=32, stride=2), False),
    "s2 32>64": (dict(cin=32, cout=64, stride=2), False),
    "s2 64>128": (dict(cin=64, cout=128, stride=2), False),
    "s2 128>256": (dict(cin=128, cout=256, stride=2), False),
    "s2 256>512": (dict(cin=256, cout=512, stride=2), False),
    "s1 32": (dict(cin=32, cout=32), True),
    "s1 64": (dict(cin=64, cout=64), True),
    "s1 128": (dict(cin=128, cout=128), True),
    "s1 256": (dict(cin=256, cout=256), True),
    "s1 512": (dict(cin=512, cout=512), True),
    "bias 64>27": (dict(cin=64, cout=27, bias=True), False),
    "bias 256>27": (dict(cin=256, cout=27, bias=True), False),
    "bias 64>256": (dict(cin=64, cout=256, bias=True), False),
    "k1 64>64": (dict(cin=64, cout=64, k=1, padding=0), True),
    "bias k1 256>3": (dict(cin=256, cout=3, k=1, padding=0, bias=True), False),
    "dilation 2": (dict(cin=64, cout=64, padding=2, dilation=2), True),
    "groups 2": (dict(cin=64, cout=64, groups=2), True),
    "reflect": (dict(cin=64, cout=64, padding_mode="reflect"), True),
    "same": (dict(cin=64, cout=64, padding="same"), True),
    "bias k5 64>64": (dict(cin=64, cout=64, k=5, padding=2, bias=True), False),
    "dcn 64": (dict(cin=64, cout=64, dcn=True), False),
    "dcn 256>128": (dict(cin=256, cout=128, dcn=True), False),
}

BASES = ((8, 384, 1280), (1, 384, 1280), (2, 96, 320), (2, 94, 318))
DIVISORS = (1, 2, 4, 8, 16, 32)
# name -> (B, H, W, is_cuda, dtype, requires_grad)
INPUTS = {"%dx%dx%d" % (b, h // d, w // d): (b, h // d, w // d, True, torch.float32, True)
          for (b, h, w), d in itertools.product(BASES, DIVISORS)}
INPUTS["8x384x1280 host"] = (8, 384, 1280, False, torch.float32, True)
INPUTS["8x384x1280 half"] = (8, 384, 1280, True, torch.float16, True)
INPUTS["8x384x1280 nograd"] = (8, 384, 1280, True, torch.float32, False)
INPUTS["2x96x320 nograd"] = (2, 96, 320, True, torch.float32, False)

PRECISIONS = ("f32", "bf16x3", "bf16")
S2D_MODES = ("auto", "1", "0")
# (precision scope, ops._S2D_MODE, grad mode, capturing): the order of the letters of a line's first (and second) word
STATES = tuple(itertools.product(PRECISIONS, S2D_MODES, (True, False), (False, True)))
# one switch off (or one value changed) at a time, in f32 / auto, on the inputs derived from (8, 384, 1280): third and fourth word
SWITCHES = (("conv", "_ENABLED", False), ("conv", "_SKIP", False), ("conv", "_STEM", False), ("ops", "_WRW_ENABLED", False),
            ("ops", "_S2_NATIVE", False), ("ops", "_OFFSET_CONV_BWD", False), ("ops", "_OFFSET_CONV_FWD", False),
            ("dcn_v2", "_ONE_NODE", False), ("ops", "_CONV_MIN_MAP", 7680))
SWITCH_STATES = tuple(itertools.product(range(len(SWITCHES)), (True, False), (False, True)))
SWITCH_INPUTS = tuple("8x%dx%d" % (384 // d, 1280 // d) for d in DIVISORS)


class _Input:
    """What the route predicates read of a tensor."""
    device = torch.device("cuda")

    def __init__(self, shape, is_cuda, dtype, requires_grad):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = torch.Size(shape), is_cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


class _Out(str):
    """A stub's return value: its name, with what `DCN.forward` reads of its offset convolution's output."""
    shape = torch.Size((1, 27, 1, 1))
    is_cuda = True
    dtype = torch.float32

    def is_contiguous(self):
        return True


def _modules():
    from dcd_amd import ops
    from dcd_amd.model.backbone.DCNv2 import dcn_v2
    from dcd_amd.model.layers import conv
    return {"ops": ops, "conv": conv, "dcn_v2": dcn_v2}


def _build(spec):
    mods = _modules()
    spec = dict(spec)
    cin, cout, k = spec.pop("cin"), spec.pop("cout"), spec.pop("k", 3)
    with torch.device("meta"):
        if spec.pop("dcn", False):
            return mods["dcn_v2"].DCN(cin, cout, k, 1, 1)
        spec.setdefault("padding", 1)
        spec.setdefault("bias", False)
        return mods["conv"].Conv2d(cin, cout, k, **spec)


def compute_routes():
    """{"layer @ input": "<forward> <forward_with_skip> <forward, switches> <forward_with_skip, switches>"}: a word that was not
    recorded is `-`, trailing ones are left out."""
    from dcd_amd import _ext
    mods = _modules()
    ops, conv, dcn_v2 = mods["ops"], mods["conv"], mods["dcn_v2"]
    layers = {name: (_build(spec), skip) for name, (spec, skip) in LAYERS.items()}
    inputs = {name: _Input((b, 0, h, w), cuda, dtype, rg) for name, (b, h, w, cuda, dtype, rg) in INPUTS.items()}
    words = {(ln, xn): [[], [], [], []] for ln in layers for xn in inputs}
    capturing = [False]

    def run(call):
        try:
            out = call()
        except RuntimeError as e:
            assert "inside a stream capture" in str(e), e
            return CODE["raises"]
        return CODE[out[0] if isinstance(out, tuple) else out]

    def sweep(first_word, input_names):
        for ln, (layer, skip) in layers.items():
            cin = layer.in_channels
            for xn in input_names:
                x = inputs[xn]
                x.shape = torch.Size((x.shape[0], cin, x.shape[2], x.shape[3]))
                words[ln, xn][first_word].append(run(lambda: layer.forward(x)))
                if skip:
                    words[ln, xn][first_word + 1].append(run(lambda: layer.forward_with_skip(x)))

    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("DCD_CONV_SPLIT", raising=False)
        for mod, name, value in (("conv", "_ENABLED", True), ("conv", "_SKIP", True), ("conv", "_STEM", True),
                                 ("ops", "_WRW_ENABLED", True), ("ops", "_S2_NATIVE", True), ("ops", "_OFFSET_CONV_BWD", True),
                                 ("ops", "_OFFSET_CONV_FWD", True), ("dcn_v2", "_ONE_NODE", True), ("dcn_v2", "_FUSED_GLUE", True),
                                 ("ops", "_CONV_MIN_MAP", 480), ("ops", "_CONV_SPLIT_MIN_MAP", 7680),
                                 ("ops", "_CONV_BF16_MIN_MAP", 0), ("ops", "_S2_NATIVE_MIN_PIXELS", 3840)):
            mp.setattr(mods[mod], name, value)                   # the defaults, whatever the environment says
        for name in ENTRY_POINTS:
            mp.setattr(ops, name, lambda *a, _name=name: _Out(_name))
        mp.setattr(nn.Conv2d, "forward", lambda self, x: _Out("stock"))
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
        mp.setattr(dcn_v2._DCNWithOffsets, "apply", staticmethod(lambda *a: _Out("dcn_one_node")))
        mp.setattr(dcn_v2._OffsetMask, "apply", staticmethod(lambda out: (out, out)))
        mp.setattr(dcn_v2, "dcn_v2_conv", lambda input, offset, *a: offset)       # three nodes: the offset convolution's route
        grad_before = torch.is_grad_enabled()
        try:
            for prec, s2d, grad, capturing[0] in STATES:
                mp.setattr(ops, "_S2D_MODE", s2d)
                torch.set_grad_enabled(grad)
                with _ext.precision_scope(prec):
                    sweep(0, inputs)
            mp.setattr(ops, "_S2D_MODE", "auto")
            for i, grad, capturing[0] in SWITCH_STATES:
                mod, name, value = SWITCHES[i]
                torch.set_grad_enabled(grad)
                with pytest.MonkeyPatch.context() as one, _ext.precision_scope("f32"):
                    one.setattr(mods[mod], name, value)
                    sweep(2, SWITCH_INPUTS)
        finally:
            torch.set_grad_enabled(grad_before)
    return {"%s @ %s" % key: " ".join("".join(w) or "-" for w in ws).rstrip(" -") for key, ws in words.items()}


@pytest.fixture(scope="module")
def routes():
    return compute_routes()


def _state(prec="f32", s2d="auto", grad=True, capturing=False):
    return STATES.index((prec, s2d, grad, capturing))


def _switch(name, grad=True, capturing=False):
    return SWITCH_STATES.index(([s[1] for s in SWITCHES].index(name), grad, capturing))


def _words(routes, layer, inp):
    words = [w.strip("-") for w in routes["%s @ %s" % (layer, inp)].split(" ")]
    return words + [""] * (4 - len(words))


def _forward(routes, layer, inp):
    return _words(routes, layer, inp)[0]


LEVELS = ("s2 16>32", "s2 32>64", "s2 64>128", "s2 128>256", "s2 256>512")


def _level_inputs(b, h, w):
    """The five level convolutions with the maps they see for a (b, h, w) image: full resolution, then halved per level."""
    return [(layer, "%dx%dx%d" % (b, h // d, w // d)) for layer, d in zip(LEVELS, DIVISORS)]


def test_routes_match_the_recorded_table(routes):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["code"] == CODE
    want = golden["routes"]
    assert sorted(routes) == sorted(want)
    wrong = ["%s: got %s, recorded %s" % (k, routes[k], want[k]) for k in want if routes[k] != want[k]]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(want), "\n".join(wrong[:20]))


def test_level_convs_native_in_f32(routes):
    for layer, inp in _level_inputs(8, 384, 1280):
        assert _forward(routes, layer, inp)[_state("f32")] == CODE["conv3x3_stride2_native"]


def test_level_convs_space_to_depth_in_bf16(routes):
    for layer, inp in _level_inputs(8, 384, 1280):
        assert _forward(routes, layer, inp)[_state("bf16")] == CODE["conv3x3_stride2"]


def test_level_convs_off_alignment(routes):
    for layer, inp in _level_inputs(2, 94, 318) + [(layer, "2x94x318") for layer in LEVELS]:
        for prec in PRECISIONS:
            assert _forward(routes, layer, inp)[_state(prec, "auto")] == CODE["stock"]
            # a process that captures whole steps: every stride-2 layer with at least 16 input channels stays on our kernels
            assert _forward(routes, layer, inp)[_state(prec, "1")] == CODE["conv3x3_stride2"]
            assert _forward(routes, layer, inp)[_state(prec, "1", capturing=True)] == CODE["conv3x3_stride2"]


def test_stride2_on_stock_inside_a_capture_raises(routes):
    for layer, inp in _level_inputs(2, 94, 318):
        got = _forward(routes, layer, inp)
        assert got[_state("f32", "auto", grad=True, capturing=True)] == CODE["raises"]
        assert got[_state("f32", "auto", grad=False, capturing=True)] == CODE["stock"]      # nothing needs a gradient
        assert got[_state("f32", "0", grad=True, capturing=True)] == CODE["raises"]


def test_stock_forward_needs_a_raised_map_limit(routes):
    line = _words(routes, "s1 256", "8x24x80")
    assert line[0][_state("f32")] == CODE["conv3x3"] and line[1][_state("f32")] == CODE["conv3x3_with_skip"]
    assert line[2][_switch("_CONV_MIN_MAP")] == CODE["conv3x3_stock_forward"]
    assert line[3][_switch("_CONV_MIN_MAP")] == CODE["conv3x3_stock_forward"]
    assert line[2][_switch("_CONV_MIN_MAP", grad=False)] == CODE["stock"]
    reachable = {k for k, v in routes.items() if CODE["conv3x3_stock_forward"] in "".join(v.split(" ")[:2])}
    assert not reachable, reachable                             # never with the default limit


def test_host_and_half_inputs_take_stock(routes):
    for layer in LAYERS:
        for inp in ("8x384x1280 host", "8x384x1280 half"):
            got = set("".join(_words(routes, layer, inp)[:2]))
            # (a half-precision device tensor is still a device tensor to `stock_conv_in_capture`)
            assert got <= ({CODE["stock"]} if inp.endswith("host") or not layer.startswith("s2") else {CODE["stock"], CODE["raises"]}), (layer, inp, got)


def test_stride1_stem_bias_and_dcn(routes):
    s = _state("f32")
    assert _forward(routes, "s1 64", "8x96x320")[s] == CODE["conv3x3"]
    assert _words(routes, "s1 64", "8x96x320")[1][s] == CODE["conv3x3_with_skip"]
    assert _words(routes, "s1 64", "8x384x1280 nograd")[1][s] == CODE["conv3x3"]          # no gradient to fold into the kernel
    assert _forward(routes, "s1 32", "8x96x320")[s] == CODE["stock"]                         # below 64 channels
    assert _forward(routes, "stem 16>16", "8x384x1280")[s] == CODE["conv_stem"]
    assert _forward(routes, "stem 3>16 k7", "8x384x1280")[s] == CODE["stock"]                # its input would need a gradient
    assert _forward(routes, "stem 3>16 k7", "8x384x1280 nograd")[s] == CODE["conv_stem"]
    assert _forward(routes, "bias 64>256", "8x96x320")[s] == CODE["conv2d_bias"]
    assert _forward(routes, "bias 64>256", "8x96x320")[_state("f32", grad=False)] == CODE["stock"]
    assert _forward(routes, "bias k5 64>64", "8x96x320")[s] == CODE["conv2d_bias"]           # large map: the bias gradient alone
    assert _forward(routes, "dcn 64", "8x96x320")[s] == CODE["dcn_one_node"]
    assert _forward(routes, "dcn 64", "2x94x318")[s] == CODE["stock"]
    line = _words(routes, "dcn 64", "8x96x320")
    for name in ("_WRW_ENABLED", "_OFFSET_CONV_BWD", "_OFFSET_CONV_FWD", "_ONE_NODE"):
        assert line[2][_switch(name)] == CODE["conv2d_bias"], name
    for layer in ("k1 64>64", "dilation 2", "groups 2", "reflect", "same"):
        assert set(_forward(routes, layer, "8x96x320")) == {CODE["stock"]}, layer


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    table = compute_routes()
    with open(GOLDEN, "w") as f:
        f.write('{"code": %s,\n "routes": {\n%s\n}}\n' % (json.dumps(CODE), ",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v))
                                                                                     for k, v in table.items())))
    print("%d lines, %d routes" % (len(table), sum(len(v.replace(" ", "")) for v in table.values())))
