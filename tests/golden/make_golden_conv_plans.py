"""tests/golden/conv_plans.json: every size the dcd_conv* entry points of a given build of the library advertise (pure host code;
without a device the CU count falls back to 256, the MI355X's) for the geometries of tests/test_gpu_conv.py, under the default
environment.  Recorded from the commit before csrc/conv_plan.h existed; the header must advertise the same sizes.

    python tests/golden/make_golden_conv_plans.py path/to/libdcd_hip.so
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

I5 = [ctypes.c_int] * 5
# name -> (entry point, argument types, arguments from a geometry (B, Cin, H, W, Cout)); the first HOST_SIZES are also computed by
# tests/host/conv_plan_host.cpp in this order
SIZES = [
    ("conv3x3_workspace", "dcd_conv3x3_workspace_bytes", I5, lambda B, C, H, W, K: (B, C, H, W, K)),
    ("conv3x3_weights_fwd", "dcd_conv3x3_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 0)),
    ("conv3x3_weights_bwd", "dcd_conv3x3_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 1)),
    ("split_weights_fwd", "dcd_conv3x3_split_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 0)),
    ("split_weights_bwd", "dcd_conv3x3_split_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 1)),
    ("split_workspace", "dcd_conv3x3_split_workspace_bytes", I5, lambda B, C, H, W, K: (B, C, H, W, K)),
    ("bf16_workspace", "dcd_conv3x3_bf16_workspace_bytes", I5, lambda B, C, H, W, K: (B, C, H, W, K)),
    ("wrw_workspace", "dcd_conv3x3_wrw_workspace_bytes", I5, lambda B, C, H, W, K: (B, C, H, W, K)),
    ("s2_wrw_workspace", "dcd_conv3x3_s2_f32_wrw_workspace_bytes", I5, lambda B, C, H, W, K: (B, C, H, W, K)),
    ("conv1x1_wrw_bf16_workspace", "dcd_conv1x1_wrw_bf16_workspace_bytes", I5[:3] + [ctypes.c_longlong],
     lambda B, C, H, W, K: (B, K, C, H * W)),
    ("conv1x1_wrw_f32_workspace", "dcd_conv1x1_wrw_f32_workspace_bytes", I5[:3] + [ctypes.c_longlong],
     lambda B, C, H, W, K: (B, K, C, H * W)),
    ("bf16_weights_fwd", "dcd_conv3x3_bf16_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 0)),
    ("bf16_weights_bwd", "dcd_conv3x3_bf16_weights_bytes", I5[:3], lambda B, C, H, W, K: (C, K, 1)),
]
SIZE_NAMES = [s[0] for s in SIZES]
HOST_SIZES = 11
BATCH_FREE = {n for n in SIZE_NAMES if "weights" in n}        # sizes that depend on the channel counts only

# the inline parametrize lists of tests/test_gpu_conv.py as (B, Cin, Cout, H, W), the test's name beside each
INLINE = {
    "test_conv3x3_region_shapes": [(2, 64, 64, 14, 44), (1, 72, 80, 24, 80), (1, 64, 64, 26, 36)],
    "test_conv3x3_full_size_against_stock_solver": [(8, 64, 256, 96, 320), (8, 128, 128, 48, 160), (8, 256, 256, 24, 80),
                                                    (8, 512, 512, 12, 40)],
    "test_conv3x3_split_bf16_form": [(2, 64, 27, 24, 64), (1, 128, 27, 12, 40)],
    "test_conv3x3_mixed_bf16_form": [(2, 64, 27, 24, 64), (1, 128, 27, 12, 40), (8, 64, 64, 96, 320)],
    "test_conv3x3_direct_bf16_is_the_exact_product_of_rounded_operands": [
        (2, 64, 64, 16, 32), (2, 72, 80, 10, 36), (1, 512, 72, 12, 40), (1, 256, 64, 9, 32), (3, 27, 64, 14, 44), (1, 64, 27, 24, 64),
        (1, 16, 16, 96, 128), (2, 128, 256, 24, 80)],
    # 1x1 lists: Cin = the sum of the concatenated inputs' channels
    "test_conv1x1_of_cat_in_the_bf16_scope": [(2, 128, 64, 24, 80), (1, 448, 128, 12, 40), (2, 64, 128, 16, 20), (1, 1280, 512, 12, 40),
                                              (3, 48, 48, 6, 10), (8, 128, 64, 96, 320)],
    "test_conv1x1_of_cat_on_the_fp32_pointwise_kernels": [(2, 128, 64, 24, 80), (1, 448, 128, 12, 40), (2, 64, 128, 16, 20),
                                                          (1, 1280, 512, 12, 40), (3, 48, 48, 6, 10), (2, 32, 64, 96, 320),
                                                          (8, 128, 64, 96, 320), (2, 96, 96, 10, 14), (1, 16, 16, 2, 2)],
    "test_stride2_conv_native_fp32_kernels": [(2, 16, 32, 48, 80), (1, 32, 64, 24, 80), (2, 64, 128, 24, 80), (1, 128, 256, 24, 80),
                                              (1, 256, 512, 12, 40), (3, 16, 48, 8, 16), (8, 16, 32, 384, 1280), (8, 64, 128, 96, 320)],
    "test_stride2_conv_through_space_to_depth": [(2, 16, 32, 48, 80), (1, 32, 64, 24, 80), (2, 64, 128, 24, 80), (1, 128, 256, 24, 80),
                                                 (2, 256, 512, 6, 20), (1, 64, 128, 13, 38)],
}
# not one size is positive / only the sizes that ignore B, H and W are
INVALID = [(2, 0, 16, 32, 64), (2, 64, 16, 32, -3), (0, 0, 0, 0, 0)]
NO_IMAGE = [(0, 64, 16, 32, 64), (2, 64, 16, 0, 64)]


def geometries():
    """(B, Cin, H, W, Cout): every shape at its own batch and at one and eight images."""
    from test_gpu_conv import CASES
    shapes = list(CASES) + [s for lst in INLINE.values() for s in lst]
    out = [(b, C, H, W, K) for B, C, K, H, W in shapes for b in (B, 1, 8)]
    return sorted(set(out)) + INVALID + NO_IMAGE


def sizes(L, geoms):
    """{size name: [bytes per geometry]} from the library L."""
    out = {}
    for name, entry, argtypes, args in SIZES:
        fn = getattr(L, entry)
        fn.restype, fn.argtypes = ctypes.c_size_t, argtypes
        out[name] = [int(fn(*args(*q))) for q in geoms]
    return out


if __name__ == "__main__":
    geoms = geometries()
    nbytes = sizes(ctypes.CDLL(sys.argv[1]), geoms)
    with open(os.path.join(HERE, "conv_plans.json"), "w") as f:                    # one geometry / one size per line
        f.write('{"geometries": [\n' + ",\n".join(json.dumps(list(q)) for q in geoms) + '\n],\n"bytes": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in nbytes.items()) + "\n}}\n")
    print("%d geometries x %d sizes" % (len(geoms), len(SIZES)))
