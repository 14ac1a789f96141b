"""tests/golden/dcn_workspace_bytes.json: dcd_dcn_v2_workspace_bytes of a given build of the library (pure host code) for the
geometries of tests/test_gpu_dcn.py under the per-call environment switches the size depends on.  Recorded from the commit before
the workspace map (csrc/dcn_workspace.h) existed; the map must advertise the same sizes.

    python tests/golden/make_golden_dcn_workspace.py path/to/libdcd_hip.so
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ENVS = [{}, {"DCD_DCN_DENSE": "0"}, {"DCD_DCN_DENSE": "1"}, {"DCD_BWD_SWEEP": "0"}, {"DCD_BWD_SWEEP": "2"}]
K3 = (3, 3, 1, 1, 1, 1, 1, 1)


def env_key(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def geometries():
    """(B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg), the argument order of the C entry point."""
    from test_gpu_dcn import CASES, DENSE_CASES, DGDE_GEOMETRIES, WIDE_SWEEP_CASES
    out = []
    for B in (1, 8):
        out += [(B, C, H, W, Co) + K3 + (dg,) for _, C, Co, H, W, dg, _ in CASES]
        out += [(B, C, H, W, Co) + K3 + (1,) for _, C, Co, H, W, _ in WIDE_SWEEP_CASES]
        out += [(B, C, H, W, Co) + geo + (dg,) for _, C, Co, H, W, dg, _, geo in DENSE_CASES]
        out += [(B, C, H, W, Co) + K3 + (1,) for C, Co, H, W in DGDE_GEOMETRIES]
    # the cases at their own batch (the poisoned-buffer tests run them so)
    out += [(B, C, H, W, Co) + K3 + (dg,) for B, C, Co, H, W, dg, _ in CASES]
    out += [(B, C, H, W, Co) + K3 + (1,) for B, C, Co, H, W, _ in WIDE_SWEEP_CASES]
    out += [(B, C, H, W, Co) + geo + (dg,) for B, C, Co, H, W, dg, _, geo in DENSE_CASES]
    # test_general_geometry
    out += [(2, 8, 11, 13, 6) + geo + (1,) for geo in ((3, 3, 2, 2, 1, 1, 1, 1), (3, 3, 1, 1, 2, 2, 2, 2), (1, 1, 1, 1, 0, 0, 1, 1),
                                                        (3, 1, 1, 2, 1, 0, 1, 1))]
    out.append((8, 64, 96, 320, 64, 3, 3, 0, 1, 1, 1, 1, 1, 1))      # stride 0: invalid, 0 bytes
    return sorted(set(out))


def sizes(query, geoms):
    """{env key: [bytes per geometry]} from `query(*geometry)`; the environment is restored."""
    saved = {k: os.environ.get(k) for e in ENVS for k in e}
    out = {}
    try:
        for env in ENVS:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(env)
            out[env_key(env)] = [int(query(*q)) for q in geoms]
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


if __name__ == "__main__":
    L = ctypes.CDLL(sys.argv[1])
    L.dcd_dcn_v2_workspace_bytes.restype = ctypes.c_size_t
    L.dcd_dcn_v2_workspace_bytes.argtypes = [ctypes.c_int] * 14
    geoms = geometries()
    nbytes = sizes(L.dcd_dcn_v2_workspace_bytes, geoms)
    with open(os.path.join(HERE, "dcn_workspace_bytes.json"), "w") as f:          # one geometry / one environment per line
        f.write('{"geometries": [\n' + ",\n".join(json.dumps(list(q)) for q in geoms) + '\n],\n"bytes": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in nbytes.items()) + "\n}}\n")
    print("%d geometries x %d environments" % (len(geoms), len(ENVS)))
