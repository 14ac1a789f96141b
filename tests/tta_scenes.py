"""The seeded pairs of views that test_tta_host.py and test_gpu_tta.py share: built once per process, on the CPU, under the margin
and quarter conditions of `tta_refs.build_scene`, and left unchanged.  TEST INFRASTRUCTURE.

(B, K) -> the candidates of view A of every image: the smallest block, one pair, prefixes of 0 / 1 / 50 in one launch, both sides
of the wave boundary, and the limit with all 128 over the threshold (the 64 KB match table).  The final score differs from the
raw one in two of them, so the visit order is not the rank order."""
import tta_refs as R

SHAPES = {(1, 1): [1], (1, 2): [2], (3, 50): [0, 1, 50], (2, 64): [64, 64], (2, 65): [65, 65], (2, 128): [128, 128]}
SEEDS = {(1, 2): 2}
NK = 73
_SCENES = {}


def scene(bk):
    if bk not in _SCENES:
        _SCENES[bk] = R.build_scene(SEEDS.get(bk, 1), bk[0], bk[1], SHAPES[bk], nk=NK, confidence=bk[1] in (50, 128))
    return _SCENES[bk]
