"""The inputs of the dot-patch tests (test_patches_cpu.py, test_gpu_patches.py) beyond those of geodesics_cases.py, each
named for what it reaches in patches.hip.  The CPU file pins every case to what it is named for from the model alone,
the GPU file compares the kernels with the model.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import depth_cases as dc
import geodesics_cases as gc

F = np.float32
PS_BLOCK = 256                    # kPsBlock of device_types.h: the lanes of a k_patch_sample workgroup (the argmax's stride)
PS_QUEUE = 1024                   # kPsQueue: the dots a frontier queue holds
# a lone atom has exactly n_points dots: one, two, a wave and a workgroup and the queue's capacity, each less and more
LONE_POINTS = (1, 2, 63, 64, 65, PS_BLOCK - 1, PS_BLOCK, PS_BLOCK + 1, 960, PS_QUEUE - 1, PS_QUEUE, PS_QUEUE + 1)
# ... and with a link that joins every dot to every other the first pick lowers n_points - 1 dots in one step: exactly
# the queue's capacity, and one more - the first overflow
FULL_POINTS = (960, PS_QUEUE + 1, PS_QUEUE + 2)
FULL_LINK = 1e4


@functools.lru_cache(maxsize=None)
def ladder():
    """Five atoms with ONE lattice point each (the exact +z pole), radius 1, probe 1, centres at x = 0 .. 4: the dots lie
    at integer x and z = 2 and link 1 joins neighbours only, every edge of weight exactly 1.  By hand at spacing 0:
    centres [0, 4, 2, 1, 3], cover [inf, 4, 2, 1, 1] (the tie of dots 1 and 3 goes to 1); spacing 1 stops after three."""
    xyz = np.zeros((5, 3), F)
    xyz[:, 0] = np.arange(5)
    return dc._case("ladder", [dc._cols(xyz, np.ones(5, F))], probe=1.0, link=F(1.0))


@functools.lru_cache(maxsize=None)
def mixed():
    """tiny (an empty structure between others), ladder's row, cavity and a lone atom as ONE batch at probe 1.4: structures
    of 100 .. 9 000 dots whose sampling ends at different picks."""
    t, c = gc.get("tiny"), gc.get("cavity")
    lad = ladder()
    parts = [t.part(s)[:4] + (None,) for s in range(len(t.so) - 1)]
    parts += [lad.part(0)[:4] + (None,), c.part(0)[:4] + (None,), gc.get("lone").part(0)[:4] + (None,)]
    return dc._case("mixed", parts)


CASES = dict(gc.CASES, ladder=ladder, mixed=mixed)


def get(name):
    return CASES[name]()
