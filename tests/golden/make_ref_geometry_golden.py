"""Generates tests/golden/ref_geometry.npz: what the REFERENCE's own spconv geometry code (geometry.h, built by
oracle/Makefile into oracle/_ref/libref_geometry.so) returns on the inputs of tests/test_oracle_ref_geometry.py, so that
those tests also run where oracle/_ref could not be built.  Stores, per rulebook case i of CASES, the reference's
output voxels, pairs and pair counts (out_i, pairs_i, num_i), and per getValidOutPos probe the sorted (x, y, z, offset)
rows it returns (vop_<S>_<stride>_<x>).

    python tests/golden/make_ref_geometry_golden.py     # needs oracle/_ref/libref_geometry.so
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import native as K  # noqa: E402
from test_oracle_ref_geometry import CASES, VOP_PROBES, vop_position, voxels  # noqa: E402


def main():
    ref = K.ref_lib()
    assert ref is not None, "oracle/_ref/libref_geometry.so absent: build it first (oracle/Makefile, target ref)"
    z = {}
    for i, (S, ks, st, pad, subm) in enumerate(CASES):
        idx = voxels(S + st, 2, S, 120)
        z["out_%d" % i], z["pairs_%d" % i], z["num_%d" % i], _ = K.get_indice_pairs(idx, 2, [S] * 3, ks, st, pad, 1,
                                                                                     subm=subm, use_ref=True)
    for S, st in VOP_PROBES:
        Sout = (S + 2 - 2 - 1) // st + 1
        osh = (C.c_int * 3)(Sout, Sout, Sout)
        for x in range(S):
            pos = (C.c_int * 3)(*vop_position(S, x))
            out = (C.c_int * (27 * 4))()
            n = ref.ref_valid_out_pos(pos, 3, st, 1, 1, osh, out)
            z["vop_%d_%d_%d" % (S, st, x)] = np.array(sorted(tuple(out[j * 4:j * 4 + 4]) for j in range(n)),
                                                     np.int32).reshape(-1, 4)
    path = os.path.join(ROOT, "tests", "golden", "ref_geometry.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
