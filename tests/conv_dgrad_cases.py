"""Shapes, widths, transposed rulebooks and the hand-made table for the direct sparse-conv input gradient (csrc/conv_dgrad.hip:
ops.sparse_conv_dgrad, its host twin ops.sparse_conv_dgrad_host, sparse_conv_backward(dgrad="direct")).  Built on the helpers of
conv_grad_cases.py -- the same seeded voxels, operands and float64 references.  CPU only, no test functions.  Everything is
cached; a reference or a twin result is computed once per process and shared -- never modify a returned array in place."""
import numpy as np

import conv_grad_cases as cg

# name -> (crops, grid side, voxels per crop, stride); kernel 3, padding 1.  The kernel's tiles are 128 (cin <= 32) or 64 rows.
SHAPES = {
    "tail100": (1, 8, 100, 1),         # fewer rows than one tile
    "edge2049": (1, 16, 2049, 1),      # whole tiles plus one row (conv_grad_cases has the same entry)
    "two1500": (2, 16, 1500, 1),       # a crop boundary inside a tile (row 1500 of 3000)
    "stride2s": (1, 16, 3000, 2),      # n_in 3000 > n_out <= 512: cap_in != cap_out
}
for _name, _shape in SHAPES.items():   # conv_grad_cases.geometry looks its shapes up by name
    assert cg.SHAPES.setdefault(_name, _shape) == _shape, _name

# (shape, subm): the stride-1 shapes as submanifold and as dilating convolution
GEOMETRIES = tuple((s, subm) for s in ("tail100", "edge2049", "two1500") for subm in (True, False)) + (("stride2s", False),)
BACKBONE_WIDTHS = tuple((ci, co) for ci, co, _ in cg.BACKBONE[1:])           # the seven layers with a dX
ODD_WIDTHS = ((7, 16), (5, 3), (1, 1), (33, 40))                              # zero-filled lanes, unaligned rows
WIDTHS = BACKBONE_WIDTHS + ODD_WIDTHS
CASES = tuple((s, ci, co, subm) for s, subm in GEOMETRIES for ci, co in WIDTHS)


def inverse_table(geo, cap_in=None, fill=-1):
    """inv (27, cap_in) i32 of a conv_grad_cases geometry: inv[k][i] = o for the oracle's pair (i, o) of offset k, `fill`
    elsewhere -- what dcl_rulebook_transpose makes of the device rulebook"""
    cap_in = geo["n_in"] if cap_in is None else cap_in
    inv = np.full((geo["pairs"].shape[0], max(cap_in, 1)), fill, np.int32)
    for k in range(inv.shape[0]):
        n = int(geo["num"][k])
        inv[k, geo["pairs"][k, 0, :n]] = geo["pairs"][k, 1, :n]
    return inv


_INV = {}


def case_inv(oracle, case):
    key = (case[0], case[3])
    if key not in _INV:
        _INV[key] = inverse_table(cg.geometry(oracle, case[0], case[3]))
    return _INV[key]


_TWIN = {}


def twin(dcl, oracle, case, operands):
    """the host twin's dX of a case (float32), once per process"""
    key = (case, operands)
    if key not in _TWIN:
        c = cg.conv_case(oracle, case, operands)
        _TWIN[key] = dcl.ops.sparse_conv_dgrad_host(c["G"], case_inv(oracle, case), c["geo"]["n_in"], c["W"])
    return _TWIN[key]


# ---- the hand-made table: 8 input rows, 6 dout rows that count and 3 behind them, 5 offsets ------------------------------------
HAND_N_IN, HAND_N_OUT, HAND_ROWS, HAND_KVOL = 8, 6, 9, 5
HAND_INV = np.array([
    #  0   1   2   3   4   5   6   7      input row (row 3: no neighbour at all)
    [  0,  1, -1, -1,  2,  6,  5, -1],   # 6 = n_out: no neighbour
    [ -1, -1, -1, -1, -1, -1, -1, -1],   # an offset nobody has
    [  3,  8,  4, -1, -7,  0,  1,  2],   # 8 >= n_out, -7 < 0
    [  5, -1,  0, -1,  1, 2 ** 30, 7, 3],
    [ -1,  2,  5, -1,  4,  3, -1, -2 ** 31],
], np.int32)
# what each row's chain holds: (offset, dout row) ascending
HAND_NEIGHBOURS = {0: [(0, 0), (2, 3), (3, 5)], 1: [(0, 1), (4, 2)], 2: [(2, 4), (3, 0), (4, 5)], 3: [],
                   4: [(0, 2), (3, 1), (4, 4)], 5: [(2, 0), (4, 3)], 6: [(0, 5), (2, 1)], 7: [(2, 2), (3, 3)]}


def hand_operands(cin, cout, exact):
    """(W (5, cin, cout), G (9, cout) with rows 6 .. 8 NaN)"""
    rng = np.random.default_rng(1000 * cin + cout + (1 if exact else 0))
    if exact:
        W, G = cg.exact_array(rng, (HAND_KVOL, cin, cout)), cg.exact_array(rng, (HAND_ROWS, cout))
    else:
        W = (rng.normal(size=(HAND_KVOL, cin, cout)) / np.sqrt(cout)).astype(np.float32)
        G = rng.normal(size=(HAND_ROWS, cout)).astype(np.float32)
    G[HAND_N_OUT:] = np.nan
    return W, G


def hand_ref(W, G):
    """float64 dX of the hand-made table from HAND_NEIGHBOURS"""
    dX = np.zeros((HAND_N_IN, W.shape[1]))
    for i, nb in HAND_NEIGHBOURS.items():
        for k, o in nb:
            dX[i] += W[k].astype(np.float64) @ G[o].astype(np.float64)
    return dX


def hand_embedded(cap_in, rng):
    """the same table in a wider one: valid-looking junk behind the 8 rows"""
    wide = rng.integers(-3, HAND_ROWS + 3, size=(HAND_KVOL, cap_in)).astype(np.int32)
    wide[:, :HAND_N_IN] = HAND_INV
    return wide
