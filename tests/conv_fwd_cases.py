"""Shapes, widths, rulebooks, float64 references and the hand-made table for the compact sparse-conv forward
(csrc/conv_fwd_compact.hip: ops.sparse_conv(form="compact"), its host twin ops.sparse_conv_compact_host).  Built on the helpers of
conv_grad_cases.py and conv_dgrad_cases.py -- the same seeded voxels and operands (X and W of conv_grad_cases.conv_case) and a
float64 forward reference from the oracle's pair lists.  CPU only, no test functions.  Everything is cached; a reference or a
twin result is computed once per process and shared -- never modify a returned array in place."""
import numpy as np

import conv_dgrad_cases as dc
import conv_grad_cases as cg

SHAPES = dc.SHAPES                      # tail100, edge2049, two1500, stride2s
GEOMETRIES = dc.GEOMETRIES              # the three stride-1 shapes as subm and as dilating convolution, stride2s dilating
WIDTHS = dc.WIDTHS                      # the seven backbone widths with a 3^3 kernel + (7, 16), (5, 3), (1, 1), (33, 40)
CASES = dc.CASES                        # (shape, cin, cout, subm)
DILATING_WIDTHS = ((32, 32), (64, 64), (128, 128))     # the layers that open levels 1 - 3: what CONV_FWD_COMPACT_WIDTHS may hold


def forward_table(geo, cap=None, fill=-1):
    """nbr (27, cap) i32 of a conv_grad_cases geometry: nbr[k][o] = i for the oracle's pair (i, o) of offset k, `fill` elsewhere
    -- what spconv.ops.build_rulebook makes on the device"""
    cap = geo["n_out"] if cap is None else cap
    nbr = np.full((geo["pairs"].shape[0], max(cap, 1)), fill, np.int32)
    for k in range(nbr.shape[0]):
        n = int(geo["num"][k])
        nbr[k, geo["pairs"][k, 1, :n]] = geo["pairs"][k, 0, :n]
    return nbr


_NBR = {}


def case_nbr(oracle, case):
    key = (case[0], case[3])
    if key not in _NBR:
        _NBR[key] = forward_table(cg.geometry(oracle, case[0], case[3]))
    return _NBR[key]


def forward_ref(X, W, pairs, num, n_out):
    """float64 out (n_out, cout): per offset out[rows_out] += X[rows_in] W[k] (rows_out are unique inside an offset).  On the
    exact operands every sum is an integer below 2^53: the result IS the integer result."""
    cin, cout = W.shape[-2], W.shape[-1]
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64).reshape(-1, cin, cout)
    out = np.zeros((n_out, cout))
    for k in range(W64.shape[0]):
        n = int(num[k])
        if n > 0:
            out[pairs[k, 1, :n]] += X64[pairs[k, 0, :n]] @ W64[k]
    return out


_REF, _TWIN, _E32 = {}, {}, {}


def ref(oracle, case, operands):
    """the float64 forward of a case on the operands of conv_grad_cases.conv_case, once per process"""
    key = (case, operands)
    if key not in _REF:
        c = cg.conv_case(oracle, case, operands)
        _REF[key] = forward_ref(c["X"], c["W"], c["geo"]["pairs"], c["geo"]["num"], c["geo"]["n_out"])
    return _REF[key]


def twin(dcl, oracle, case, operands):
    """the host twin's result of a case (float32), once per process"""
    key = (case, operands)
    if key not in _TWIN:
        c = cg.conv_case(oracle, case, operands)
        _TWIN[key] = dcl.ops.sparse_conv_compact_host(c["X"], case_nbr(oracle, case), c["geo"]["n_out"], c["W"], case[3])
    return _TWIN[key]


def fp32_oracle_error(oracle, case):
    """e32 = max |oracle.native.indice_conv in fp32 - float64 reference| on the gaussian operands of `case`: the yardstick of the
    rounding test.  It comes from the reference side, never from the kernel."""
    if case not in _E32:
        c = cg.conv_case(oracle, case, "gaussian")
        geo = c["geo"]
        o32 = oracle.indice_conv(c["X"], c["W"].reshape(3, 3, 3, case[1], case[2]), geo["pairs"], geo["num"], geo["n_out"], case[3])
        _E32[case] = float(np.abs(o32.astype(np.float64) - ref(oracle, case, "gaussian")).max())
    return _E32[case]


# ---- the hand-made table: 70 output rows (one 128-row tile, two 64-row tiles), 40 input rows that count and 8 NaN rows behind
# them, 27 offsets --------------------------------------------------------------------------------------------------------------
HAND_N_OUT, HAND_N_IN, HAND_ROWS, HAND_KVOL = 70, 40, 48, 27
HAND_EMPTY = 17                         # the row without any neighbour
HAND_ALL, HAND_32, HAND_33, HAND_ONE = 0, 3, 5, 9     # offsets present in every row but HAND_EMPTY / in exactly 32 / 33 / 1 rows
HAND_NONE = (1, 2, 20, 21, 22, 23, 24, 25, 26)        # offsets present in no row
HAND_ONE_ROW = 69
_BAD = (HAND_N_IN, HAND_N_IN + 3, HAND_ROWS, 10 ** 6, -2, -7, -2 ** 31)      # entries that name no row: >= n_in or negative


def _hand_table():
    rng = np.random.default_rng(2718)
    rows = np.array([o for o in range(HAND_N_OUT) if o != HAND_EMPTY])
    nbr = np.full((HAND_KVOL, HAND_N_OUT), -1, np.int64)
    present = np.zeros((HAND_KVOL, HAND_N_OUT), bool)
    present[HAND_ALL, rows] = True
    present[HAND_32, np.sort(rng.permutation(rows)[:32])] = True
    present[HAND_33, np.sort(rng.permutation(rows)[:33])] = True
    present[HAND_ONE, HAND_ONE_ROW] = True
    for k in range(HAND_KVOL):
        if k not in (HAND_ALL, HAND_32, HAND_33, HAND_ONE) + HAND_NONE:
            present[k, rows] = rng.random(rows.size) < 0.4
    nbr[present] = rng.integers(0, HAND_N_IN, size=int(present.sum()))
    absent = np.argwhere(~present)
    for j in rng.permutation(absent.shape[0])[:300]:           # a good part of the absent entries: values that name no row
        nbr[tuple(absent[j])] = _BAD[int(rng.integers(0, len(_BAD)))]
    nbr[HAND_NONE[0], HAND_EMPTY] = 2 ** 30
    nbr[HAND_ALL, HAND_EMPTY] = HAND_N_IN
    nbr[HAND_33, HAND_EMPTY] = -7
    return nbr.astype(np.int32), present


HAND_NBR, HAND_PRESENT = _hand_table()


def hand_neighbours(o, subm):
    """(offset, input row) of output row o in the visiting order: k ascending, the centre first for subm"""
    ks = [k for k in range(HAND_KVOL) if HAND_PRESENT[k, o]]
    centre = HAND_KVOL // 2
    if subm and centre in ks:
        ks = [centre] + [k for k in ks if k != centre]
    return [(k, int(HAND_NBR[k, o])) for k in ks]


def hand_operands(cin, cout, exact):
    """(X (48, cin) with rows 40 .. 47 NaN, W (27, cin, cout))"""
    rng = np.random.default_rng(1000 * cin + cout + (1 if exact else 0))
    if exact:
        X, W = cg.exact_array(rng, (HAND_ROWS, cin)), cg.exact_array(rng, (HAND_KVOL, cin, cout))
    else:
        X = rng.normal(size=(HAND_ROWS, cin)).astype(np.float32)
        W = (rng.normal(size=(HAND_KVOL, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    X[HAND_N_IN:] = np.nan
    return X, W


def hand_ref(X, W):
    """float64 result of the hand-made table from HAND_PRESENT"""
    out = np.zeros((HAND_N_OUT, W.shape[2]))
    for o in range(HAND_N_OUT):
        for k, i in hand_neighbours(o, False):
            out[o] += X[i].astype(np.float64) @ W[k].astype(np.float64)
    return out


def hand_embedded(cap, rng):
    """the same table in a wider one: valid-looking junk behind the 70 rows"""
    wide = rng.integers(-3, HAND_ROWS + 3, size=(HAND_KVOL, cap)).astype(np.int32)
    wide[:, :HAND_N_OUT] = HAND_NBR
    return wide
