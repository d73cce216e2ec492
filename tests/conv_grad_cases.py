"""Shapes, operands and float64 references for the sparse-conv and pool gradients (csrc/backward.hip: k_conv_wgrad_mfma,
k_conv_wgrad_valu, k_wgrad_reduce, k_rulebook_transpose, k_sparse_avgpool_bwd; the dX route re-enters csrc/sparse_conv.hip with
the transposed rulebook and W^T).  tests/test_gpu_conv_backward.py checks the references on the CPU and runs the kernels on
exactly the same bits.  CPU only, no test functions.  Every builder is seeded and cached; a reference is computed once and
shared -- never modify a returned array in place.

Two operand sets.  EXACT: X, W and G from {-2, -1, 1, 2}.  Every product is an integer of magnitude <= 4 and every partial sum,
in any order and association, an integer below 2^24 (dW: <= 4 pairs-of-one-offset <= 4 * 163840; dX: <= 27 * 256 * 4), so every
fp32 FMA / MFMA chain is exact and a correct kernel equals the reference bit for bit; no zero is drawn, so a dropped, doubled or
misplaced row changes every element it touches.  GAUSSIAN: as in tests/test_backward.py, for the rounding behaviour, measured
against the error of the fp32 numpy oracle (oracle/backward.py) on the same inputs.

The references take the oracle's pair lists (oracle.get_indice_pairs) and treat every offset alike: no subm shortcut, the
centre offset is an ordinary pair list."""
import zlib

import numpy as np

from test_gpu_ops import rand_voxels

EXACT_LIMIT = 2 ** 24

# name -> (crops, grid side, voxels per crop, stride); kernel 3, padding 1 throughout
SHAPES = {
    "mid": (2, 32, 13000, 1),          # 26000 input rows: past kConvFewRowsHint = 24576; 13 (subm) or 32 (not subm) wgrad splits
    "cap": (5, 32, 9000, 1),           # n_out 163673 > 64 * 2048: the 64-split cap, rows_per_split 2560
    "edge2049": (1, 16, 2049, 1),      # the first split boundary: 2 splits of 1032 rows, the second holds 1017
    "edge2055": (1, 16, 2055, 1),      # ... and 1023: a ragged tail of 7 rows in the last step of 8
    "few5000": (1, 32, 5000, 1),       # few-row dX above kConvFewRows = 4096
    "stride2": (2, 32, 13000, 2),      # n_in 26000 > n_out 8191: transposed rulebook with cap_in != cap_out
}
BACKBONE = ((7, 16, False), (16, 32, True), (32, 32, False), (32, 64, True), (64, 64, False), (64, 128, True), (128, 128, False),
            (128, 256, True))
# (shape, cin, cout, subm)
CASES_MID = tuple(("mid",) + l for l in BACKBONE)
CASES_CAP = (("cap", 32, 32, False), ("cap", 7, 16, False))
CASES_EDGE = tuple((s, ci, co, True) for s in ("edge2049", "edge2055") for ci, co in ((16, 32), (32, 64), (64, 64)))
CASES_FEW = (("few5000", 64, 128, True), ("few5000", 128, 256, True))
CASES_STRIDE = (("stride2", 32, 32, False),)
CASES = CASES_MID + CASES_CAP + CASES_EDGE + CASES_FEW + CASES_STRIDE
CASES_GAUSSIAN = CASES_MID + CASES_CAP
# one mid-size case per kernel family of the dX route: LDS-DMA (64 -> 32), LDS-DMA 128x128 tiles, the general MFMA kernel (256 -> 128)
CASES_FAMILY = (("mid", 32, 64, True), ("mid", 128, 128, False), ("mid", 128, 256, True))

POOL_SHAPE = "stride2"                 # the pool gradient: kernel 3, stride 2 over the same voxels
POOL_CHANNELS = (32, 64, 256)


def case_id(case):
    return "%s-%d-%d-%s" % (case[0], case[1], case[2], "subm" if case[3] else "conv")


def wgrad_splits(n_out):
    """dcl_sparse_conv_wgrad_splits and the rows_per_split of dcl_sparse_conv_wgrad, restated"""
    splits = min(64, max(1, (max(n_out, 1) + 2047) // 2048))
    per = (max(n_out, 1) + splits - 1) // splits
    return splits, (per + 7) // 8 * 8


def _rng(*key):
    """a generator seeded by the case's name and sizes (the same bits in every process)"""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


_GEOMETRY = {}


def geometry(oracle, shape, subm, padding=1):
    """-> dict(idx (n_in, 4) i32, b, S, stride, padding, pairs (27, 2, n_in), num (27), n_in, n_out) from the oracle's rulebook"""
    key = (shape, bool(subm), padding)
    if key not in _GEOMETRY:
        b, S, per, stride = SHAPES[shape]
        assert not (subm and stride != 1)
        idx = rand_voxels(_rng("voxels", shape, 1), b, S, per)   # (a seed whose dilated sets have odd row counts: 65531, 163673)
        out_idx, pairs, num, _ = oracle.get_indice_pairs(idx, b, [S] * 3, 3, stride, padding, 1, subm=subm)
        _GEOMETRY[key] = dict(idx=idx, b=b, S=S, stride=stride, padding=padding, pairs=pairs, num=num, n_in=idx.shape[0],
                              n_out=idx.shape[0] if subm else out_idx.shape[0])
    return _GEOMETRY[key]


_VALUES = np.array([-2.0, -1.0, 1.0, 2.0], np.float32)


def exact_array(rng, shape):
    return _VALUES[rng.integers(0, 4, size=shape)]


def exact_operands(key, n_in, n_out, cin, cout):
    """(X (n_in, cin), W (27, cin, cout), G (n_out, cout)) float32, every element one of -2, -1, 1, 2"""
    rng = _rng("exact", key, n_in, n_out, cin, cout)
    return exact_array(rng, (n_in, cin)), exact_array(rng, (27, cin, cout)), exact_array(rng, (n_out, cout))


def gaussian_operands(key, n_in, n_out, cin, cout):
    """(X, W, G) float32 normal, W / sqrt(9 cin): the operands of tests/test_backward.py"""
    rng = _rng("gaussian", key, n_in, n_out, cin, cout)
    return (rng.normal(size=(n_in, cin)).astype(np.float32),
            (rng.normal(size=(27, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32),
            rng.normal(size=(n_out, cout)).astype(np.float32))


def conv_backward_ref(X, W, G, pairs, num):
    """float64 (dX (n_in, cin), dW (kvol, cin, cout)): per offset dW[k] = X[rows_in]^T G[rows_out] and dX[rows_in] += G[rows_out]
    W[k]^T.  rows_in are unique inside an offset (every (k, in) pair has at most one out).  On integer operands below 2^53 / terms
    every float64 sum is exact: the result IS the integer gradient."""
    cin, cout = W.shape[-2], W.shape[-1]
    X64, G64 = np.asarray(X, np.float64), np.asarray(G, np.float64)
    W64 = np.asarray(W, np.float64).reshape(-1, cin, cout)
    dX, dW = np.zeros((X64.shape[0], cin)), np.zeros(W64.shape)
    for k in range(W64.shape[0]):
        n = int(num[k])
        if n <= 0:
            continue
        rows_in, rows_out = pairs[k, 0, :n], pairs[k, 1, :n]
        g = G64[rows_out]
        dW[k] = X64[rows_in].T @ g
        dX[rows_in] += g @ W64[k].T
    return dX, dW


def avgpool_backward_ref(n_in, G, pairs, num, rf):
    """float64 (din (n_in, c), magnitude (n_in, c)): din[in] += G[out] / rf[out]; magnitude = the same sum over |G|"""
    G64, rf64 = np.asarray(G, np.float64), np.asarray(rf, np.float64)
    din, mag = np.zeros((n_in, G64.shape[1])), np.zeros((n_in, G64.shape[1]))
    for k in range(pairs.shape[0]):
        n = int(num[k])
        if n <= 0:
            continue
        rows_in, rows_out = pairs[k, 0, :n], pairs[k, 1, :n]
        t = G64[rows_out] / rf64[rows_out, None]
        din[rows_in] += t
        mag[rows_in] += np.abs(t)
    return din, mag


def without_pair(pairs, num, k, j):
    """the rulebook with pair j of offset k removed -> (pairs, num, row_in, row_out of the removed pair)"""
    p, n = pairs.copy(), num.copy()
    cnt = int(num[k])
    assert 0 <= j < cnt
    gone = (int(pairs[k, 0, j]), int(pairs[k, 1, j]))
    p[k, :, j:cnt - 1] = pairs[k, :, j + 1:cnt]
    p[k, :, cnt - 1] = -1
    n[k] = cnt - 1
    return p, n, gone[0], gone[1]


_CASES = {}


def conv_case(oracle, case, operands):
    """-> dict(geo, X, W, G, dX, dW): operands 'exact' or 'gaussian' and their float64 reference, computed once per process"""
    key = (case, operands)
    if key not in _CASES:
        shape, cin, cout, subm = case
        geo = geometry(oracle, shape, subm)
        gen = exact_operands if operands == "exact" else gaussian_operands
        X, W, G = gen(case, geo["n_in"], geo["n_out"], cin, cout)
        dX, dW = conv_backward_ref(X, W, G, geo["pairs"], geo["num"])
        _CASES[key] = dict(geo=geo, X=X, W=W, G=G, dX=dX, dW=dW)
    return _CASES[key]


_E32 = {}


def fp32_oracle_error(oracle, case):
    """(e32 of dX, e32 of dW): max |oracle/backward.py in fp32 numpy - float64 reference| on the gaussian operands of `case` --
    the yardstick of the rounding tests: it comes from the reference side, never from the kernel"""
    if case not in _E32:
        from oracle import backward as ob
        c = conv_case(oracle, case, "gaussian")
        dx32, dw32 = ob.indice_conv_backward(c["X"], c["W"].reshape(3, 3, 3, case[1], case[2]), c["G"], c["geo"]["pairs"],
                                             c["geo"]["num"], case[3])
        _E32[case] = (float(np.abs(dx32 - c["dX"]).max()), float(np.abs(dw32.reshape(c["dW"].shape) - c["dW"]).max()))
    return _E32[case]


# ---- operands from outside (tests/test_gpu_step_replay.py: a call recorded inside the network) ---------------------------------
def pairs_of_table(nbr, n_out, n_in):
    """a device-style neighbour table nbr (kvol, cap), nbr[k][o] = input row of output row o at offset k (an entry names a
    neighbour iff it is one of the n_in rows), as the pair lists of `geometry`: (pairs (kvol, 2, cap) i64, num (kvol,))"""
    nbr = np.asarray(nbr)[:, :int(n_out)]
    kvol = nbr.shape[0]
    pairs, num = np.full((kvol, 2, max(nbr.shape[1], 1)), -1, np.int64), np.zeros(kvol, np.int64)
    for k in range(kvol):
        o = np.nonzero((nbr[k] >= 0) & (nbr[k] < int(n_in)))[0]
        num[k] = o.size
        pairs[k, 0, :o.size], pairs[k, 1, :o.size] = nbr[k][o], o
    return pairs, num


def conv_form(X, W, G, pairs, num, n_out, dtype):
    """forward_ref of tests/conv_fwd_cases.py and conv_backward_ref above with every array and sum in `dtype`: float64 is the
    reference, float32 the module form (the reference's per-offset gather - GEMM - scatter) -> (out, dX, dW (kvol, cin, cout))"""
    cin, cout = W.shape[-2], W.shape[-1]
    X, G, W = np.asarray(X, dtype), np.asarray(G, dtype), np.asarray(W, dtype).reshape(-1, cin, cout)
    out, dX, dW = np.zeros((int(n_out), cout), dtype), np.zeros((X.shape[0], cin), dtype), np.zeros(W.shape, dtype)
    for k in range(W.shape[0]):
        n = int(num[k])
        if n <= 0:
            continue
        rows_in, rows_out = pairs[k, 0, :n], pairs[k, 1, :n]
        out[rows_out] += X[rows_in] @ W[k]
        g = G[rows_out]
        dW[k] = X[rows_in].T @ g
        dX[rows_in] += g @ W[k].T
    return out, dX, dW


def avgpool_form(X, G, pairs, num, n_out, dtype):
    """the average pool over the same pair lists in `dtype` (avgpool_backward_ref above is its gradient in float64): rf[o] = the
    number of pairs that name output row o, out[o] = (sum of its input rows) / rf[o], din[i] += G[o] / rf[o] -> (out, din, rf)"""
    X, G = np.asarray(X, dtype), np.asarray(G, dtype)
    rf = np.zeros(int(n_out), np.int64)
    for k in range(pairs.shape[0]):
        np.add.at(rf, pairs[k, 1, :int(num[k])], 1)
    div = np.maximum(rf, 1).astype(dtype)[:, None]
    out, din = np.zeros((int(n_out), X.shape[1]), dtype), np.zeros(X.shape, dtype)
    for k in range(pairs.shape[0]):
        n = int(num[k])
        if n > 0:
            rows_in, rows_out = pairs[k, 0, :n], pairs[k, 1, :n]
            out[rows_out] += X[rows_in]
            din[rows_in] += G[rows_out] / div[rows_out]
    return out / div, din, rf
