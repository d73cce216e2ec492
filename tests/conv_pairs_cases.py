"""A synthetic rulebook and numpy restatements for the ordered pair list and the pair-walking weight gradient
(csrc/conv_wgrad_pairs.hip); shared by tests/test_conv_pairs_abi.py (CPU) and tests/test_gpu_conv_wgrad_pairs.py.  CPU only, no
test functions.  Builders are seeded and cached -- never modify a returned array in place.

The synthetic gather table: n_in = 3000, n_out = 4000, cap = 4100.  Offset k holds exactly pair_counts(S)[k] pairs -- every
length around a 16-pair slab and around a split of S pairs, and offsets without any --, on random output rows with distinct input
rows (an input row meets an offset at most once: the precondition the list is sized by).  The entries that are no pair cycle
through -1, -5, n_in and 2^30; rows at or past n_out hold valid-looking indices, which must never be read as pairs."""
import numpy as np

N_IN, N_OUT, CAP = 3000, 4000, 4100
NOT_A_PAIR = (-1, -5, N_IN, 2 ** 30)
HEAD, HEAD_START, HEAD_NSPLIT, HEAD_OVERFLOW, HEAD_FIRST_SPLIT = 96, 32, 60, 61, 64


def pair_counts(S):
    c = [0, 1, 2, 15, 16, 17, S - 1, S, S + 1, 2 * S + 1, 0, 31, 33, 2 * S, 2 * S - 1, min(3 * S, N_IN - 1), N_IN, 0, 7, S + 17,
         64, 100, 2 * S + 16, 1, 48, min(5 * S + 3, N_IN - 7), 0]
    assert len(c) == 27 and max(c) <= N_IN and sum(c) <= 27 * N_IN
    return c


_NBR = {}


def synthetic_nbr(S):
    """-> (nbr (27, CAP) int32, counts)"""
    if S not in _NBR:
        rng = np.random.default_rng(950 + S)
        counts = pair_counts(S)
        nbr = np.empty((27, CAP), np.int32)
        for k, c in enumerate(counts):
            row = np.array([NOT_A_PAIR[(o + k) % 4] for o in range(CAP)], np.int64)
            outs = np.sort(rng.choice(N_OUT, size=c, replace=False))
            row[outs] = rng.permutation(N_IN)[:c]
            row[N_OUT:] = rng.integers(0, N_IN, size=CAP - N_OUT)
            nbr[k] = row.astype(np.int32)
        _NBR[S] = (nbr, counts)
    return _NBR[S]


def pairs_ref(nbr, n_out, n_in, max_pairs, S):
    """the contract of dcl_conv_pairs restated -> dict(head, pair_in, pair_out, split_tab, nsplit); entries nobody writes are -1"""
    kvol = nbr.shape[0]
    head = np.full(HEAD, -1, np.int32)
    pin, pout = np.full(max(max_pairs, 1), -1, np.int32), np.full(max(max_pairs, 1), -1, np.int32)
    tab = np.full((max_pairs // S + kvol, 4), -1, np.int32)
    start, nsplit = 0, 0
    for k in range(kvol):
        v = nbr[k, :n_out].astype(np.int64)
        outs = np.nonzero((v >= 0) & (v < n_in))[0]                   # ascending o
        count = outs.size
        stored = int(min(max(max_pairs - start, 0), count))
        pin[start:start + stored] = v[outs[:stored]]
        pout[start:start + stored] = outs[:stored]
        head[k], head[HEAD_START + k], head[HEAD_FIRST_SPLIT + k] = count, start, nsplit
        for f in range(0, stored, S):
            tab[nsplit] = (k, start + f, min(S, stored - f), 0)
            nsplit += 1
        start += count
    head[HEAD_START + kvol], head[HEAD_FIRST_SPLIT + kvol], head[HEAD_NSPLIT] = start, nsplit, nsplit
    head[HEAD_OVERFLOW] = max(0, start - max_pairs)
    return dict(head=head, pair_in=pin, pair_out=pout, split_tab=tab, nsplit=nsplit)


def same_list(got, want, kvol=27):
    """'' if two pair lists (dicts of numpy arrays) agree in everything the contract defines, else what differs"""
    gh, wh = np.asarray(got["head"]), np.asarray(want["head"])
    for name, lo, n in (("count", 0, kvol), ("start", HEAD_START, kvol + 1), ("nsplit", HEAD_NSPLIT, 1),
                        ("overflow", HEAD_OVERFLOW, 1), ("first split", HEAD_FIRST_SPLIT, kvol + 1)):
        if not np.array_equal(gh[lo:lo + n], wh[lo:lo + n]):
            return "%s: got %s want %s" % (name, gh[lo:lo + n].tolist(), wh[lo:lo + n].tolist())
    stored = int(min(wh[HEAD_START + kvol], np.asarray(want["pair_in"]).shape[0]))
    for name in ("pair_in", "pair_out"):
        g, w = np.asarray(got[name])[:stored], np.asarray(want[name])[:stored]
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            return "%s: %d of %d differ, first at %d (got %d want %d)" % (name, bad.size, stored, bad[0], g[bad[0]], w[bad[0]])
    ns = int(wh[HEAD_NSPLIT])
    g, w = np.asarray(got["split_tab"]).reshape(-1, 4)[:ns], np.asarray(want["split_tab"]).reshape(-1, 4)[:ns]
    if not np.array_equal(g, w):
        bad = np.nonzero((g != w).any(1))[0]
        return "split table: row %d got %s want %s" % (bad[0], g[bad[0]].tolist(), w[bad[0]].tolist())
    return ""


def oracle_style_pairs(nbr, n_out, n_in):
    """(pairs (kvol, 2, n_in), num (kvol)) in the layout of conv_grad_cases.conv_backward_ref, from a gather table"""
    kvol = nbr.shape[0]
    pairs, num = np.full((kvol, 2, max(n_in, 1)), -1, np.int64), np.zeros(kvol, np.int64)
    for k in range(kvol):
        v = nbr[k, :n_out].astype(np.int64)
        outs = np.nonzero((v >= 0) & (v < n_in))[0]
        num[k] = outs.size
        pairs[k, 0, :outs.size], pairs[k, 1, :outs.size] = v[outs], outs
    return pairs, num
