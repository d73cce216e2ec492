"""Shared cases of the device-resident evaluation tables (include/dclnet_hip.h: dcl_metric_tabulate): the edge distances and
shapes both the CPU tests (host twin) and the GPU tests (kernel) run, and the expectation -- the HOST classes of
dcl-net_amd/sharding.py fed the same floats crop by crop."""
import numpy as np
import torch

F = np.float32
INF = float("inf")
# nextafter(0.1f, 0), 0.1f, nextafter(0.02f, 0), 0.02f, 0, a subnormal, NaN, +inf  (0.1f > 0.1 and 0.02f < 0.02 in double)
EDGE = np.array([np.nextafter(F(0.1), F(0)), F(0.1), np.nextafter(F(0.02), F(0)), F(0.02), F(0), F(1e-42), F("nan"), F("inf")], F)
MODES = ("adds", "lm", "lmo")
CLASSES = (1, 21, 64, 65, 130)


def diameters(C):
    """per class: a diameter EQUAL to (double)d of a finite edge distance, one ulp above it, or an ordinary one"""
    d = np.empty(C, np.float64)
    for c in range(C):
        e = float(EDGE[c % 6])
        d[c] = e if c % 3 == 0 else np.nextafter(e, 1.0) if c % 3 == 1 else 0.015
    return d


def _case(name, mode, C, T, cls, dis, valid):
    cls = np.asarray(cls, np.int32).reshape(-1)
    dis = np.asarray(dis, F).reshape(T, len(cls))
    return dict(name=name, mode=mode, C=C, T=T, b=len(cls), cls=cls, dis=dis,
                valid=None if valid is None else np.asarray(valid, np.int32).reshape(-1), diameter=diameters(C))


def edge_cases():
    """every mode x C in {1, 21, 64, 65, 130} x T in {1, 3} x b in {0, 1, 7} with different distances per step, some crops
    invalid; all crops invalid; every edge distance valid and invalid in ONE class; a crop AT its class's diameter and one
    ulp below it; class ids -1 and C"""
    out = []
    for mode in MODES:
        k = 0
        for C in CLASSES:
            for T in (1, 3):
                for b in (0, 1, 7):
                    i = np.arange(b)
                    dis = [[EDGE[(j + 3 * t + k) % 8] for j in range(b)] for t in range(T)]
                    valid = None if k % 3 == 2 else ((i + k) % 4 != 3).astype(np.int32)
                    out.append(_case("%s C%d T%d b%d" % (mode, C, T, b), mode, C, T, (i * 5 + k) % C, dis, valid))
                    k += 1
                out.append(_case("%s C%d T%d all invalid" % (mode, C, T), mode, C, T, np.arange(7) % C,
                                 [[EDGE[(j + t) % 8] for j in range(7)] for t in range(T)], np.zeros(7, np.int32)))
        # all 8 edge distances, valid then invalid, into one class: the order of sum D and every comparison at once
        out.append(_case("%s one class" % mode, mode, 1, 3, np.zeros(16, np.int32),
                         [np.roll(np.concatenate([EDGE, EDGE]), t) for t in range(3)], [1] * 8 + [0] * 8))
        # a distance equal to its class's diameter (c % 3 == 0: a miss) and one ulp below it (c % 3 == 1: a hit)
        cs = [c for c in range(21) if c % 3 != 2]
        out.append(_case("%s at the diameter" % mode, mode, 21, 1, cs, [EDGE[c % 6] for c in cs], None))
        for C in (1, 21, 130):
            out.append(_case("%s C%d bad ids" % (mode, C), mode, C, 3, [0, -1, C, C - 1, 1 << 30],
                             [[0.01, 0.011, 0.012, 0.013, 0.014 + t] for t in range(3)], [1, 1, 1, 0, 0]))
    return out


def new_arrays(dcl, case, device="cpu"):
    return dcl.ops.metric_table_arrays(case["mode"], case["T"], case["C"], device)


def tensors(case, device="cpu"):
    """(dis, cls, valid, diameter) of a case as tensors on `device`"""
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    return to(case["dis"]), to(case["cls"]), to(case["valid"]), to(case["diameter"])


def expected(dcl, case):
    """the host classes fed crop by crop -> (sums (T,C,4), maxd (T,C), counts (T,C,2), bad) as numpy arrays"""
    S = dcl.sharding
    T, C, mode = case["T"], case["C"], case["mode"]
    sums, maxd, counts, bad = np.zeros((T, C, 4)), np.zeros((T, C)), np.zeros((T, C, 2), np.int64), 0
    for t in range(T):
        tab = S.AddsTable(C) if mode == "adds" else (S.LmTable if mode == "lm" else S.LmoTable)(case["diameter"])
        for i in range(case["b"]):
            c, d = int(case["cls"][i]), float(case["dis"][t, i])
            ok = case["valid"] is None or case["valid"][i] != 0
            if not 0 <= c < C:
                bad = 1
            elif mode == "adds":
                tab.add(c, d if ok else INF)
            elif ok:
                tab.add(c, d)
            elif mode == "lmo":
                tab.add_lost(c)
        if mode == "adds":
            sums[t], maxd[t] = tab.sums, tab.maxd
        else:
            counts[t] = tab.counts
    return sums, maxd, counts, bad


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def assert_equals_expected(arrays, want, mode, what=""):
    sums, maxd, counts, bad = want
    if mode == "adds":
        assert bits(arrays["sums"]) == bits(sums), (what, "sums")
        assert bits(arrays["maxd"]) == bits(maxd), (what, "maxd")
    else:
        assert bits(arrays["counts"]) == bits(counts), (what, "counts")
    assert int(arrays["bad"].cpu()[0]) == bad, (what, "bad")


# ---------------------------------------------------------------------------------------------- poses for the distance kernels
def rotations(gen, *lead):
    """random proper rotations (.., 3, 3) float32 by QR"""
    q, r = torch.linalg.qr(torch.randn(*lead, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)
    q[..., :, 0] *= torch.linalg.det(q).unsqueeze(-1)
    return q.float().contiguous()


def pose_case(seed, T, b, P, n_clouds):
    g = torch.Generator().manual_seed(seed)
    return dict(cld=(torch.randn(n_clouds, P, 3, generator=g) * 0.05), cls=torch.randint(0, n_clouds, (b,), generator=g).int(),
                Rp=rotations(g, T, b), tp=torch.randn(T, b, 3, generator=g) * 0.02, Rg=rotations(g, b),
                tg=torch.randn(b, 3, generator=g) * 0.02, sym=(torch.arange(b) % 2).int())
