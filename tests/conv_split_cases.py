"""Shared cases and host models of the split-bf16 sparse-conv tests (test_conv_split_model.py on the CPU,
test_gpu_conv_split.py on the GPU): voxel sets with prescribed neighbourhoods, operand families, the float64 reference over a
gather table, the error unit of tests/split_cases.py (2^-24 (sum |x| |w| + |bias|) per output) and a host model of the prepared
filter planes.  References are computed once per case (functools.lru_cache) and never modified."""
import functools

import numpy as np
import torch

from split_cases import PRODUCTS, rn_bf16, split3

WIDTHS = ((32, 64, True), (64, 128, True), (128, 256, True), (64, 64, False), (128, 128, False))


# ------------------------------------------------------------------------------------------------------------ voxel sets
def voxel_set(b, S, n_per_crop, seed):
    """(n, 4) int32 [b, x, y, z], sorted by linear index inside each crop, exactly n_per_crop voxels per crop: a full 4^3 block
    (its 8 interior voxels have all 27 neighbours), isolated voxels on a stride-3 lattice of one slab (only the centre), and
    random filling in between."""
    rng = np.random.default_rng(seed)
    rows = []
    for c in range(b):
        keep = set()
        for x in range(1, 5):
            for y in range(1, 5):
                for z in range(1, 5):
                    keep.add((x, y, z))
        for x in range(8, S - 1, 3):                              # isolated: a slab the random filling stays out of
            for y in range(1, S - 1, 3):
                keep.add((x, y, S - 2))
        assert len(keep) <= n_per_crop, (len(keep), n_per_crop)
        while len(keep) < n_per_crop:
            x, y, z = (int(v) for v in rng.integers(0, S, 3))
            if z >= S - 4 and x >= 6:                             # keep clear of the isolated slab
                continue
            keep.add((x, y, z))
        pts = sorted(keep, key=lambda p: (p[0] * S + p[1]) * S + p[2])
        rows += [(c,) + p for p in pts]
    return np.asarray(rows, np.int32)


# --------------------------------------------------------------------------------------------------------------- operands
def exact_operands(kind, n_in, cin, cout, seed):
    """features / filters whose every piece product and partial sum is exact in fp32, so the split form must reproduce the fp32
    form bit for bit:
      "hh"    small integers times powers of two on both sides (one piece each)
      "x3"    18-bit features (all three pieces) against filters that are signed powers of two or zero
      "w3"    the same with the roles swapped (a row has few non-zero channels so the sums stay below 2^24 granules)
      "mm"    one-hot rows of 9-bit integers against 10-bit integer filters: the products xh wh, xm wh, xh wm and xm wm
              are all present, nothing is dropped, every sum stays below 2^24"""
    rng = np.random.default_rng(seed)
    if kind == "hh":
        x = rng.integers(-3, 4, (n_in, cin)) * 2.0 ** rng.integers(0, 2, (n_in, cin))
        w = rng.integers(-3, 4, (27, cin, cout)) * 2.0 ** rng.integers(-1, 1, (27, cin, cout))
    elif kind == "x3":
        x = rng.integers(-(2 ** 17), 2 ** 17, (n_in, cin)).astype(np.float64) * 2.0 ** -18
        x *= rng.random((n_in, cin)) < 0.25                      # sum of <= 27 * cin terms of 18 bits: keep it sparse
        w = np.sign(rng.integers(-1, 2, (27, cin, cout))) * 2.0 ** rng.integers(-1, 1, (27, cin, cout))
        w *= rng.random((27, cin, cout)) < 4.0 / cin             # about four non-zero channels per column and offset
    elif kind == "w3":
        w = rng.integers(-(2 ** 17), 2 ** 17, (27, cin, cout)).astype(np.float64) * 2.0 ** -18
        w *= rng.random((27, cin, cout)) < 4.0 / cin
        x = np.sign(rng.integers(-1, 2, (n_in, cin))) * 2.0 ** rng.integers(-1, 1, (n_in, cin))
        x *= rng.random((n_in, cin)) < 0.25
    elif kind == "mm":
        x = np.zeros((n_in, cin))
        x[np.arange(n_in), rng.integers(0, cin, n_in)] = rng.integers(-(2 ** 9) + 1, 2 ** 9, n_in)
        w = rng.integers(-(2 ** 10) + 1, 2 ** 10, (27, cin, cout)).astype(np.float64)
    else:
        raise KeyError(kind)
    return x.astype(np.float32), w.astype(np.float32)


def error_operands(kind, n_in, cin, cout, seed):
    """"gauss": N(0, 1) features, N(0, 1 / (27 cin)) filters; "cancel": every channel pair (2 i, 2 i + 1) carries nearly opposite
    contributions, so the outputs are small against sum |x| |w|; "range": magnitudes spread over 2^-12 .. 2^12, random signs."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_in, cin))
    w = rng.normal(size=(27, cin, cout)) / np.sqrt(27 * cin)
    if kind == "cancel":
        x[:, 1::2] = x[:, 0::2] * (1 + 2.0 ** -10 * rng.normal(size=(n_in, cin // 2)))
        w[:, 1::2, :] = -w[:, 0::2, :] * (1 + 2.0 ** -10 * rng.normal(size=(27, cin // 2, cout)))
    elif kind == "range":
        x *= 2.0 ** rng.integers(-12, 13, (n_in, cin))
        w *= 2.0 ** rng.integers(-12, 13, (27, cin, cout))
    elif kind != "gauss":
        raise KeyError(kind)
    return x.astype(np.float32), w.astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- references
def reference64(x, w, nbr, n_out):
    """float64 conv over a gather table nbr (27, cap) (-1 = no neighbour) -> (value, magnitude sum |x| |w|), both (n_out, cout)"""
    x64, w64 = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(w, dtype=torch.float64)
    nb = torch.as_tensor(nbr)[:, :n_out].long()
    val = torch.zeros((n_out, w64.shape[2]), dtype=torch.float64)
    mag = torch.zeros_like(val)
    for k in range(w64.shape[0]):
        have = nb[k] >= 0
        rows = x64[nb[k].clamp(min=0)] * have[:, None]
        val += rows @ w64[k]
        mag += rows.abs() @ w64[k].abs()
    return val, mag


def units(got, val, mag):
    """per-output error in units of 2^-24 sum |x| |w| (outputs nobody contributes to must be exactly zero)"""
    err = (torch.as_tensor(got, dtype=torch.float64) - val).abs()
    dead = mag == 0
    assert bool((err[dead] == 0).all())
    return (err / (2.0 ** -24 * mag.masked_fill(dead, 1.0))).masked_fill(dead, 0.0)


# --------------------------------------------------------------------------------- host model of the prepared filter planes
def model_planes(w):
    """W (27, cin, cout) -> the three bf16 planes in the kernel's order, as float32 of shape
    (27, cin / 32, cout / 64, 3, 2, 2, 64, 8): [k][chunk][column tile][plane][k step s][lane half h][column][channel 16 s + 8 h + j]"""
    w = torch.as_tensor(w, dtype=torch.float32)
    kvol, cin, cout = w.shape
    pieces = torch.stack(split3(w, rn_bf16), 0)                                      # (3, k, cin, cout)
    v = pieces.reshape(3, kvol, cin // 32, 2, 2, 8, cout // 64, 64)                  # [p][k][chunk][s][h][j][by][col]
    return v.permute(1, 2, 6, 0, 3, 4, 7, 5).contiguous()


def model_split_conv(x, w, nbr, n_out):
    """the six piece products kept by the split form (xl wh, xh wl, xm wm, xm wh, xh wm, xh wh), each exact, summed in float64:
    what the kernel computes up to its fp32 accumulation"""
    xs = [p.double() for p in split3(torch.as_tensor(x, dtype=torch.float32), rn_bf16)]
    ws = [p.double() for p in split3(torch.as_tensor(w, dtype=torch.float32), rn_bf16)]
    nb = torch.as_tensor(nbr)[:, :n_out].long()
    out = torch.zeros((n_out, w.shape[2]), dtype=torch.float64)
    for k in range(w.shape[0]):
        have = (nb[k] >= 0)[:, None]
        g = nb[k].clamp(min=0)
        for a, b in PRODUCTS:
            out += (xs[a][g] * have) @ ws[b][k]
    return out


def host_nbr(idx, b, S, subm=True):
    """gather table of a k3 s1 p1 (submanifold) conv over the voxel set idx, on the host: (27, n) int32, offset k = (dx + 1) * 9 +
    (dy + 1) * 3 + (dz + 1), the reference's ascending offset order"""
    assert subm
    key = {tuple(int(v) for v in r): i for i, r in enumerate(idx)}
    nbr = np.full((27, idx.shape[0]), -1, np.int32)
    for i, (c, x, y, z) in enumerate(idx):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    j = key.get((int(c), int(x) + dx, int(y) + dy, int(z) + dz))
                    if j is not None:
                        nbr[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1), i] = j
    return nbr


@functools.lru_cache(maxsize=None)
def host_case(n_per_crop=150, S=12, cin=32, cout=64, seed=3):
    idx = voxel_set(1, S, n_per_crop, seed)
    nbr = host_nbr(idx, 1, S)
    x, w = error_operands("gauss", idx.shape[0], cin, cout, seed)
    val, mag = reference64(x, w, nbr, idx.shape[0])
    return idx, nbr, x, w, val, mag
