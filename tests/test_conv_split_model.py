"""CPU-only checks of the split-bf16 sparse conv's host side (no GPU, no library call): the layout of the prepared filter planes
(ops.conv_split_planes is the inverse of the kernel's order), the exactness of the three-piece split on filters, the size of what
the six kept products drop, the exact-operand families the GPU test relies on, and the shape-only selection table."""
import importlib

import numpy as np
import torch

import conv_split_cases as CS


def test_planes_layout_round_trip_and_exact_sum():
    dcl = importlib.import_module("dcl-net_amd")
    for cin, cout in ((32, 64), (64, 128), (128, 256)):
        rng = np.random.default_rng(cin)
        w = torch.from_numpy((rng.normal(size=(27, cin, cout)) * 2.0 ** rng.integers(-20, 20, (27, cin, cout))).astype(np.float32))
        model = CS.model_planes(w)                                          # kernel order, float32 holding bf16 values
        assert tuple(model.shape) == (27, cin // 32, cout // 64, 3, 2, 2, 64, 8)
        assert model.numel() * 2 == 27 * cin * cout * 6                     # bytes of the three bf16 planes
        as_bytes = model.to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1)
        back = dcl.ops.conv_split_planes(as_bytes, cin, cout)               # (3, 27, cin, cout)
        assert torch.equal(back.double().sum(0), w.double())                # h + m + l == W exactly
        # element (plane p, offset k, channel c, column n) sits where the kernel reads it
        for p, k, c, n in ((0, 0, 0, 0), (1, 13, cin - 1, cout - 1), (2, 26, 17, 65 % cout), (0, 5, 24, 63)):
            chunk, s, h, j = c // 32, (c % 32) // 16, (c % 16) // 8, c % 8
            assert float(model[k, chunk, n // 64, p, s, h, n % 64, j]) == float(back[p, k, c, n])


def test_six_products_drop_less_than_an_fp32_rounding():
    """|model of the six exact products - float64| <= 3 * 2^-25 sum |x| |w| (the three dropped products, each <= 2^-8-8-9 ... of
    the product): well below one unit per accumulation step of an fp32 chain"""
    idx, nbr, x, w, val, mag = CS.host_case()
    got = CS.model_split_conv(x, w, nbr, idx.shape[0])
    u = CS.units(got, val, mag)
    assert float(u.max()) <= 1.5, float(u.max())


def test_exact_operand_families_are_exact_in_fp32():
    """every product and every partial sum of the exact families fits fp32: the float64 result, the fp32 rounding of it and the
    six-product model agree exactly, whatever the summation order"""
    idx, nbr, _, _, _, _ = CS.host_case()
    n = idx.shape[0]
    for kind in ("hh", "x3", "w3", "mm"):
        x, w = CS.exact_operands(kind, n, 32, 64, 5)
        val, mag = CS.reference64(x, w, nbr, n)
        assert float(mag.max()) < 2.0 ** 24 * float(min(np.abs(x[x != 0]).min() * np.abs(w[w != 0]).min(), 1.0)), kind
        assert torch.equal(val.float().double(), val), kind
        assert torch.equal(CS.model_split_conv(x, w, nbr, n), val), kind
        assert float(val.abs().max()) > 0, kind


def test_voxel_set_has_full_and_centre_only_rows():
    idx, nbr, _, _, _, _ = CS.host_case()
    present = (nbr >= 0).sum(0)
    assert (present == 27).sum() >= 8 and (present == 1).sum() >= 4
    assert (nbr[13] == np.arange(idx.shape[0])).all()                        # the centre is the row itself


def test_selection_is_by_shape_only():
    dcl = importlib.import_module("dcl-net_amd")
    ops = dcl.ops
    assert ops.conv_split_ok(27, 32, 64) and ops.conv_split_ok(27, 128, 256) and ops.conv_split_ok(27, 64, 64)
    assert not ops.conv_split_ok(27, 16, 32) and not ops.conv_split_ok(27, 32, 32) and not ops.conv_split_ok(8, 64, 64)
    assert ops.CONV_SPLIT_ROWS_PER_CROP == (3600, 1800, 900, 450)
    chans = ops.BACKBONE_CHANNELS
    for (cin, cout, subm), rows in ops.CONV_SPLIT_WIDTHS.items():
        assert ops.conv_split_ok(27, cin, cout) and isinstance(subm, bool)
        layer = [i for i in range(8) if (chans[i], chans[i + 1]) == (cin, cout) and bool(i % 2) == subm]
        assert len(layer) == 1
        # measured at 32 crops only: no launch of fewer crops (the one-crop and six-crop graph paths among them) takes the split form
        assert rows >= 32 * ops.CONV_SPLIT_ROWS_PER_CROP[layer[0] // 2]
    # the pointer array of a batch: NULL below the thresholds, pieces from them on (no GPU: the planes are stand-ins)
    pieces = ops.ConvSplitPieces.__new__(ops.ConvSplitPieces)
    pieces.meta = [((27, chans[i], chans[i + 1]), bool(i % 2)) for i in range(8)]
    pieces.planes = [torch.zeros(16, dtype=torch.uint8) if ops.conv_split_ok(27, chans[i], chans[i + 1]) else None for i in range(8)]
    pieces._arrs = {}
    assert pieces.ptrs(6) is None and pieces.ptrs(16) is None
    arr = pieces.ptrs(32)
    assert [bool(arr[i]) for i in range(8)] == [(chans[i], chans[i + 1], bool(i % 2)) in ops.CONV_SPLIT_WIDTHS for i in range(8)]
