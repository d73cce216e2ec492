"""AutoClip's device form without a GPU: the host twin of the kernels (ops.autoclip_observe_host -> dcl_autoclip_observe_host,
the same functions of csrc/optim_clip.h compiled for the host) against np.percentile and dcl.optim.AutoClip.observe bit for bit
after every step of every case of tests/autoclip_cases.py, the sorted buffer against np.sort, both parities of the ping-pong and
growth from capacity 2; the refusals of the C entries; the Python surface that needs no device.  `make hostcheck` (run by
tests/test_metric_table_abi.py) puts the twin under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import autoclip_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQS = AC.sequences()


def test_the_cases_cover_both_branches_of_the_lerp_and_stay_few():
    taken = {bool(AC.branch_of(n, q)) for seq in SEQS.values() for q in AC.PERCENTILES for n in range(len(seq))}
    assert taken == {True, False}
    assert len(SEQS) * len(AC.PERCENTILES) <= 57
    for name, seq in SEQS.items():
        assert seq.dtype == np.float64 and not np.signbit(seq).any(), name
    assert {len(s) for s in SEQS.values()} >= {1, 2, 3}
    assert sum(np.isinf(SEQS["one_inf"])) == 1 and sum(np.isinf(SEQS["two_inf"])) == 2 and np.isnan(SEQS["nan_at_5"][5])


@pytest.mark.parametrize("q", AC.PERCENTILES)
@pytest.mark.parametrize("name", sorted(SEQS))
def test_host_twin_equals_numpy_and_autoclip_after_every_step(dcl, name, q):
    seq = SEQS[name]
    twin = AC.HostClip(dcl.ops, q, capacity=2)
    host = dcl.optim.AutoClip(q)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # numpy's "invalid value" at inf - inf
        for step, x in enumerate(seq):
            x = float(x)
            twin.observe(x)
            scale = host.observe(x)
            history = seq[:step + 1]
            want = np.percentile(history, q)
            assert AC.bits(np.float64(twin.clip_value)) == AC.bits(np.float64(want)), (step, twin.clip_value, want)
            assert AC.bits(np.float64(twin.clip_value)) == AC.bits(np.float64(host.clip_value)), step
            assert AC.bits(np.float64(twin.scale)) == AC.bits(np.float64(scale)), (step, twin.scale, scale)
            assert AC.bits(twin.scale32) == AC.bits(np.float32(scale)), step
            assert AC.bits(np.float64(float(twin.out[0]))) == AC.bits(np.float64(x))
            assert AC.bits(twin.held) == AC.bits(np.sort(history)), step
            assert AC.bits(twin.arrival[:step + 1]) == AC.bits(history)
            assert AC.bits(twin.beyond) == AC.bits(np.full(twin.capacity - twin.n, np.nan)), "a write beyond the n + 1 entries"
            assert 0.0 <= twin.scale <= 1.0
    if len(seq) > 2:
        assert twin.grown >= 1                                          # growth from capacity 2; both parities came by


def test_ties_go_behind_their_equals(dcl):
    """the new entry lands behind equal ones: seen through the position of the one store of x among entries of other bits"""
    ops = dcl.ops
    src = torch.tensor([1.0, 2.0, 2.0, 3.0], dtype=torch.float64)
    for x, at in ((2.0, 3), (0.5, 0), (3.0, 4), (9.0, 4), (1.0, 1)):
        dst = torch.full((5,), -7.0, dtype=torch.float64)
        arrival = torch.full((5,), -7.0, dtype=torch.float64)
        marked = src.clone()
        out = torch.zeros(AC.OUT_DOUBLES, dtype=torch.float64)
        ops.autoclip_observe_host(4, marked, dst, arrival, torch.tensor([x], dtype=torch.float64), 50, out)
        want = src.tolist()
        want.insert(at, x)
        assert dst.tolist() == want and arrival.tolist() == [-7.0] * 4 + [x]
    # NaN is behind inf, and a second NaN behind the first (told apart by their payloads)
    nan2 = np.frombuffer(np.uint64(0x7FF8000000000001).tobytes(), dtype=np.float64)[0]
    src = torch.tensor([1.0, np.inf, np.nan], dtype=torch.float64)
    dst = torch.zeros(4, dtype=torch.float64)
    ops.autoclip_observe_host(3, src, dst, torch.zeros(4, dtype=torch.float64), torch.from_numpy(np.array([nan2])), 50,
                              torch.zeros(AC.OUT_DOUBLES, dtype=torch.float64))
    assert AC.bits(dst) == AC.bits(np.array([1.0, np.inf, np.nan, nan2]))
    ops.autoclip_observe_host(3, src, dst, torch.zeros(4, dtype=torch.float64), torch.tensor([np.inf], dtype=torch.float64), 50,
                              torch.zeros(AC.OUT_DOUBLES, dtype=torch.float64))
    assert AC.bits(dst) == AC.bits(np.array([1.0, np.inf, np.inf, np.nan]))


def test_bad_arguments_return_einval_before_any_work(dcl):
    lib = dcl._native.lib()
    assert lib.dcl_abi_version() == 2
    src = np.array([1.0, 2.0])
    dst, arr = np.full(3, -7.0), np.full(3, -7.0)
    x, out = np.array([1.5]), np.full(AC.OUT_DOUBLES, -7.0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    null = C.c_void_p(0)
    good = [2, p(src), p(dst), p(arr), p(x), 50.0, p(out)]
    for at, bad in ((0, -1), (0, (1 << 31) + 1), (1, null), (2, null), (3, null), (4, null), (6, null), (1, p(dst)), (5, -0.5),
                    (5, 100.25), (5, float("nan"))):
        args = list(good)
        args[at] = bad
        assert lib.dcl_autoclip_observe_host(*args) == -1, (at, bad)
        assert b"invalid argument" in lib.dcl_last_error()
        # the device entry refuses the same before any GPU call (no GPU is needed to be refused)
        assert lib.dcl_autoclip_observe(*(args + [null])) == -1, (at, bad)
    assert (dst == -7.0).all() and (arr == -7.0).all() and (out == -7.0).all()
    assert lib.dcl_autoclip_observe_host(*good) == 0
    assert dst.tolist() == [1.0, 1.5, 2.0] and arr[2] == 1.5 and out[:3].tolist() == [1.5, 1.5, 1.5 / (1.5 + 1e-6)]
    assert lib.dcl_autoclip_observe_host(0, null, p(dst), p(arr), p(x), 50.0, p(out)) == 0       # n == 0: no source needed
    # dcl_adam_step_dev: dcl_adam_step's refusals, and a NULL or misaligned factor pointer
    f = C.c_float
    tab = np.zeros(48, dtype=np.uint8)
    ct, cb = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    one = np.ones(2, dtype=np.float32)
    assert lib.dcl_adam_step_dev(-1, p(tab), 1, p(ct), p(cb), p(one), f(0.5), f(0.999), f(1e-6), null) == -1
    assert lib.dcl_adam_step_dev(1, p(tab), 1, p(ct), p(cb), null, f(0.5), f(0.999), f(1e-6), null) == -1
    assert lib.dcl_adam_step_dev(1, p(tab), 1, p(ct), p(cb), C.c_void_p(one.ctypes.data + 2), f(0.5), f(0.999), f(1e-6), null) == -1
    assert lib.dcl_adam_step_dev(1, p(tab), 1, p(ct), p(cb), p(one), f(1.0), f(0.999), f(1e-6), null) == -1
    assert lib.dcl_adam_step_dev(1, p(tab), 1, p(ct), p(cb), p(one), f(0.5), f(0.999), f(0.0), null) == -1
    assert lib.dcl_adam_step_dev(1, null, 1, p(ct), p(cb), p(one), f(0.5), f(0.999), f(1e-6), null) == -1
    assert lib.dcl_adam_step_dev(0, null, 0, null, null, null, f(0.5), f(0.999), f(1e-6), null) == 0


def test_the_python_surface(dcl):
    ops, optim = dcl.ops, dcl.optim
    assert ops.AUTOCLIP_OUT_DOUBLES * 8 == 32 and ops.AUTOCLIP_SCALE_F32_INDEX * 4 == 24     # the header's two constants
    header = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert "#define DCL_AUTOCLIP_OUT_BYTES 32" in header and "#define DCL_AUTOCLIP_SCALE_F32_OFFSET 24" in header
    for name in ("autoclip_observe", "autoclip_observe_host", "adam_step_dev"):
        assert callable(getattr(ops, name))
    with pytest.raises(TypeError, match="dcl.optim.Adam"):
        optim.DeviceAutoClip(50)
    with pytest.raises(TypeError, match="dcl.optim.Adam"):
        optim.DeviceAutoClip(50, optimizer=torch.optim.Adam([torch.zeros(1, requires_grad=True)]))
    cpu = [torch.zeros(n, dtype=torch.float64) for n in (2, 3, 3, 1, AC.OUT_DOUBLES)]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.autoclip_observe(2, cpu[0], cpu[1], cpu[2], cpu[3], 50, cpu[4])
    # AutoClip is what it was: same keys, a plain list, no new attribute
    a = optim.AutoClip(50)
    a.observe(2.0)
    assert a.state_dict() == {"percentile": 50, "history": [2.0]} and sorted(vars(a)) == ["_ring", "clip_value", "history",
                                                                                         "optimizer", "percentile"]
    text = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert "--autoclip" in text and "DeviceAutoClip" in text
    assert "DeviceAutoClip" in open(os.path.join(ROOT, "tools", "bench_optim.py")).read()
    make = open(os.path.join(ROOT, "dcl-net_amd", "csrc", "Makefile")).read()
    assert "optim_clip_host.cpp" in make and "autoclip_host_check" in make
