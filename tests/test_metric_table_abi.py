"""The device-resident evaluation tables without a GPU (include/dclnet_hip.h: "device-resident eval tables"): the entries are
declared with the documented argument lists, exported by both libraries and refuse bad arguments before any device work; the
host twin of the tabulation (dcl_metric_tabulate_host) and the tables on CPU tensors (sharding.Device*Table(device="cpu"))
equal the host classes fed the same floats -- on the reference-generated fixtures, on the edge distances and over two gloo
ranks; `make hostcheck` runs the twin under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import metric_table_cases as MC
from test_conv_pairs_abi import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TAB = ["int mode", "int T", "int b", "int C", "const float *dis", "const int32_t *cls", "const int32_t *valid",
        "const double *diameter", "double *sums", "double *maxd", "int64_t *counts", "int32_t *bad"]
WANT = {
    "dcl_add_traj": ["int T", "int b", "int P", "int n_clouds", "const float *cld", "const int32_t *cls", "const int32_t *sym",
                     "int all_mode", "const float *R_pred", "const float *t_pred", "const float *R_gt", "const float *t_gt",
                     "const int32_t *valid", "float *partial_scratch", "float *dis", "dclStream_t stream"],
    "dcl_metric_tabulate": _TAB + ["dclStream_t stream"],
    "dcl_metric_tabulate_host": _TAB,
    "dcl_add_tabulate": ["int mode", "int T", "int b", "int P", "int n_clouds", "int C", "const float *cld", "const int32_t *cloud",
                         "const int32_t *cls", "const int32_t *sym", "int all_mode", "const float *R_pred", "const float *t_pred",
                         "const float *R_gt", "const float *t_gt", "const int32_t *valid", "const double *diameter",
                         "float *partial_scratch", "float *dis", "double *sums", "double *maxd", "int64_t *counts", "int32_t *bad",
                         "dclStream_t stream"],
}


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


# ------------------------------------------------------------------------------------------- 1. the ABI
def test_header_declares_the_entries_and_both_libraries_export_them(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    header = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    for name, value in (("DCL_TABLE_ADDS", 0), ("DCL_TABLE_LM", 1), ("DCL_TABLE_LMO", 2), ("DCL_ABI_VERSION", 2)):
        assert "#define %s %d\n" % (name, value) in header, name
    assert dcl.ops.TABLE_MODES == {"adds": 0, "lm": 1, "lmo": 2}
    for op in ("add_traj", "metric_tabulate", "metric_tabulate_host", "add_tabulate", "metric_table_arrays"):
        assert callable(getattr(dcl.ops, op)), op
    nm = subprocess.run(["nm", "-D", dcl._native.SO_PATH], capture_output=True, text=True).stdout
    assert "dcl_metric_tabulate" in nm and "dcl_debug" not in nm                   # the product library: no hooks


_HOST = (C.c_int64 * 4096)()            # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)


def _tabulate(L, host, mode=0, T=1, b=1, Cn=2, dis=_P, cls=_P, valid=None, diameter=_P, sums=_P, maxd=_P, counts=_P, bad=_P):
    a = (mode, T, b, Cn, dis, cls, valid, diameter, sums, maxd, counts, bad)
    return L.dcl_metric_tabulate_host(*a) if host else L.dcl_metric_tabulate(*(a + (None,)))


def _traj(L, T=1, b=1, P=8, n_clouds=1, cld=_P, cls=None, sym=None, all_mode=1, Rp=_P, tp=_P, Rg=_P, tg=_P, valid=None, part=_P,
          dis=_P):
    return L.dcl_add_traj(T, b, P, n_clouds, cld, cls, sym, all_mode, Rp, tp, Rg, tg, valid, part, dis, None)


def _fused(L, mode=0, T=1, b=1, P=8, n_clouds=1, Cn=2, cld=_P, cloud=None, cls=_P, sym=None, all_mode=1, Rp=_P, tp=_P, Rg=_P,
           tg=_P, valid=None, diameter=_P, part=_P, dis=None, sums=_P, maxd=_P, counts=_P, bad=_P):
    return L.dcl_add_tabulate(mode, T, b, P, n_clouds, Cn, cld, cloud, cls, sym, all_mode, Rp, tp, Rg, tg, valid, diameter, part,
                              dis, sums, maxd, counts, bad, None)


_BAD_TAB = [dict(mode=3), dict(mode=-1), dict(T=0), dict(b=-1), dict(Cn=0), dict(Cn=(1 << 20) + 1), dict(dis=None), dict(cls=None),
            dict(bad=None), dict(sums=None), dict(maxd=None), dict(mode=1, counts=None), dict(mode=1, diameter=None),
            dict(mode=2, counts=None), dict(mode=2, diameter=None)]
_BAD_TRAJ = [dict(T=0), dict(b=-1), dict(P=0), dict(P=12801), dict(b=65536), dict(all_mode=2), dict(all_mode=-1), dict(cld=None),
             dict(Rp=None), dict(tp=None), dict(Rg=None), dict(tg=None), dict(part=None), dict(n_clouds=-1),
             dict(b=2, n_clouds=1)]


def test_bad_arguments_return_einval_without_a_gpu(dcl):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        for host in (False, True):
            for kw in _BAD_TAB:
                assert _tabulate(lib, host, **kw) == -1, (tag, host, kw)
                assert b"invalid argument" in lib.dcl_last_error(), tag
            # an empty batch: nothing is launched, nothing dereferenced -- and the arrays the mode does not use may be NULL
            assert _tabulate(lib, host, b=0, dis=None, cls=None, counts=None, diameter=None) == 0, (tag, host)
            assert _tabulate(lib, host, mode=1, b=0, dis=None, cls=None, sums=None, maxd=None) == 0, (tag, host)
        for kw in _BAD_TRAJ:
            assert _traj(lib, **kw) == -1, (tag, kw)
            assert _fused(lib, **kw) == -1, (tag, kw)
        assert _traj(lib, dis=None) == -1 and _fused(lib, cls=None) == -1, tag
        for kw in _BAD_TAB:
            if "dis" not in kw and "cls" not in kw:
                assert _fused(lib, **kw) == -1, (tag, kw)
        assert _traj(lib, b=0, cld=None, Rp=None, tp=None, Rg=None, tg=None, part=None, dis=None) == 0, tag
        assert _fused(lib, b=0, cld=None, cls=None, Rp=None, tp=None, Rg=None, tg=None, part=None) == 0, tag


def test_wrappers_refuse_the_wrong_side_and_the_wrong_shape(dcl):
    arr = dcl.ops.metric_table_arrays("adds", 2, 3)
    cls, dis = torch.zeros(4, dtype=torch.int32), torch.zeros((2, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        dcl.ops.metric_tabulate(arr, dis, cls)                                       # CPU arrays: the twin's, not the kernel's
    with pytest.raises(AssertionError, match="steps"):
        dcl.ops.metric_tabulate_host(arr, dis[:1], cls)
    with pytest.raises(ValueError, match="mode"):
        dcl.ops.metric_table_arrays("ycbv")
    with pytest.raises(RuntimeError, match="diameter"):
        dcl.ops.metric_tabulate_host(dcl.ops.metric_table_arrays("lm", 2, 3), dis, cls, mode="lm")
    tab = dcl.sharding.DeviceAddsTable(3, steps=2, device="cpu")
    with pytest.raises(ValueError, match="step"):
        tab.add_distances(cls, dis[0])
    with pytest.raises(ValueError, match="step"):
        tab.add_frame(torch.zeros(3, 8, 3), cls, torch.zeros(3, 4, 3, 3), torch.zeros(3, 4, 3), torch.zeros(4, 3, 3), torch.zeros(4, 3))
    assert "ONE stream" in dcl.sharding.DeviceAddsTable.__doc__ and "ONE stream" in dcl.sharding.DeviceLmoTable.__doc__


# ------------------------------------------------------------------------------------------- 2. the edge cases
def test_host_twin_equals_the_host_classes_on_every_edge_case(dcl):
    assert float(MC.EDGE[1]) > 0.1 and float(MC.EDGE[3]) < 0.02 and float(MC.EDGE[0]) < 0.1          # why double is pinned
    cases = MC.edge_cases()
    assert {c["b"] for c in cases} >= {0, 1, 7} and {c["C"] for c in cases} == set(MC.CLASSES) and {c["T"] for c in cases} == {1, 3}
    for case in cases:
        arr = MC.new_arrays(dcl, case)
        dis, cls, valid, diam = MC.tensors(case)
        dcl.ops.metric_tabulate_host(arr, dis, cls, valid, mode=case["mode"], diameter=diam)
        want = MC.expected(dcl, case)
        MC.assert_equals_expected(arr, want, case["mode"], case["name"])
        if "bad ids" in case["name"]:
            assert want[3] == 1
        # ... and the table class on CPU tensors, through add_distances, accumulating a second identical frame
        S = dcl.sharding
        tab = S.DeviceAddsTable(case["C"], case["T"], "cpu") if case["mode"] == "adds" else \
            (S.DeviceLmTable if case["mode"] == "lm" else S.DeviceLmoTable)(case["diameter"], case["T"], "cpu")
        tab.add_distances(cls, dis, valid)
        MC.assert_equals_expected(tab.arrays, want, case["mode"], case["name"])
        if want[3]:
            with pytest.raises(ValueError, match="class id"):
                tab.finalize()


def test_known_answers_at_the_thresholds(dcl):
    """written out by hand, not through the host classes: 0.1f is NOT <= 0.1, 0.02f IS < 0.02; NaN / inf are misses"""
    arr = dcl.ops.metric_table_arrays("adds", 1, 1)
    dcl.ops.metric_tabulate_host(arr, torch.from_numpy(MC.EDGE.copy()), torch.zeros(8, dtype=torch.int32))
    n, m, sd, c2 = arr["sums"][0, 0].tolist()
    inside = [float(MC.EDGE[k]) for k in (0, 2, 3, 4, 5)]                              # every one but 0.1f, NaN, inf
    assert (n, m, c2) == (8.0, 5.0, 4.0) and float(arr["maxd"][0, 0]) == float(MC.EDGE[0])
    acc = 0.0
    for d in inside:
        acc += d
    assert sd == acc
    d = np.array([0.005, 0.005, 0.005], np.float64)
    for mode, num in (("lm", 2), ("lmo", 3)):
        arr = dcl.ops.metric_table_arrays(mode, 1, 3)
        dcl.ops.metric_tabulate_host(arr, torch.tensor([0.004, float("nan"), 0.001], dtype=torch.float32),
                                     torch.tensor([1, 1, 1], dtype=torch.int32), torch.tensor([1, 1, 0], dtype=torch.int32),
                                     mode=mode, diameter=torch.from_numpy(d))
        assert arr["counts"][0].tolist() == [[0, 0], [num, 1], [0, 0]]


# ------------------------------------------------------------------------------------------- 3. the fixtures
@pytest.mark.parametrize("frame", [1, 6, 33])
def test_ycbv_golden_through_the_cpu_table(dcl, golden_dir, frame):
    """tests/golden/metric_ref.npz (the reference's cal_auc_acc / cal_metric_auc_acc): the distances rounded to fp32, the finite
    ones valid and the inf ones valid = 0, in file order, `frame` crops per call"""
    z = np.load(os.path.join(golden_dir, "metric_ref.npz"))
    for case in range(6):
        d, idx = z["d%d" % case], z["idx%d" % case].astype(np.int32)
        assert 220 <= len(d) <= 349 and 9 <= int(np.isinf(d).sum()) <= 44
        d32 = d.astype(np.float32)
        host = dcl.sharding.AddsTable()
        for c, x in zip(idx, d32):
            host.add(int(c), float(np.float32(x)))
        tab = dcl.sharding.DeviceAddsTable(device="cpu")
        for s in range(0, len(d), frame):
            dd, valid = d32[s:s + frame].copy(), np.isfinite(d32[s:s + frame]).astype(np.int32)
            dd[valid == 0] = 0.0                                                  # an invalid crop's distance is not looked at
            tab.add_distances(torch.from_numpy(idx[s:s + frame].copy()), torch.from_numpy(dd), torch.from_numpy(valid))
        got = tab.to_host()
        assert MC.bits(got.sums) == MC.bits(host.sums) and MC.bits(got.maxd) == MC.bits(host.maxd)
        mean_auc, mean_acc, auc, acc = tab.finalize()
        assert np.abs(auc - z["auc%d" % case]).max() <= 1e-4
        assert np.abs(acc - z["acc%d" % case]).max() <= 1e-9
        assert abs(mean_auc - float(z["mean_auc%d" % case][0])) <= 0.0100001      # both rounded to 2 decimals
        if "mean_acc%d" % case in z.files:
            assert abs(mean_acc - float(z["mean_acc%d" % case][0])) <= 0.0100001


def _lm_feed(z, table, lost_by, frames=None):
    """one fixture frame per call: the detected objects' distances, and the lost ones (flag -1) either through add_lost
    (where the fixture names them) or as valid = 0 crops"""
    n_lost = 0
    for f in (range(int(z["n_frames"][0])) if frames is None else frames):
        flags, idx = z["f%d_flags" % f], z["f%d_idx" % f].astype(np.int32)
        det = flags != -1
        d = np.where(flags[det] != 0, z["f%d_cd" % f], z["f%d_l2" % f]).astype(np.float32)
        with_lost = len(idx) == len(flags)                                        # the collate names the lost object too
        n_lost += int((~det).sum())
        if not with_lost:                                                         # LineMOD: lost detections carry no index
            table.add_distances(torch.from_numpy(idx), torch.from_numpy(d))
        elif lost_by == "add_lost":
            table.add_distances(torch.from_numpy(idx[det].copy()), torch.from_numpy(d))
            table.add_lost(idx[~det])
        else:
            full = np.zeros(len(flags), np.float32)
            full[det] = d
            table.add_distances(torch.from_numpy(idx), torch.from_numpy(full), torch.from_numpy(det.astype(np.int32)))
    return n_lost


@pytest.mark.parametrize("lost_by", ["add_lost", "valid"])
def test_linemod_goldens_through_the_cpu_tables(dcl, golden_dir, lost_by):
    z = np.load(os.path.join(golden_dir, "lm_metric_ref.npz"))
    lm = dcl.sharding.DeviceLmTable(z["diameter"], device="cpu")
    assert _lm_feed(z, lm, lost_by) > 0
    # LineMOD drops a lost detection: fed explicitly, by either route, it still changes nothing
    lm.add_lost([0, 3]) if lost_by == "add_lost" else lm.add_distances(torch.tensor([0, 3], dtype=torch.int32), torch.zeros(2),
                                                                      torch.zeros(2, dtype=torch.int32))
    got = lm.to_host()
    assert type(got) is dcl.sharding.LmTable
    assert np.array_equal(got.counts[:, 0], z["num_count"]) and np.array_equal(got.counts[:, 1], z["success_count"])
    assert abs(lm.finalize()[0] - z["success_count"].sum() / z["num_count"].sum()) <= 1e-12
    z = np.load(os.path.join(golden_dir, "lmo_metric_ref.npz"))
    lmo = dcl.sharding.DeviceLmoTable(z["diameter"], device="cpu")
    assert _lm_feed(z, lmo, lost_by) >= 5
    got = lmo.to_host()
    assert type(got) is dcl.sharding.LmoTable
    assert np.array_equal(got.counts[:, 0], z["num_count"]) and np.array_equal(got.counts[:, 1], z["success_count"])
    assert int(got.counts[:, 0].sum()) == int(z["n_frames"][0])                   # every frame counted, the lost ones included


def test_add_frame_on_cpu_tensors_scores_every_step(dcl):
    """device="cpu": the distances come from sharding.add_s's torch form, the table from the twin; three steps in one call"""
    p = MC.pose_case(5, 3, 4, 40, 6)
    valid = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    tab = dcl.sharding.DeviceAddsTable(6, steps=3, device="cpu")
    tab.add_frame(p["cld"], p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid)
    for t in range(3):
        host = dcl.sharding.AddsTable(6)
        d = dcl.sharding.add_s(p["cld"][p["cls"].long()], p["Rp"][t], p["tp"][t], p["Rg"], p["tg"])
        for i in range(4):
            host.add(int(p["cls"][i]), float(d[i]) if valid[i] else float("inf"))
        got = tab.to_host(t)
        assert MC.bits(got.sums) == MC.bits(host.sums) and MC.bits(got.maxd) == MC.bits(host.maxd)
    assert tab.finalize()[0] == tab.to_host(-1).finalize()[0]


# ------------------------------------------------------------------------------------------- 4. two ranks
WORKER = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np, torch, torch.distributed as dist
    sys.path.insert(0, %r)
    dcl = importlib.import_module("dcl-net_amd")
    S = dcl.sharding
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    z = np.load(%r)
    d32, idx = z["d0"].astype(np.float32), z["idx0"].astype(np.int32)
    frames = [(s, min(s + 6, len(d32))) for s in range(0, len(d32), 6)]

    def feed(table, which):
        for f in which:
            a, b = frames[f]
            table.add_distances(torch.from_numpy(idx[a:b].copy()), torch.from_numpy(np.where(np.isfinite(d32[a:b]), d32[a:b], 0).astype(np.float32)),
                                torch.from_numpy(np.isfinite(d32[a:b]).astype(np.int32)))
        return table
    whole = feed(S.DeviceAddsTable(device="cpu"), range(len(frames)))
    shards = [feed(S.DeviceAddsTable(device="cpu"), S.shard_indices(len(frames), r, world)) for r in range(world)]
    mine = shards[rank]
    assert float(mine.sums[0, :, 0].sum()) < float(whole.sums[0, :, 0].sum())                # really a shard
    same = lambda a, b: a.numpy().tobytes() == b.numpy().tobytes()
    parts = [s.sums[..., 2].clone() for s in shards]
    mine.reduce()
    assert same(mine.maxd, whole.maxd) and same(mine.sums[..., [0, 1, 3]], whole.sums[..., [0, 1, 3]])
    assert same(mine.sums[..., 2], parts[0] + parts[1])
    assert np.abs((mine.sums[..., 2] - whole.sums[..., 2]).numpy()).max() <= 1e-12
    # the LineMOD tables: integer counts, exact
    zl = np.load(%r)
    n = int(zl["n_frames"][0])
    lm = S.DeviceLmTable(zl["diameter"], device="cpu")
    for f in S.shard_indices(n, rank, world):
        flags = zl["f%%d_flags" %% f]
        d = np.where(flags[flags != -1] != 0, zl["f%%d_cd" %% f], zl["f%%d_l2" %% f]).astype(np.float32)
        lm.add_distances(torch.from_numpy(zl["f%%d_idx" %% f].astype(np.int32)), torch.from_numpy(d))
    assert int(lm.counts[0, :, 0].sum()) < int(zl["num_count"].sum())
    got = lm.reduce().to_host()
    assert np.array_equal(got.counts[:, 0], zl["num_count"]) and np.array_equal(got.counts[:, 1], zl["success_count"])
    dist.destroy_process_group()
    print("rank", rank, "ok", mine.finalize()[0], got.finalize()[0])
''')


def test_cpu_tables_allreduce_two_processes_gloo(tmp_path, golden_dir):
    """device="cpu" tables sharded by shard_indices over 2 gloo ranks: after reduce() counts and maxd equal the single-process
    table exactly, sum D equals the float64 sum of the two shard sums"""
    script = tmp_path / "metric_table_worker.py"
    script.write_text(WORKER % (ROOT, os.path.join(golden_dir, "metric_ref.npz"), os.path.join(golden_dir, "lm_metric_ref.npz")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29553", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_reduce_is_a_no_op_without_a_process_group(dcl):
    tab = dcl.sharding.DeviceAddsTable(3, device="cpu")
    tab.add_distances(torch.tensor([1], dtype=torch.int32), torch.tensor([0.01]))
    before = MC.bits(tab.sums)
    assert tab.reduce() is tab and MC.bits(tab.sums) == before


# ------------------------------------------------------------------------------------------- 5. the sanitizer build of the twin
def test_make_hostcheck_runs_clean():
    """`make hostcheck`: the host twins as stand-alone CPU programs under AddressSanitizer + UBSan (nothing is loaded into
    Python under a sanitizer)"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dcl-net_amd", "csrc"), "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "metric_table_host_check: ok" in r.stdout and "crop_draw_host_check: ok" in r.stdout
