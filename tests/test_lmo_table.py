"""sharding.LmoTable against the eval loop of the reference's tools/test_LMO.py (run from the reference source by
tests/golden/make_lmo_metric_golden.py): lost detections are counted into num_count, everything else is LmTable."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(golden_dir):
    z = np.load(os.path.join(golden_dir, "lmo_metric_ref.npz"))
    return z, [{k: z["f%d_%s" % (f, k)] for k in ("flags", "idx", "Rp", "tp", "Rg", "tg", "l2", "cd")}
               for f in range(int(z["n_frames"][0]))]


def test_object_list_and_symmetric_indices(dcl):
    T = dcl.sharding.LmoTable
    assert issubclass(T, dcl.sharding.LmTable)
    assert T.OBJLIST == (1, 5, 6, 8, 9, 10, 11, 12) and T.SYM_IDX == (5, 6)
    assert [T.OBJLIST[i] for i in T.SYM_IDX] == [10, 11]                      # eggbox, glue
    assert len(dcl.sharding.LmTable.OBJLIST) == 13 and not hasattr(dcl.sharding.LmTable, "add_lost")


def test_occlusion_linemod_metric_matches_reference_loop_golden(dcl, golden_dir):
    z, frames = _frames(golden_dir)
    clouds = torch.from_numpy(z["clouds"])
    table = dcl.sharding.LmoTable(z["diameter"])
    lost = 0
    for fr in frames:
        flags = fr["flags"]
        if flags[0] == -1:                                  # the loader's collate still names the lost object (:341-352)
            lost += 1
            table.add_batch(fr["idx"], [], flags)
            continue
        sym = torch.from_numpy(flags.astype(np.int32))
        assert int(sym[0]) == int(int(fr["idx"][0]) in table.SYM_IDX)
        d = dcl.sharding.add_lm(clouds[torch.from_numpy(fr["idx"]).long()], *[torch.from_numpy(fr[k]) for k in ("Rp", "tp", "Rg", "tg")],
                                sym)
        assert np.abs(d.numpy() - np.where(sym.numpy() != 0, fr["cd"], fr["l2"])).max() <= 1e-6
        table.add_batch(fr["idx"], d.tolist(), flags)
    assert lost >= 5
    assert np.array_equal(table.counts[:, 0], z["num_count"]) and np.array_equal(table.counts[:, 1], z["success_count"])
    assert int(table.counts[:, 0].sum()) == len(frames)                       # every frame counted, the lost ones included
    all_rate, per = table.finalize()
    assert abs(all_rate - z["success_count"].sum() / z["num_count"].sum()) <= 1e-12
    assert np.allclose(per, z["success_count"] / z["num_count"])


def test_add_lost_counts_the_attempt_only_and_lm_table_still_drops_it(dcl):
    d = np.full(8, 0.01)
    t = dcl.sharding.LmoTable(d)
    t.add_lost(3)
    t.add(3, 0.001)
    t.add(3, 0.5)
    assert t.counts[3].tolist() == [3, 1] and int(t.counts.sum()) == 4
    # a frame of three objects, the middle one lost: with its index it is counted, without it it is skipped as in LmTable
    a, b, lm = dcl.sharding.LmoTable(d), dcl.sharding.LmoTable(d), dcl.sharding.LmTable(d)
    a.add_batch([0, 1, 2], [0.001, 0.5], [0, -1, 1])
    b.add_batch([0, 2], [0.001, 0.5], [0, -1, 1])
    lm.add_batch([0, 2], [0.001, 0.5], [0, -1, 1])
    assert a.counts.tolist()[:3] == [[1, 1], [1, 0], [1, 0]]
    assert np.array_equal(b.counts, lm.counts) and lm.counts.tolist()[:3] == [[1, 1], [0, 0], [1, 0]]


def test_lm_table_results_are_unchanged(dcl, golden_dir):
    """LmTable on its own fixture, as before the subclass existed -- and the subclass fed the LineMOD way (indices of the
    detected objects only) drops lost detections exactly like it"""
    z = np.load(os.path.join(golden_dir, "lm_metric_ref.npz"))
    table, sub = dcl.sharding.LmTable(z["diameter"]), dcl.sharding.LmoTable(z["diameter"])
    lost = 0
    for f in range(int(z["n_frames"][0])):
        flags = z["f%d_flags" % f]
        d = np.where(flags[flags != -1] != 0, z["f%d_cd" % f], z["f%d_l2" % f])
        table.add_batch(z["f%d_idx" % f], d.tolist(), flags)
        sub.add_batch(z["f%d_idx" % f], d.tolist(), flags)
        lost += int((flags == -1).sum())
    assert lost > 0
    assert np.array_equal(table.counts[:, 0], z["num_count"]) and np.array_equal(table.counts[:, 1], z["success_count"])
    assert np.array_equal(sub.counts, table.counts)


WORKER = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np, torch, torch.distributed as dist
    sys.path.insert(0, %r)
    dcl = importlib.import_module("dcl-net_amd")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    z = np.load(%r)
    n = int(z["n_frames"][0])
    mine = dcl.sharding.LmoTable(z["diameter"])
    for f in dcl.sharding.shard_indices(n, rank, world):               # frames r, r+W, ... on this rank
        flags = z["f%%d_flags" %% f]
        d = np.where(flags[flags != -1] != 0, z["f%%d_cd" %% f], z["f%%d_l2" %% f])
        mine.add_batch(z["f%%d_idx" %% f], d.tolist(), flags)
    assert mine.counts[:, 0].sum() < z["num_count"].sum()                # really a shard
    mine.reduce()
    assert np.array_equal(mine.counts[:, 0], z["num_count"]) and np.array_equal(mine.counts[:, 1], z["success_count"])
    dist.destroy_process_group()
    print("rank", rank, "ok", mine.finalize()[0])
''')


def test_occlusion_linemod_table_allreduce_two_processes_gloo(tmp_path, golden_dir):
    """SUM of success_count[8] / num_count[8] over 2 gloo ranks reproduces the reference's single-process counts exactly"""
    script = tmp_path / "lmo_worker.py"
    script.write_text(WORKER % (ROOT, os.path.join(golden_dir, "lmo_metric_ref.npz")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)
