"""The template-row scatter on the GPU (csrc/template_rows.hip: k_template_rows) against its host twin, bit for bit: the
network's five blocks, aligned widths (16 bytes per lane), widths 1 / 3 / 7 and a destination off 16-byte alignment (float by
float), one and three crops with a repeated class, 1 .. 517 template rows, cache rows 644 and 643 floats apart.  Destinations
are pre-filled with a sentinel and compared as whole buffers, so a write outside a block fails."""
import numpy as np
import pytest
import torch

import template_cases as tc

pytestmark = pytest.mark.gpu

_TWIN = {}


def twin(dcl, n_tmp, ids, name):
    """the host twin's buffers of a case, computed once and shared (read-only)"""
    key = (n_tmp, ids, name)
    if key not in _TWIN:
        got, miss = tc.run(dcl.ops.template_rows_host, n_tmp, ids, name, 644, "cpu")
        want, miss_want = tc.reference(n_tmp, ids, name)
        assert miss == miss_want and all(np.array_equal(got[k], want[k]) for k in want)
        for v in got.values():
            v.setflags(write=False)
        _TWIN[key] = (got, miss)
    return _TWIN[key]


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_kernel_equals_host_twin_bit_for_bit(dcl, case):
    b, n_tmp, name, pitch = case
    ids = tc.BATCHES[b]
    want, _ = twin(dcl, n_tmp, ids, name)
    got, miss = tc.run(dcl.ops.template_rows, n_tmp, ids, name, pitch, "cuda")
    assert miss == 0                                                             # a clean call leaves the flag alone
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    again, _ = tc.run(dcl.ops.template_rows, n_tmp, ids, name, pitch, "cuda")    # a second call: the same bits
    assert all(np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)) for k in want)


@pytest.mark.parametrize("n_tmp", [5, 517])
def test_vector_and_scalar_paths_give_the_same_bits(dcl, n_tmp):
    """the same blocks on aligned buffers with aligned cache rows (16 bytes per lane) and on buffers one float off / dense 643-
    float cache rows (float by float)"""
    ids = tc.BATCHES[3]
    vec, _ = tc.run(dcl.ops.template_rows, n_tmp, ids, "aligned_4_12", 644, "cuda")
    for name, pitch in (("base_off", 644), ("aligned_4_12", 643), ("base_off", 643)):
        got, _ = tc.run(dcl.ops.template_rows, n_tmp, ids, name, pitch, "cuda")
        assert all(np.array_equal(got[k].view(np.uint32), vec[k].view(np.uint32)) for k in vec), (name, pitch)


def test_class_ids_as_int32_on_the_device_and_int64_on_the_host(dcl):
    ids = tc.BATCHES[3]
    want, _ = twin(dcl, 64, ids, "network")
    for cls in (torch.tensor(ids, dtype=torch.int32, device="cuda"), torch.tensor(ids, dtype=torch.int64), list(ids),
                torch.tensor(ids, dtype=torch.int64, device="cuda")):
        got, miss = tc.run(dcl.ops.template_rows, 64, ids, "network", 644, "cuda", cls=cls)
        assert miss == 0 and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("name", ["network", "narrow_1_3_7"])
def test_a_miss_writes_zeros_and_raises_the_flag(dcl, name):
    """ids {5, 3, -1}: the crops with ids 3 (in the table, not cached) and -1 (outside it) are all zeros, crop 5 is exact"""
    ids = (5, 3, -1)
    want, miss_want = twin(dcl, 64, ids, name)
    got, miss = tc.run(dcl.ops.template_rows, 64, ids, name, 644, "cuda")
    assert miss == miss_want == 1
    blocks, _ = tc.BLOCK_SETS[name]
    for src_col, width, buf, dst_col in blocks:
        blk = got[buf][:, dst_col:dst_col + width].reshape(3, 64, width)
        assert not blk[1:].any() and not np.signbit(blk[1:]).any()
        assert np.array_equal(blk[0], tc.cache_rows(64)[tc.CLASS_IDS.index(5), :, src_col:src_col + width])
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    # the caller's flag: stays 0 on a clean call, is raised by a miss, and a later clean call does not lower it
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert tc.run(dcl.ops.template_rows, 5, (7, 2), name, 644, "cuda", miss=flag)[1] == 0
    assert tc.run(dcl.ops.template_rows, 5, (7, 22), name, 644, "cuda", miss=flag)[1] == 1
    assert tc.run(dcl.ops.template_rows, 5, (7, 2), name, 644, "cuda", miss=flag)[1] == 1


def test_runs_on_the_callers_stream_and_under_capture(dcl):
    """the launch is capturable (no read-back, no allocation of its own): a replay with other class ids staged deals their rows"""
    n_tmp, name = 64, "network"
    views, blocks = tc.buffers(n_tmp, 3, name, "cuda")
    cache, lut = tc.cache_tensor(n_tmp, 644, "cuda"), torch.from_numpy(tc.lut()).cuda()
    cls = torch.tensor((2, 2, 2), dtype=torch.int32, device="cuda")
    miss = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dcl.ops.template_rows(cache, lut, cls, blocks, miss)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dcl.ops.template_rows(cache, lut, cls, blocks, miss)
    cls.copy_(torch.tensor(tc.BATCHES[3], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    want, _ = twin(dcl, n_tmp, tc.BATCHES[3], name)
    assert int(miss[0]) == 0 and all(np.array_equal(views[k].cpu().numpy(), want[k]) for k in want)
