"""Which kernels one cross_attention call launches, by its size: the launch census of the diagnostic library against the launch
plan of csrc/dense.hip (attn_plan), with the results checked against float64."""
import pytest
import torch

import test_gpu_ops as TO
import test_kernel_census as TC

pytestmark = pytest.mark.gpu


_SPLIT_KERNELS = ("k_attn_split_v", "k_attn_split_k", "k_cross_attn_split")


@pytest.mark.parametrize("b,nq,nk,conc,planes,kernels,combine", [
    (2, 256, 256, 1, True, ("k_cross_attn_dma<4>",), True),                        # a small launch: 4-wave, keys split
    (128, 256, 64, 1, True, ("k_cross_attn_dma<4>",), False),                      # half a round alone
    (128, 256, 64, 2, True, _SPLIT_KERNELS, False),                                # ... one round with the other direction
    (160, 256, 128, 2, True, _SPLIT_KERNELS + ("k_cross_attn_dma<4>",), False),    # whole round of 128 + a rest of 32
    (255, 256, 64, 2, True, _SPLIT_KERNELS + ("k_cross_attn_dma<8>",), False),     # ... + a rest of 127 in the pair window, no planes
    (160, 512, 256, 1, True, _SPLIT_KERNELS, True),                                # 320 workgroups = 1.25 rounds: keys split
    (128, 512, 64, 1, False, ("k_cross_attn_dma<8>",), False),                     # a whole round without planes
    (64, 256, 8192, 1, True, _SPLIT_KERNELS, False),                               # 64 workgroups x 256 key tiles: the long-key rule
    (63, 256, 8192, 1, True, ("k_cross_attn_dma<4>",), False),                     # ... and just below it
], ids=["C1", "C2", "C3", "C4", "C5", "C6", "C7", "C8a", "C8b"])
def test_cross_attention_launches_the_kernels_its_size_calls_for(request, dcl, b, nq, nk, conc, planes, kernels, combine):
    """which kernels one ops.cross_attention call launches (launch census of the diagnostic library) at the smallest shapes on
    either side of each threshold of the launcher's plan (csrc/dense.hip: attn_plan), and the first and the last crop -- one of
    each part where a pair call is cut into whole rounds + rest -- against float64"""
    lib = TO.enter_diag(dcl, request)
    g = torch.Generator(device="cuda").manual_seed(1000 * b + nq + nk + conc)
    Q = torch.randn(b * nq, 64, device="cuda", generator=g)
    K = torch.randn(b * nk, 64, device="cuda", generator=g) * 0.3
    V1 = torch.randn(b * nk, 256, device="cuda", generator=g)
    V2 = torch.randn(b * nk, 64, device="cuda", generator=g)
    O1 = torch.full((b * nq, 256), float("nan"), device="cuda")
    O2 = torch.full((b * nq, 64), float("nan"), device="cuda")
    keep = dcl.ops.ATTENTION_SPLIT
    dcl.ops.ATTENTION_SPLIT = planes
    try:
        lib.dcl_debug_launch_census_reset()
        dcl.ops.cross_attention(b, Q, K, V1, O1, V2, O2, concurrent=conc)
        seen = TC.census(lib)
    finally:
        dcl.ops.ATTENTION_SPLIT = keep
    ran = {k for k, n in seen.items() if n > 0 and (k.startswith("k_cross_attn") or k.startswith("k_attn_split"))}
    assert ran - {"k_cross_attn_combine"} == set(kernels), sorted(ran)
    assert ("k_cross_attn_combine" in ran) == combine, sorted(ran)
    assert bool(torch.isfinite(O1).all()) and bool(torch.isfinite(O2).all())
    for i in (0, b - 1):
        q, k = Q[i * nq:(i + 1) * nq], slice(i * nk, (i + 1) * nk)
        want = TO._attn_ref(q[None], K[k][None], torch.cat([V1[k], V2[k]], 1)[None])[0]
        got = torch.cat([O1[i * nq:(i + 1) * nq], O2[i * nq:(i + 1) * nq]], 1).double()
        err = float((got - want).abs().max())
        assert err <= 2e-5 * max(1.0, float(want.abs().max())), (i, err)
