"""ctypes loader of libdclnet_hip.so (the C ABI declared in include/dclnet_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails, a RuntimeError
is raised.  PyTorch is used for device memory and streams only.
"""
import ctypes as C
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdclnet_hip.so")
DIAG_SO_PATH = os.path.join(os.path.dirname(_HERE), "tools", "_bin", "libdclnet_hip_diag.so")
_LIB = None

vp = C.c_void_p


def build(verbose=False, diag=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libdclnet_hip.so (in-tree); diag=True also builds the diagnostic
    library (tools/_bin/libdclnet_hip_diag.so: the same sources with -DDCL_DIAG, see csrc/Makefile)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"] + (["all", "diag"] if diag else []), stdout=out)
    return SO_PATH


ABI_VERSION = 2                 # include/dclnet_hip.h: DCL_ABI_VERSION this package's ctypes calls are written against


def _open(path):
    L = C.CDLL(path)
    L.dcl_last_error.restype = C.c_char_p
    got = int(L.dcl_abi_version())
    if got != ABI_VERSION:
        raise RuntimeError("%s speaks C-ABI version %d, this package calls version %d (include/dclnet_hip.h): rebuild the "
                           "library (make -C dcl-net_amd/csrc)" % (path, got, ABI_VERSION))
    # csrc/linear_bwd.hip: int64 pitches between int sizes -- declared, so that a plain Python int converts correctly
    i, i64 = C.c_int, C.c_int64
    L.dcl_linear_wgrad_splits.argtypes = [i, C.POINTER(C.c_int32)]
    L.dcl_linear_wgrad.argtypes = [vp, i64, vp, i64, i, i, i, vp, vp, i64, vp]
    L.dcl_relu_bwd.argtypes = [vp, i64, vp, i64, vp, vp, i64, i, i, i, vp, i64, vp, vp, vp]
    # csrc/conv_dgrad.hip
    L.dcl_sparse_conv_dgrad.argtypes = [vp, i, vp, i, i, vp, i, i, i, vp, vp]
    L.dcl_sparse_conv_dgrad_host.argtypes = [vp, i, vp, i, i, vp, i, i, i, vp]
    # csrc/conv_fwd_compact.hip
    L.dcl_sparse_conv_fwd_compact.argtypes = [vp, i, vp, i, i, vp, i, i, i, i, vp, vp]
    L.dcl_sparse_conv_fwd_compact_host.argtypes = [vp, i, vp, i, i, vp, i, i, i, i, vp]
    # csrc/conf_pool_grad.hip: an int64 scratch size among the pointers
    L.dcl_conf_pool_cm_fwd.argtypes = [i] * 4 + [vp] * 5
    L.dcl_conf_pool_cm_fwd_host.argtypes = [i] * 4 + [vp] * 4
    L.dcl_conf_pool_cm_bwd_ws_bytes.argtypes = [i] * 4 + [C.POINTER(C.c_int64)]
    L.dcl_conf_pool_cm_bwd.argtypes = [i] * 4 + [vp] * 11 + [i64, vp]
    L.dcl_conf_pool_cm_bwd_host.argtypes = [i] * 4 + [vp] * 10
    # csrc/conf_pool_pm.hip: the channel-major set's argument lists
    L.dcl_conf_pool_pm_fwd.argtypes = [i] * 4 + [vp] * 5
    L.dcl_conf_pool_pm_fwd_host.argtypes = [i] * 4 + [vp] * 4
    L.dcl_conf_pool_pm_bwd_ws_bytes.argtypes = [i] * 4 + [C.POINTER(C.c_int64)]
    L.dcl_conf_pool_pm_bwd.argtypes = [i] * 4 + [vp] * 11 + [i64, vp]
    L.dcl_conf_pool_pm_bwd_host.argtypes = [i] * 4 + [vp] * 10
    # csrc/bn_relu.hip: int64 row counts, and eps / momentum as C floats
    f = C.c_float
    L.dcl_bn_relu_ws_bytes.argtypes = [i64, i, C.POINTER(C.c_int64)]
    L.dcl_bn_relu_fwd.argtypes = [i64, i] + [vp] * 3 + [f, f] + [vp] * 5 + [i, vp, i64, vp]
    L.dcl_bn_relu_fwd_host.argtypes = [i64, i] + [vp] * 3 + [f, f] + [vp] * 5 + [i]
    L.dcl_bn_relu_bwd.argtypes = [i64, i] + [vp] * 6 + [i] + [vp] * 3 + [vp, i64, vp]
    L.dcl_bn_relu_bwd_host.argtypes = [i64, i] + [vp] * 6 + [i] + [vp] * 3
    # csrc/linear_narrow.hip: an int64 row count and row pitch
    L.dcl_linear_narrow_fwd.argtypes = [i64, i, i, vp, i64] + [vp] * 4
    L.dcl_linear_narrow_fwd_host.argtypes = [i64, i, i, vp, i64] + [vp] * 3
    L.dcl_linear_narrow_bwd_ws_bytes.argtypes = [i64, i, i, C.POINTER(C.c_int64)]
    L.dcl_linear_narrow_bwd.argtypes = [i64, i, i, vp, i64] + [vp] * 6 + [i64, vp]
    L.dcl_linear_narrow_bwd_host.argtypes = [i64, i, i, vp, i64] + [vp] * 5
    # csrc/pose_heads_grad.hip
    L.dcl_pose_heads_train_fwd.argtypes = [i] * 6 + [vp] * 18
    L.dcl_pose_heads_train_fwd_host.argtypes = [i] * 6 + [vp] * 17
    L.dcl_pose_heads_train_bwd_ws_bytes.argtypes = [i] * 6 + [C.POINTER(C.c_int64)]
    L.dcl_pose_heads_train_bwd.argtypes = [i] * 6 + [vp] * 25 + [i64, vp]
    L.dcl_pose_heads_train_bwd_host.argtypes = [i] * 6 + [vp] * 24
    # csrc/template_rows.hip: an int64 class pitch
    L.dcl_template_rows.argtypes = [vp, i64, i, i, vp, i, vp, i, vp, i, vp, vp]
    L.dcl_template_rows_host.argtypes = [vp, i64, i, i, vp, i, vp, i, vp, i, vp]
    L.dcl_template_rows.restype = L.dcl_template_rows_host.restype = i
    # csrc/optim.hip, csrc/optim_clip_host.cpp: an int64 count and a double percentile among the pointers
    L.dcl_autoclip_observe.argtypes = [i64] + [vp] * 4 + [C.c_double, vp, vp]
    L.dcl_autoclip_observe_host.argtypes = [i64] + [vp] * 4 + [C.c_double, vp]
    L.dcl_autoclip_observe.restype = L.dcl_autoclip_observe_host.restype = i
    for fn in (L.dcl_linear_narrow_fwd, L.dcl_linear_narrow_fwd_host, L.dcl_linear_narrow_bwd_ws_bytes, L.dcl_linear_narrow_bwd,
               L.dcl_linear_narrow_bwd_host, L.dcl_pose_heads_train_fwd, L.dcl_pose_heads_train_fwd_host,
               L.dcl_pose_heads_train_bwd_ws_bytes, L.dcl_pose_heads_train_bwd, L.dcl_pose_heads_train_bwd_host):
        fn.restype = i
    for fn in (L.dcl_linear_wgrad_splits, L.dcl_linear_wgrad, L.dcl_relu_bwd, L.dcl_sparse_conv_dgrad,
               L.dcl_sparse_conv_dgrad_host, L.dcl_sparse_conv_fwd_compact, L.dcl_sparse_conv_fwd_compact_host, L.dcl_conf_pool_cm_fwd, L.dcl_conf_pool_cm_fwd_host,
               L.dcl_conf_pool_cm_bwd_ws_bytes, L.dcl_conf_pool_cm_bwd, L.dcl_conf_pool_cm_bwd_host,
               L.dcl_conf_pool_pm_fwd, L.dcl_conf_pool_pm_fwd_host, L.dcl_conf_pool_pm_bwd_ws_bytes, L.dcl_conf_pool_pm_bwd,
               L.dcl_conf_pool_pm_bwd_host, L.dcl_bn_relu_ws_bytes, L.dcl_bn_relu_fwd, L.dcl_bn_relu_fwd_host, L.dcl_bn_relu_bwd, L.dcl_bn_relu_bwd_host):
        fn.restype = i
    return L


def lib():
    """the product library.  It has no tuning hooks and reads no environment; there is no CPU fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "libdclnet_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C dcl-net_amd/csrc`.  There is no CPU fallback." % SO_PATH)
        _LIB = _open(SO_PATH)
    return _LIB


class diagnostic_library(object):
    """`with _native.diagnostic_library() as L:` -- tests/ and tools/ only.  Inside the block every op of this package
    calls into the DIAGNOSTIC build (tools/_bin/libdclnet_hip_diag.so or `path`: same sources, -DDCL_DIAG) whose
    dcl_debug_* hooks select kernel variants; the product library is restored on exit."""

    def __init__(self, path=None):
        self.path = path or DIAG_SO_PATH

    def __enter__(self):
        global _LIB
        if not os.path.exists(self.path):
            raise RuntimeError("diagnostic library missing (%s): make -C dcl-net_amd/csrc diag" % self.path)
        self.prev = _LIB
        _LIB = _open(self.path)
        return _LIB

    def __exit__(self, *exc):
        global _LIB
        _LIB = self.prev
        return False


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("libdclnet_hip %s failed (rc=%d): %s" % (what, rc, lib().dcl_last_error().decode()))


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device/host pointer of a tensor (None -> NULL)."""
    if t is None:
        return vp(0)
    return vp(t.data_ptr())


def need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dcl-net_amd: this op runs on the GPU only (got a %s tensor); no CPU fallback" % t.device)


def f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def i32c(t):
    return t.contiguous() if t.dtype == torch.int32 else t.int().contiguous()
