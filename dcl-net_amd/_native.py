"""ctypes loader of libdclnet_hip.so (the C ABI declared in include/dclnet_hip.h).

The header is the ONE source of the call signatures and of the constants this package shares with the library: it is parsed
once per process, and every declared entry point a library exports gets its argtypes / restype from its prototype, so the call
sites pass plain Python ints and floats.  The header therefore travels with the package.

The product path has NO CPU fallback: if the library is missing or a call fails, a RuntimeError
is raised.  PyTorch is used for device memory and streams only.
"""
import ctypes as C
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdclnet_hip.so")
DIAG_SO_PATH = os.path.join(os.path.dirname(_HERE), "tools", "_bin", "libdclnet_hip_diag.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dclnet_hip.h")
_LIB = None

vp = C.c_void_p


def build(verbose=False, diag=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libdclnet_hip.so (in-tree); diag=True also builds the diagnostic
    library (tools/_bin/libdclnet_hip_diag.so: the same sources with -DDCL_DIAG, see csrc/Makefile)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"] + (["all", "diag"] if diag else []), stdout=out)
    return SO_PATH


# ---- include/dclnet_hip.h -> signatures and constants.  The header's whole vocabulary; anything else is an error, never a guess.
_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_longlong, "uint64_t": C.c_uint64,
             "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double, "dclStream_t": vp}
_RETURNS = {"int": C.c_int, "void": None, "int64_t": C.c_int64, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "const char *": C.c_char_p}
_PROTOTYPE = re.compile(r"(.*?)\b(\w+)\s*\((.*)\)", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(DCL_\w+)[ \t]+(.*?)[ \t]*$", re.M)
_INT_LITERAL = re.compile(r"(-?(?:0[xX][0-9a-fA-F]+|\d+))|\(\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)")


def _blank(m):
    return " " + "\n" * m.group(0).count("\n")              # (line numbers survive)


def _parameter(text, line):
    if "*" in text or "[" in text:
        return vp
    words = [w for w in text.split() if w != "const"]
    for typ in (" ".join(words), " ".join(words[:-1])):     # unnamed, or followed by the parameter's name
        if typ in _BY_VALUE:
            return _BY_VALUE[typ]
    raise RuntimeError("include/dclnet_hip.h line %d: no ctypes type for the parameter `%s` (by-value types: %s)"
                       % (line, text, ", ".join(sorted(_BY_VALUE))))


def parse_header(text):
    """-> (signatures {name: (restype, [argtypes])}, constants {DCL_X: int, or the text of a non-literal #define})"""
    text = re.sub(r"/\*.*?\*/", _blank, text, flags=re.S)
    constants = {}
    for name, value in _DEFINE.findall(text):
        m = _INT_LITERAL.fullmatch(value)
        constants[name] = int(m.group(1) or m.group(2), 0) if m else value
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", _blank, text, flags=re.M)
    text = re.sub(r"\btypedef\b[^;{]*(?:\{[^}]*\}[^;]*)?;", _blank, text)
    text = re.sub(r'extern\s+"C"\s*\{', _blank, text)
    signatures, pos = {}, 0
    for stmt in text.split(";"):
        line = text.count("\n", 0, pos + len(stmt) - len(stmt.lstrip())) + 1
        pos += len(stmt) + 1
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = _PROTOTYPE.fullmatch(stmt)
        if not m:
            raise RuntimeError("include/dclnet_hip.h line %d: not a prototype this loader can read: `%s`" % (line, stmt))
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise RuntimeError("include/dclnet_hip.h line %d: no ctypes type for the return type `%s` of %s" % (line, ret, name))
        args = [] if params in ("", "void") else [_parameter(p.strip(), line) for p in params.split(",")]
        signatures[name] = (_RETURNS[ret], args)
    return signatures, constants


_HEADER = None


def _header():
    global _HEADER
    if _HEADER is None:
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError("include/dclnet_hip.h is missing (%s): the header travels with the package -- every ctypes "
                               "signature and shared constant is read from it.  There is no fallback table." % HEADER_PATH)
        with open(HEADER_PATH) as f:
            _HEADER = parse_header(f.read())
    return _HEADER


def signatures():
    """{entry point: (restype, [argtypes])} of every prototype include/dclnet_hip.h declares (the DCL_DIAG block included)"""
    return _header()[0]


def define(name):
    """the value of `#define DCL_...` in include/dclnet_hip.h; integer literals only -- anything else raises"""
    value = _header()[1].get(name)
    if not isinstance(value, int):
        raise RuntimeError("include/dclnet_hip.h: %s is %s" % (
            name, "not defined" if value is None else "`%s`, not an integer literal" % value))
    return value


ABI_VERSION = define("DCL_ABI_VERSION")     # the header this package's calls are written against


def _open(path):
    L = C.CDLL(path)
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(L, name, None)         # (the product library lacks the `#ifdef DCL_DIAG` block)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    got = int(L.dcl_abi_version())
    if got != ABI_VERSION:
        raise RuntimeError("%s speaks C-ABI version %d, this package calls version %d (include/dclnet_hip.h): rebuild the "
                           "library (make -C dcl-net_amd/csrc)" % (path, got, ABI_VERSION))
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


def query(sym, *args, what=None, ctype=C.c_int64):
    """the integer `sym` writes through its LAST parameter, an `int64_t *` -- the *_ws_bytes family.  ctype: another integer
    type, or a tuple of them for several trailing out-parameters (-> a tuple).  what: the label of a failure (default: the
    symbol without its dcl_ prefix)."""
    outs = [t(0) for t in (ctype if isinstance(ctype, tuple) else (ctype,))]
    check(getattr(lib(), sym)(*args, *[C.byref(o) for o in outs]), sym[4:] if what is None else what)
    return tuple(int(o.value) for o in outs) if isinstance(ctype, tuple) else int(outs[0].value)


def twin(sym, host, what, *args):
    """a kernel or its host twin on one argument list: <sym>_host(*args), or <sym>(*args, stream) on torch's current stream
    (a device form's workspace arguments are the caller's to append)"""
    L = lib()
    check(getattr(L, sym + "_host")(*args) if host else getattr(L, sym)(*args, stream()), what)


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
