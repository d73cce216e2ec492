"""dcl-net_amd/_native.py derives every ctypes signature and every shared constant from include/dclnet_hip.h: the parsed
prototypes cover the header's whole surface, both libraries carry them, the type mapping is what a literal list written here
by hand says, and what the parser cannot map is an error.  No GPU, no compute call."""
import ctypes as C
import os
import re

import pytest

from test_abi import ROOT, declared_symbols

i, i32, i64, ll, ull, u64, f, d, vp = (C.c_int, C.c_int32, C.c_int64, C.c_longlong, C.c_ulonglong, C.c_uint64, C.c_float,
                                       C.c_double, C.c_void_p)

# written out from the header by hand, NOT with the parser: (restype, argtypes) -- every type of the header's vocabulary occurs
WANT = {
    "dcl_last_error": (C.c_char_p, []),
    "dcl_abi_version": (i, []),
    "dcl_linear_split_weight_bytes": (i64, [i, i]),
    "dcl_linear_fwd": (i, [vp, i64, vp, i64, vp, vp, i64, i, i, i, i, vp, i64, vp]),
    "dcl_adam_step": (i, [i, vp, i, vp, vp, f, f, f, f, vp]),
    "dcl_autoclip_observe": (i, [i64, vp, vp, vp, vp, d, vp, vp]),
    "dcl_autoclip_observe_host": (i, [i64, vp, vp, vp, vp, d, vp]),
    "dcl_crop_draw": (i, [i, i, vp, i, i, u64, u64, vp, vp, vp]),
    "dcl_pose_heads": (i, [i, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dcl_pad_copy_many": (i, [vp, i, vp]),
    "dcl_template_rows": (i, [vp, i64, i, i, vp, i, vp, i, vp, i, vp, vp]),
    "dcl_backbone_caps": (i, [i, i, i, vp]),
    "dcl_profile_conv_end_calls": (i, [vp, vp, vp, vp, i32]),
    "dcl_debug_launch_census_reset": (None, []),
    "dcl_debug_force_valu_conv": (None, [i]),
    "dcl_debug_linear_plan_workspace": (ll, [i, i, i]),
    "dcl_debug_launch_census": (ll, [vp, ll]),
    "dcl_debug_nn_tests_executed": (ull, [i]),
    "dcl_debug_stamp": (i, [vp, vp]),
}

# the constants of dcl.ops (and _native.ABI_VERSION) the header backs: name -> the expression of #defines it equals
BACKED = {"TEMPLATE_MAX_BLOCKS": "DCL_TEMPLATE_MAX_BLOCKS", "POOL_PM_ROWS": "DCL_POOL_PM_ROWS", "NARROW_MAX_N": "DCL_NARROW_MAX_N",
          "NARROW_ROWS": "DCL_NARROW_ROWS", "BN_ROWS": "DCL_BN_ROWS", "OPTIM_CHUNK": "DCL_OPTIM_CHUNK",
          "CONV_PAIRS_SPLIT": "DCL_CONV_PAIRS_SPLIT", "CONV_PAIRS_HEAD": "DCL_CONV_PAIRS_HEAD", "WGRAD_ROWS": "DCL_WGRAD_ROWS",
          "CROP_DRAW_MAX_POINTS": "DCL_CROP_DRAW_MAX_POINTS", "LINEAR_GROUP_MAX": "DCL_LINEAR_MAX_JOBS",
          "POSE_ROW_BYTES": "DCL_CROP_POSE_ROW_BYTES", "POSE_ROW64_BYTES": "DCL_CROP_POSE_ROW64_BYTES",
          "PASTE_PLAN_INTS": "DCL_PASTE_PLAN_INTS"}


def header_define(name):
    """the integer an `#define name <digits>` line of the header gives, read with this test's own regex"""
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    found = re.findall(r"^#define\s+%s\s+(\d+)\b" % re.escape(name), text, flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_every_declared_symbol_has_a_parsed_prototype_and_the_reverse(dcl):
    assert set(dcl._native.signatures()) == set(declared_symbols(diag=True))


def test_both_libraries_carry_argtypes_on_every_declared_symbol_they_export(dcl):
    N = dcl._native
    sigs = N.signatures()
    product = N.lib()
    with N.diagnostic_library() as diag:
        for L, names in ((product, declared_symbols()), (diag, declared_symbols(diag=True))):
            for name in names:
                fn = getattr(L, name)                                  # (test_abi: every one of them is exported)
                assert fn.argtypes is not None, name
                assert (fn.restype, list(fn.argtypes)) == (sigs[name][0], sigs[name][1]), name
        assert not any(hasattr(product, s) for s in sigs if s.startswith("dcl_debug"))


def test_the_type_mapping_is_the_one_written_out_here(dcl):
    sigs = dcl._native.signatures()
    used = set()
    for name, (restype, argtypes) in WANT.items():
        assert (sigs[name][0], list(sigs[name][1])) == (restype, argtypes), name
        used.update([restype] + argtypes)
    assert used >= {None, C.c_char_p, i, i32, i64, ll, ull, u64, f, d, vp}, "WANT must cover the vocabulary"
    L = dcl._native.lib()
    assert L.dcl_last_error.restype is C.c_char_p and list(L.dcl_adam_step.argtypes) == WANT["dcl_adam_step"][1]


def test_the_parser_maps_arrays_and_names_to_the_same_types(dcl):
    sigs, consts = dcl._native.parse_header(
        "/* c */\n#define DCL_A 7\n#define DCL_B (-3)\n#define DCL_C 0x10 /* hex */\n#define DCL_D (DCL_A + 1)\n"
        "typedef struct { int a; float *b; } DclThing;\n"
        "int dcl_x(const DclThing *t, const int32_t counts_host[8], unsigned long long, int64_t n /* rows */, dclStream_t stream);\n"
        "#ifdef DCL_DIAG\nvoid dcl_y(void);\n#endif\n")
    assert sigs == {"dcl_x": (i, [vp, vp, ull, i64, vp]), "dcl_y": (None, [])}
    assert (consts["DCL_A"], consts["DCL_B"], consts["DCL_C"]) == (7, -3, 16) and not isinstance(consts["DCL_D"], int)


@pytest.mark.parametrize("text, names", [
    ("int dcl_ok(int a);\n\nint dcl_bad(size_t n, int b);\n", ("line 3", "size_t n")),                    # an unknown type
    ("typedef struct { int a; } DclJob;\nint dcl_bad(DclJob job, int n);\n", ("line 2", "DclJob job")),    # a by-value struct
    ("int dcl_ok(int a);\nDclJob dcl_bad(int n);\n", ("line 2", "DclJob")),                                # ... returned
    ("int dcl_ok(int a);\nint dcl_table[4];\n", ("line 2", "dcl_table")),                                  # not a prototype
])
def test_the_parser_raises_on_what_it_cannot_map_and_names_the_line(dcl, text, names):
    with pytest.raises(RuntimeError) as e:
        dcl._native.parse_header(text)
    for part in names:
        assert part in str(e.value), str(e.value)


def test_header_backed_constants_equal_their_defines(dcl):
    for name, define in BACKED.items():
        assert getattr(dcl.ops, name) == header_define(define) == dcl._native.define(define), name
    assert dcl.ops.AUTOCLIP_OUT_DOUBLES * 8 == header_define("DCL_AUTOCLIP_OUT_BYTES")
    assert dcl.ops.AUTOCLIP_SCALE_F32_INDEX * 4 == header_define("DCL_AUTOCLIP_SCALE_F32_OFFSET")
    assert dcl.ops.TABLE_MODES == {"adds": header_define("DCL_TABLE_ADDS"), "lm": header_define("DCL_TABLE_LM"),
                                   "lmo": header_define("DCL_TABLE_LMO")}
    assert dcl._native.ABI_VERSION == header_define("DCL_ABI_VERSION") == dcl._native.lib().dcl_abi_version()
    assert dcl._native.define("DCL_EINVAL") == -1


def test_a_define_that_is_no_integer_literal_is_not_offered(dcl):
    for name in ("DCL_AUTOCLIP_MAX_N", "DCL_NO_SUCH_DEFINE"):
        with pytest.raises(RuntimeError, match=name):
            dcl._native.define(name)


def test_a_missing_or_mistyped_argument_is_a_type_error(dcl):
    L = dcl._native.lib()
    n = C.c_int64(0)
    assert L.dcl_backbone_ws_bytes(2, 64, 1000, C.byref(n)) == 0 and n.value > 0
    with pytest.raises(TypeError):
        L.dcl_backbone_ws_bytes(2, 64, C.byref(n))                     # one argument too few
    with pytest.raises(C.ArgumentError):
        L.dcl_backbone_ws_bytes(2, 64, 1000.0, C.byref(n))             # a float for an int
    assert dcl._native.query("dcl_backbone_ws_bytes", 2, 64, 1000) == n.value
