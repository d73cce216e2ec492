"""The attention's size queries (include/dclnet_hip.h: dcl_cross_attention_scratch_floats / _planes_bytes / _split_crops) on the
CPU: the library loads without a GPU and these three never touch the device."""
import ctypes as C

# (b, nq, nk) -> per concurrent_launches 1 and 2: (scratch_floats, planes_bytes, split_crops).  scratch_floats has no nk and
# no concurrent argument.  Derived on the CPU from the launcher's host logic; a row names a threshold of the launch plan
# (csrc/dense.hip: attn_plan): the pair window, whole rounds + rest, the badly quantised large launch, the long-key rule.
ATTENTION_SIZE_QUERIES = {
    (1, 1024, 1024): ((5308416, 0, 0), (5308416, 0, 0)),
    (6, 1024, 1024): ((15925248, 0, 0), (15925248, 0, 0)),
    (20, 1024, 1024): ((26542080, 0, 0), (26542080, 0, 0)),
    (30, 1024, 1024): (None, (79626240, 0, 0)),
    (31, 1024, 1024): ((164560896, 0, 0), (164560896, 73138176, 31)),
    (32, 1024, 1024): ((0, 0, 0), (0, 75497472, 32)),
    (40, 1024, 1024): ((26542080, 0, 0), (26542080, 75497472, 32)),
    (64, 1024, 1024): ((0, 150994944, 64), (0, 150994944, 64)),
    (80, 1024, 1024): ((106168320, 188743680, 80), (106168320, 150994944, 64)),
    (64, 1280, 96): ((106168320, 14155776, 64), (106168320, 14155776, 64)),
    (24, 2048, 12288): ((0, 679477248, 24), (0, 679477248, 24)),
    (32, 12288, 2048): ((0, 150994944, 32), (0, 150994944, 32)),
    (4, 2048, 12288): ((5308416, 0, 0), (5308416, 0, 0)),
    (64, 256, 8192): ((0, 1207959552, 64), (0, 1207959552, 64)),
    (63, 256, 8192): ((0, 0, 0), (0, 0, 0)),
    (64, 256, 8160): ((0, 0, 0), (0, 0, 0)),
    (128, 256, 64): ((0, 0, 0), (0, 18874368, 128)),
    (121, 256, 64): ((160579584, 0, 0), (160579584, 17842176, 121)),
    (120, 256, 64): (None, (79626240, 0, 0)),
    (255, 256, 64): ((0, 0, 0), (0, 18874368, 128)),
    (256, 256, 64): ((0, 37748736, 256), (0, 37748736, 256)),
    (160, 512, 256): ((106168320, 94371840, 160), (106168320, 75497472, 128)),
}


def test_attention_size_queries_answer_what_the_launch_plan_says(dcl):
    """dcl_cross_attention_scratch_floats / _planes_bytes / _split_crops never touch the device: the callers size their
    buffers by them before the call (ops.cross_attention, ops.attention_planes, Network._disengage_buffers), so their
    answers at the thresholds of the launch plan are part of the interface"""
    lib = dcl._native.lib()
    lib.dcl_cross_attention_planes_bytes.restype = C.c_int64
    for (b, nq, nk), rows in ATTENTION_SIZE_QUERIES.items():
        for conc, want in zip((1, 2), rows):
            if want is None:
                continue
            need = C.c_int64(-1)
            assert lib.dcl_cross_attention_scratch_floats(b, nq, C.byref(need)) == 0
            got = (need.value, int(lib.dcl_cross_attention_planes_bytes(b, nq, nk, conc)),
                   int(lib.dcl_cross_attention_split_crops(b, nq, nk, conc)))
            assert got == want, (b, nq, nk, conc, got, want)
