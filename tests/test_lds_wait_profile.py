"""tools/lds_wait_profile.py counts, per phase, the waits on lgkmcnt and those within eight vector instructions of the last LDS read: a
short synthetic assembly text with known answers (CPU only)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("lds_wait_profile", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lds_wait_profile.py"))
lwp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lwp)

# a header of 20 lines: f() holds STAMP(19) at line 6 and STAMP(6) at line 9, g() holds none
SRC = "\n".join(["// header", "DI void f(float* L) {", "  a();", "  b();", "  c();", "  STAMP(19);", "  d();", "  e();", "  STAMP(6);", "  h();", "}",
                 "DI void g(float* L) {", "  a();", "}", "__global__ void mocca_step_kernel(StepArgs a) {", "  f(L);", "  g(L);", "}", "", ""])


def loc(line, outer=16):
    return f"\t.loc\t1 {line} 3 ; x/mocca_device.h:{line}:3 @[ x/mocca_device.h:{outer}:3 ]"


def valu(n):
    return ["\tv_fma_f32 v1, v2, v3, v1"] * n


ASM = [loc(3), "\tds_read_b128 v[0:3], v9", *valu(2), "\ts_waitcnt lgkmcnt(0)",              # sweeps: inward: near (2)
       *valu(3), "\tds_read_b32 v4, v9 offset:8", loc(4), *valu(9), "\ts_waitcnt lgkmcnt(0)",  #                 far (9)
       "\ts_waitcnt vmcnt(0)",                                                                 # no lgkmcnt: not counted
       loc(7), "\tds_bpermute_b32 v5, v6, v7", "\ts_mov_b32 s0, s1", *valu(8), "\ts_waitcnt vmcnt(0) lgkmcnt(1)",   # base + outward: near (8; scalar not counted)
       loc(8), "\tds_write_b32 v9, v1", *valu(1), "\ts_waitcnt lgkmcnt(0)",                    # far: 9 since the last READ (a write does not restart the count)
       loc(10), "\ts_waitcnt lgkmcnt(0)",                                                      # f, behind its last STAMP: far (still 9)
       loc(13, 17), "\tds_read2_b32 v[0:1], v9 offset1:1", "\ts_waitcnt lgkmcnt(0)",           # g: near (0)
       ".Ltmp3:", "\t; comment", "\ts_endpgm"]


def test_counts_on_a_synthetic_text():
    phase_of = lwp.make_phase_of({"mocca_device.h": lwp.source_tables(SRC)})
    got = lwp.profile(ASM, phase_of)
    assert got["sweeps: inward"] == {"waits": 2, "near": 1, "lds_reads": 2}
    assert got["sweeps: base + outward"] == {"waits": 2, "near": 1, "lds_reads": 1}
    assert got["f"] == {"waits": 1, "near": 0, "lds_reads": 0}
    assert got["g"] == {"waits": 1, "near": 1, "lds_reads": 1}
    assert set(got) == {"sweeps: inward", "sweeps: base + outward", "f", "g"}


def test_a_wait_before_any_read_is_not_near():
    got = lwp.profile([loc(3), "\ts_waitcnt lgkmcnt(0)"], lambda frames: "p")
    assert got == {"p": {"waits": 1, "near": 0, "lds_reads": 0}}


def test_phase_names_follow_the_stamps():
    starts, stamps = lwp.source_tables(SRC)
    assert [n for _, n in starts] == ["f", "g", "mocca_step_kernel"] and stamps == [(6, 19), (9, 6)]
    phase_of = lwp.make_phase_of({"mocca_device.h": (starts, stamps)})
    assert phase_of([("a/mocca_device.h", 5), ("a/mocca_device.h", 16)]) == "sweeps: inward"
    assert phase_of([("a/mocca_device.h", 16)]) == "kernel body"          # the kernel's own lines
    assert phase_of([("other.h", 3), ("a/mocca_device.h", 8)]) == "sweeps: base + outward"   # a callee from another file counts for its caller
