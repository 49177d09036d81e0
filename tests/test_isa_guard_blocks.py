"""Check (iii) of the build's ISA guard (mistra_amd/build.py: isa_hazard_report) per asm block: a counted vmcnt wait is held to the
ring its own statement streams, not to the union of every ring the function holds.  An integrating kernel inlines executors of
several ring depths; a wait too deep for a 4-slot ring passed as long as an 8-slot ring sat elsewhere in the same function."""
from mistra_amd import build

TWO_RINGS = """
_ZN6mistra9two_ringsEv:
	;;#ASMSTART
	global_load_dwordx4 v[192:195], v0, s[0:1] offset:0
	global_load_dwordx4 v[196:199], v0, s[0:1] offset:1024
	global_load_dwordx4 v[208:211], v0, s[0:1] offset:2048
	global_load_dwordx4 v[212:215], v0, s[0:1] offset:3072
	;;#ASMEND
	;;#ASMSTART
	global_load_dwordx4 v[224:227], v0, s[2:3] offset:0
	global_load_dwordx4 v[228:231], v0, s[2:3] offset:1024
	global_load_dwordx4 v[240:243], v0, s[2:3] offset:2048
	global_load_dwordx4 v[244:247], v0, s[2:3] offset:3072
	;;#ASMEND
	;;#ASMSTART
	s_waitcnt vmcnt(4)
	ds_read_b64 v[2:3], v192
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	;;#ASMSTART
	global_load_dwordx4 v[48:55], v1, s[4:5]
	global_load_dwordx4 v[64:71], v1, s[4:5] offset:2048
	global_load_dwordx4 v[80:87], v1, s[4:5] offset:4096
	global_load_dwordx4 v[96:103], v1, s[4:5] offset:6144
	s_waitcnt vmcnt(%d)
	;;#ASMEND
	s_setpc_b64 s[30:31]
"""


def test_a_wait_too_deep_for_its_own_ring_is_caught_beside_a_deeper_one():
    # the function's asm loads fill 12 distinct slots; the executor block streams 4 of its own: vmcnt(5) cannot cover that ring
    hits = build.isa_hazard_report(TWO_RINGS % 5)
    assert len(hits) == 1 and "two_rings" in hits[0] and "vmcnt(5)" in hits[0] and "its asm block" in hits[0], hits


def test_waits_within_their_rings_pass():
    # vmcnt(3) in the 4-slot executor; vmcnt(4) in a statement that only consumes the 8-slot ring loaded by separate statements
    assert build.isa_hazard_report(TWO_RINGS % 3) == []


def test_a_consuming_statement_is_held_to_the_function_ring():
    deep = (TWO_RINGS % 3).replace("s_waitcnt vmcnt(4)", "s_waitcnt vmcnt(12)")
    hits = build.isa_hazard_report(deep)
    assert len(hits) == 1 and "vmcnt(12)" in hits[0] and "the function's asm loads" in hits[0], hits


LOW_TAIL = """
_ZN6mistra12_GLOBAL__N_110tail_solveILi1ELi0ELb1EEEvNS_7TailDevEjji:
	v_mov_b32_e32 v2, 0
	;;#ASMSTART
	global_load_dwordx4 v[64:67], v0, s[0:1] offset:0
	;;#ASMEND
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	ds_read_b64 v[%d:%d], v64
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	s_setpc_b64 s[30:31]
"""


def test_the_ring_check_sees_registers_the_compiler_chose_for_asm_results(tmp_path):
    # a gather's destination is named only inside asm: below the low ring it passes, inside it the build refuses to link
    ok = tmp_path / "ok.s"
    ok.write_text(LOW_TAIL % (20, 21))
    rep = build.ring_register_report(str(ok))
    assert max(v for k, v in rep.items() if "tail_solve" in k) == 21
    bad = tmp_path / "bad.s"
    bad.write_text(LOW_TAIL % (70, 71))
    try:
        build.ring_register_report(str(bad))
    except RuntimeError as e:
        assert "v71" in str(e)
    else:
        raise AssertionError("an asm result inside the ring passed the check")
