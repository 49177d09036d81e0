"""The build's register check and the functions in which a FILLED look-ahead ring outlives compiler code (ros3_kernel.hip: gsum_run_pair
between its two programs; gsum_run_bar holds its ring across a barrier inside one statement): the ring's registers are invisible to the compiler, so these functions are sound only while every value of the compiler's stays below the
ring for the WHOLE function.  mistra_amd/build.py: ring_register_report holds them to that on the real ISA, and is shown here to refuse
crafted ISA in which a compiler value reaches the ring between a fill and its run, or in which a function it does not know fills the
ring at all.  CPU only (cross-compiles)."""
import re

import pytest

from mistra_amd import build

NEW = ("gsum_run_bar", "gsum_run_pair")


@pytest.fixture(scope="module")
def report():
    return build.ring_register_report()


def test_every_function_that_keeps_a_filled_ring_is_checked_and_below_it(report):
    assert set(NEW) <= set(build.RING_FUNCTIONS)
    for fn in NEW:
        hit = {k: v for k, v in report.items() if ("%d%sI" % (len(fn), fn)) in k}
        assert hit, "%s is not in the kernel object: %s" % (fn, sorted(k for k in report if k != "__isa_text__"))
        for k, v in hit.items():
            assert re.search(r"Lb0EEEv", k), k      # the placement, the LAST template argument (what the check reads): high — tot, aer
            assert v < min(build.RING_HIGH_SLOTS), (k, v)


# the first program's last ring turn has fetched the second program's rows; the compiler's code between the two statements sets up the
# second program's operands
PAIR = """
_ZN6mistra12_GLOBAL__N_113gsum_run_pairILi512ELi1ELb0EEEvNS_5GsDevEjijjS2_jijji:
	v_mov_b32_e32 v2, 0
	;;#ASMSTART
	global_load_dwordx4 v[192:195], v0, s[0:1] offset:0
	global_load_dwordx4 v[196:199], v0, s[0:1] offset:16
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	v_mov_b32_e32 v%d, 0x80000000
	v_lshlrev_b32_e32 v3, 5, v1
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	ds_read_b64 v[10:11], v192
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	s_setpc_b64 s[30:31]
"""


def test_a_compiler_value_in_the_ring_between_fill_and_run_is_refused(tmp_path):
    ok = tmp_path / "ok.s"
    ok.write_text(PAIR % 4)
    rep = build.ring_register_report(str(ok))
    assert max(v for k, v in rep.items() if "gsum_run_pair" in k) == 11
    bad = tmp_path / "bad.s"
    bad.write_text(PAIR % 197)      # lands in slot 1 while its load is in flight
    with pytest.raises(RuntimeError, match="v197"):
        build.ring_register_report(str(bad))


def test_a_function_the_check_does_not_know_may_not_fill_the_ring(tmp_path):
    # the same statements under a name that is not one of RING_FUNCTIONS: its registers would go unchecked
    unknown = tmp_path / "unknown.s"
    unknown.write_text((PAIR % 4).replace("13gsum_run_pairI", "14gsum_run_aheadI"))
    with pytest.raises(RuntimeError, match="not covered"):
        build.ring_register_report(str(unknown))
