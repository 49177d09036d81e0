"""The integrator policy, the part that needs no GPU (include/mistra_chem.h: mistra_chem_set_policy): the checks with their texts through
mistra_chem_check_policy, mistra_chem_get_policy before any set, and the environment of a model binary that is already linked (MISTRA_CHEM_METHOD[_G|_A|_T],
MISTRA_CHEM_ATOL_REL[_G|_A|_T]), read in fresh child processes.  tests/test_capi.py holds that every declared symbol is exported;
tests/test_gpu_policy.py holds what a policy computes."""
import os
import subprocess
import sys

import pytest

from conftest import MECHS, REPO

POLICY_VARS = [stem + sfx for stem in ("MISTRA_CHEM_METHOD", "MISTRA_CHEM_ATOL_REL") for sfx in ("", "_G", "_A", "_T")]
FACTOR_TEXT = "cell_atol: factor must be finite and positive"
FLOOR_TEXT = "cell_atol: floor must be finite and positive"


@pytest.fixture(scope="module")
def chem():
    from mistra_amd.build import build_lib
    build_lib()
    from mistra_amd import chem as c
    c.lib()
    return c


def _refused(chem, text, *args, **kw):
    with pytest.raises(chem.MistraChemError) as e:
        chem.check_policy(*args, **kw)
    assert text in str(e.value), str(e.value)
    return str(e.value)


def test_bindings_are_present(chem):
    L = chem.lib()
    for name in ("set_policy", "clear_policy", "get_policy", "check_policy"):
        assert callable(getattr(chem, name))
        assert getattr(L, "mistra_chem_" + name).argtypes is not None, name


@pytest.mark.parametrize("mech", MECHS)
def test_legal_policies(chem, mech):
    for method in (1, 2, 3, 4, 5):
        chem.check_policy(mech, method)
        chem.check_policy(mech, method, 1.0e-13)
        chem.check_policy(mech, method, 0.5, 1.0e-300)
    for name in ("Ros2", "ros3", "ROS4", "Rodas3", "rodas4"):
        chem.check_policy(mech, name, 1.0e-13, 1.0e-25)
    # the floor is not read without a factor
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        chem.check_policy(mech, 4, 0.0, floor)
        chem.check_policy(mech, 4, None, floor)


@pytest.mark.parametrize("mech", MECHS)
def test_refused_methods(chem, mech):
    text = _refused(chem, "method 0 is refused", mech, 0)
    assert "Ros4" in text and "Rosenbrock_" + "gat"[MECHS.index(mech)] in text
    _refused(chem, "method 0 is refused", mech, 0, 1.0e-13)
    for method in (6, -1):
        _refused(chem, "policy: method %d is none of" % method, mech, method)
    with pytest.raises(chem.MistraChemError):
        chem.check_policy(mech, "ros5")


@pytest.mark.parametrize("mech", MECHS)
def test_refused_tolerances(chem, mech):
    for factor in (-1.0e-13, float("nan"), float("inf"), -float("inf")):
        _refused(chem, FACTOR_TEXT, mech, 2, factor, 1.0e-25)
    for floor in (0.0, -1.0e-25, float("nan"), float("inf")):
        _refused(chem, FLOOR_TEXT, mech, 2, 1.0e-13, floor)
    _refused(chem, "method 0 is refused", mech, 0, -1.0)      # the method goes first


def test_user_slot_has_ros3_only(chem):
    users = chem.user_mechs()
    assert users, "the library is built with the demo tables in its user slots"
    for slot, name in enumerate(users):
        for mech in (3 + slot, name):
            chem.check_policy(mech, 2)
            chem.check_policy(mech, 2, 1.0e-13, 1.0e-25)
            chem.check_policy(mech, "Ros3", 0.3, 1.0e-3)
            for method in (1, 3, 4, 5):
                text = _refused(chem, "user mechanism slot %d (%s) has no kernel for this Rosenbrock method" % (slot, name), mech, method, 1.0e-13)
                assert "a user slot integrates" in text
            _refused(chem, "method 0 is refused", mech, 0)
            _refused(chem, FACTOR_TEXT, mech, 2, -1.0)


def test_unknown_mechanism(chem):
    L = chem.lib()
    for mid in (-1, 5, 7):
        assert L.mistra_chem_check_policy(mid, 2, 0.0, 0.0) != 0 and b"unknown mechanism id" in L.mistra_chem_last_error()
        assert L.mistra_chem_get_policy(mid, None, None, None, None) != 0 and b"unknown mechanism id" in L.mistra_chem_last_error()
    assert L.mistra_chem_get_policy(0, None, None, None, None) != 0 and b"null pointer" in L.mistra_chem_last_error()


def _child(**policy_env):
    """get_policy of gas, aer, tot and one check_policy in a fresh process with exactly the given policy variables -> (return code, stdout lines, stderr)"""
    env = {k: v for k, v in os.environ.items() if k not in POLICY_VARS}
    env.update(policy_env)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mistra_amd import chem\n"
            "for m in ('gas', 'aer', 'tot'):\n"
            "    try:\n"
            "        print('get', m, chem.get_policy(m))\n"
            "    except chem.MistraChemError as e:\n"
            "        print('get-error', m, e)\n"
            "try:\n"
            "    chem.check_policy('gas', 2)\n"
            "    print('check ok')\n"
            "except chem.MistraChemError as e:\n"
            "    print('check-error', e)\n" % REPO)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().split("\n")


def test_no_policy_before_any_set():
    assert _child() == ["get gas None", "get aer None", "get tot None", "check ok"]


def test_environment_forms():
    P = "Policy(method=%d, atol_rel=%s, atol_floor=%s)"
    # a name in mixed case, for all three
    assert _child(MISTRA_CHEM_METHOD="RoDaS3") == ["get %s " % m + P % (4, "0.0", "0.0") for m in MECHS] + ["check ok"]
    # a number, for one mechanism
    assert _child(MISTRA_CHEM_METHOD_T="5") == ["get gas None", "get aer None", "get tot " + P % (5, "0.0", "0.0"), "check ok"]
    # factor alone: INTEGRATE_x's ATOL is the floor, the method stays Ros3
    assert _child(MISTRA_CHEM_ATOL_REL_T="1e-13") == ["get gas None", "get aer None", "get tot " + P % (2, "1e-13", "1e-25"), "check ok"]
    # factor,floor
    assert _child(MISTRA_CHEM_ATOL_REL="1e-12,1e-30") == ["get %s " % m + P % (2, "1e-12", "1e-30") for m in MECHS] + ["check ok"]
    # the per-mechanism variable goes before the global one, each part on its own
    got = _child(MISTRA_CHEM_METHOD="ros2", MISTRA_CHEM_METHOD_A="rodas4", MISTRA_CHEM_ATOL_REL="1e-12", MISTRA_CHEM_ATOL_REL_G="0.5,1e-3")
    assert got == ["get gas " + P % (1, "0.5", "0.001"), "get aer " + P % (5, "1e-12", "1e-25"), "get tot " + P % (1, "1e-12", "1e-25"), "check ok"]


@pytest.mark.parametrize("var,value", [("MISTRA_CHEM_METHOD_T", "rodas5"), ("MISTRA_CHEM_METHOD", "0"), ("MISTRA_CHEM_ATOL_REL_A", "1e-13,"),
                                       ("MISTRA_CHEM_ATOL_REL", "-1e-13"), ("MISTRA_CHEM_ATOL_REL_G", "1e-13;1e-25")])
def test_malformed_environment_fails_with_the_variables_name(var, value):
    """never a quiet run with something else: every policy entry reports the variable (mistra_chem_init does too: tests/test_gpu_policy.py)"""
    got = _child(**{var: value})
    assert len(got) == 4
    for line in got[:3]:
        assert line.startswith("get-error") and var + "=" + value in line, line
    assert got[3].startswith("check-error") and var + "=" + value in got[3]
