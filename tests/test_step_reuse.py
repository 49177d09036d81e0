"""Step reuse of the batched driver, the part that needs no GPU (include/mistra_chem.h: mistra_chem_set_step_reuse): the flag is host state — it
round-trips per mechanism before init and without a device, defaults to off, and MISTRA_CHEM_HSTART_REUSE=1 in the environment turns it on for all three
mechanisms; the entries that touch the device-side memory fail with the library's own "no HIP device" error where there is none (no CPU path).
tests/test_capi.py holds that every declared symbol is exported; tests/test_gpu_step_reuse.py holds what reuse computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MECHS, REPO


@pytest.fixture()
def chem():
    from mistra_amd.build import build_lib
    build_lib()
    from mistra_amd import chem as c
    c.lib()
    yield c
    for mech in MECHS:
        c.set_step_reuse(mech, False)


def _child(env_value):
    """get_step_reuse of the three mechanisms in a fresh process, MISTRA_CHEM_HSTART_REUSE set to env_value (None: not set)"""
    env = dict(os.environ)
    env.pop("MISTRA_CHEM_HSTART_REUSE", None)
    if env_value is not None:
        env["MISTRA_CHEM_HSTART_REUSE"] = env_value
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mistra_amd import chem\n"
            "print(' '.join(str(int(chem.get_step_reuse(m))) for m in ('gas', 'aer', 'tot')))\n" % REPO)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_flag_round_trips_per_mechanism_without_a_device(chem):
    if "MISTRA_CHEM_HSTART_REUSE" not in os.environ:
        assert [chem.get_step_reuse(m) for m in MECHS] == [False, False, False], "the default is off"
    for mech in MECHS:
        chem.set_step_reuse(mech, False)
    for mech in MECHS:
        chem.set_step_reuse(mech, True)
        assert [chem.get_step_reuse(m) for m in MECHS] == [m == mech for m in MECHS], "the flag is per mechanism"
        chem.set_step_reuse(mech, True)       # again: no change
        assert chem.get_step_reuse(mech)
        chem.set_step_reuse(mech, False)
        assert not chem.get_step_reuse(mech)
    assert chem.lib().mistra_chem_set_step_reuse(7, 1) != 0 and b"unknown mechanism" in chem.lib().mistra_chem_last_error()
    assert chem.lib().mistra_chem_get_step_reuse(7) == 0


@pytest.mark.parametrize("value,want", [("1", "1"), ("0", "0"), (None, "0")])
def test_environment_switch(value, want):
    from mistra_amd.build import build_lib
    build_lib()
    assert _child(value) == [want] * 3


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_memory_and_hstart_entries_need_a_device(chem):
    if not _no_gpu():
        pytest.skip("a GPU is present")
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.get_step_memory("gas", 150)
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.set_step_memory("gas", np.zeros(150))
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.integrate_ex("gas", np.zeros((2, 102)), np.zeros((2, 3)), np.zeros((2, 331)), hstart=np.zeros(2))
    # ... and the flag is still there to be set
    chem.set_step_reuse("tot", True)
    assert chem.get_step_reuse("tot")


@pytest.mark.parametrize("bad", [np.zeros(3), np.zeros((2, 1)), np.zeros(1)])
def test_wrong_length_hstart_raises(chem, bad):
    with pytest.raises(chem.MistraChemError, match="hstart"):
        chem.integrate_ex("gas", np.zeros((2, 102)), np.zeros((2, 3)), np.zeros((2, 331)), hstart=bad)
