"""The reaction flux of Rosenbrock_x, CPU side: the restatement with the flux sum (tests/ros_flux_py.py) against the one without,
the bounds of the GPU tests (tests/ros_flux_bounds.py), the single-step condition the GPU's exact test rests on, and the refusals the four flux
entries make before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import ros_flux_bounds as fb
import ros_flux_py as RF
import ros_methods_py as RM
from conftest import MECHS, load_golden

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_with_the_sum_equals_the_one_without(mech):
    """VAR, IERR, IPAR(11:18), Texit, Hexit bit for bit on every set used (the closing evaluation is not counted).  What the sets are there for
    holds: the Max_no_steps set ends with -6 after accepted steps and a flux that is not zero; the backward set's flux has the sign of Direction."""
    g = load_golden(mech)
    got, want = RF.restated(mech, g), RM.restated(mech, g, 0, RF.FLUX_SETS)
    for name in RF.FLUX_SETS:
        for i in range(5):
            assert np.asarray(got[name][i]).tobytes() == np.asarray(want[name][i]).tobytes(), (name, i)
        assert got[name][5].shape == (3, RF.stoich(mech).shape[1]) and np.isfinite(got[name][5]).all(), name
    m = got["m5_max_steps_5"]
    assert (m[1] == -6).all() and (m[2][:, 3] >= 1).all() and (np.abs(m[5]).max(axis=1) > 0).all()
    # each cell's largest entry (backward in time a trace species may turn negative, and its products with it); backward only where the call
    # completes, which is gas: aer and tot are unstable backward and end with -7 from a state that has left the physical range
    fw, bw = got["m4"][5], got["m4_backward"][5]
    assert (fw[np.arange(3), np.abs(fw).argmax(axis=1)] > 0).all()
    done = got["m4_backward"][1] == 1
    assert (bw[np.arange(3), np.abs(bw).argmax(axis=1)][done] < 0).all() and (done.all() if mech == "gas" else True)


@pytest.mark.parametrize("mech", MECHS)
def test_flux_balances_the_change_of_the_state(mech):
    """S * flux approximates Y(Texit) - Y(Tstart) to the trapezoid's accuracy, forward and backward: within 1e-3 of the cell's largest concentration
    on the scalar-tolerance sets (RelTol = 1e-3 bounds the step's own error; measured: 7e-15 gas .. 4e-5 aer, tests/ros_flux_bounds.py)."""
    g = load_golden(mech)
    S = RF.stoich(mech)
    cells = list(RF.cells_of(g["var_in"].shape[0]))
    for name, r in RF.restated(mech, g).items():
        if name == "m4_vector_tol":
            continue
        dy = r[0] - g["var_in"][cells]
        off = np.abs(r[5] @ S.T - dy).max(axis=1) / np.abs(r[0]).max(axis=1)
        print("%s %s: S*flux - dY = %.2e of the cell maximum" % (mech, name, off.max()))
        assert off.max() < 1.0e-3, (name, off)


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_flux_bounds.py: no re-association changes IERR or a counter on a test cell; the constant is within [10x, 100x] of the spread
    measured now, or is the floor."""
    spread, moved = fb.measure_spread(mech, load_golden(mech))
    print("%s: flux spread %.3e" % (mech, spread))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    fb.check(mech, spread)


@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_single_step_condition(mech, method):
    """AbsTol = 1e30, RelTol = 0.5, 0 -> 1e-3 s: the restatement makes exactly one attempt, accepted, to a finite state, and its flux is
    (0.5 * 1e-3) * (A(Y_0) + A(Y_1)) bit for bit."""
    from oracle.oracle import Oracle
    g = load_golden(mech)
    o = Oracle(mech)
    var, ierr, st, texit, hexit, flux = RF.restated_single(mech, g, method)
    assert (ierr == 1).all() and (st[:, 2] == 1).all() and (st[:, 3] == 1).all() and (st[:, 4] == 0).all() and np.isfinite(var).all()
    assert (texit == RF.SINGLE_TEND).all() and (hexit == 1.0e-3).all()
    from mistra_amd import mechtab
    diag = mechtab.load(mech).diag
    for i, c in enumerate(RF.cells_of(g["var_in"].shape[0])):
        plain = RM.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *RF.single_step_set(mech, method))      # the restatement without the sum
        assert plain[0].tobytes() == var[i].tobytes() and plain[1] == ierr[i] and np.array_equal(plain[2], st[i]) and plain[3:] == (texit[i], hexit[i])
        a0 = RF.products(o, g["var_in"][c], g["fix"][c], g["rconst"][c])[1]
        a1 = RF.products(o, var[i], g["fix"][c], g["rconst"][c])[1]
        assert ((0.5 * 1.0e-3) * (a0 + a1)).tobytes() == flux[i].tobytes(), c
        assert np.abs(flux[i]).max() > 0


def test_flux_units_are_built_and_checked_like_every_unit():
    """fifteen units (three mechanisms x five methods); the gas Ros3 one compiled here passes the register-ring and hazard reports the build runs on
    every unit, and holds exactly one kernel, the VARIANT 6 instantiation"""
    from mistra_amd import build as B
    assert sorted((u.mech, u.method) for u in B.VARIANT_UNITS if u.variant == 6) == [(m, k) for m in (0, 1, 2) for k in (1, 2, 3, 4, 5)]
    assert B.unit_build(B.Unit(6, 0, 2))[0] == B.UNIT_SOURCE
    assert B.unit_build(B.Unit(6, 2, 5))[2] == ["-DMISTRA_UNIT_VARIANT=6", "-DMISTRA_UNIT_MECH=2", "-DMISTRA_UNIT_METHOD=5"]
    rep = B.ring_register_report(unit=B.Unit(6, 0, 2))
    assert B.isa_hazard_report(rep["__isa_text__"]) == []
    kernels = [k for k in rep if "ros3_integrate_kernel" in k]
    assert kernels == ["_ZN6mistra21ros3_integrate_kernelINS_9GasTraitsELi64ELi6ELi2EEEvNS_10KernelArgsE"], kernels


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """A null flux, a bad ntol, an unknown mechanism and both user slots: each fails with its own text through the flux entries it applies to, with every
    data pointer NULL and no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    vector = np.array([0, 0, 0, 2] + [0] * 16, np.int32)
    out = np.zeros(4)      # never written: every call below is refused
    vp = lambda a: C.cast(_P(a), C.c_void_p)      # noqa: E731

    def entries(mid, flux, ntol=nvar, ip=ipar):
        fh, fd = (None, None) if flux is None else (_P(flux), vp(flux))
        head = (mid, 1, None, None, None, 0.0, 10.0)
        return {
            "flux_ex": lambda: L.mistra_chem_rosenbrock_flux_ex(*head, _P(tol), _P(tol), _P(rpar), _P(ip), None, None, None, None, fh),
            "flux_device": lambda: L.mistra_chem_rosenbrock_flux_device(*head, _P(tol), _P(tol), _P(rpar), _P(ip), None, None, None, None, None, None, fd),
            "flux_cells_ex": lambda: L.mistra_chem_rosenbrock_flux_cells_ex(*head, _P(tol), _P(tol), ntol, _P(rpar), _P(ip), None, None, None, None, fh),
            "flux_cells_device": lambda: L.mistra_chem_rosenbrock_flux_cells_device(*head, vp(tol), vp(tol), ntol, _P(rpar), _P(ip), None, None, None,
                                                                                    None, None, None, fd),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    refused(entries(0, None), "null flux pointer (flux: [ncell][NREACT])")
    refused(entries(9, out), "unknown mechanism id")
    refused(entries(-1, out), "unknown mechanism id")
    cells = lambda **kw: {k: v for k, v in entries(0, out, **kw).items() if "cells" in k}      # noqa: E731
    refused(cells(ntol=2), "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    refused(cells(ntol=0), "ntol = 0: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    refused(cells(ntol=1, ip=vector), "vector tolerances (ipar[1] = 0) need rows of NVAR = %d entries, ntol = 1" % nvar)
    # both user slots: the slot's existing text, whatever else the call carries (ids 3 and 4 of a library without slots are no mechanisms)
    names = chem.user_mechs()
    for i in range(2):
        if i < len(names):
            refused(entries(3 + i, out), "user mechanism slot %d (%s) has no reaction-flux entries: a user slot integrates" % (i, names[i]))
            refused(entries(3 + i, None), "and nothing else")
        else:
            refused(entries(3 + i, out), "unknown mechanism id")
    assert len(names) == 2      # the library this repository builds has both
    # the Python surface passes the refusals on, without init()
    g = load_golden("gas")
    V, F, K = g["var_in"][:2], g["fix"][:2], g["rconst"][:2]
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_flux_cells("gas", V, F, K, 0.0, 10.0, None, None, np.ones((2, 5)), np.ones((2, 5)))
    with pytest.raises(chem.MistraChemError, match="has no reaction-flux entries"):
        chem.rosenbrock_flux(3, np.zeros((1, chem.DIMS[names[0]][0])), np.zeros((1, chem.DIMS[names[0]][1])), np.zeros((1, chem.DIMS[names[0]][2])), 0.0, 10.0)


def test_tool_on_the_cpu():
    """tools/reaction_budget.py --cpu on two golden gas cells, the controlling species of their Ros3 trace: runs without a GPU and prints a table per
    species.  Nothing is asserted on the figures but that they are numbers."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    path = os.path.join(REPO, "tests", "golden", "integrate_gas.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "reaction_budget.py"), "gas", "--golden", path, "--cells", "0:2", "--cpu", "--controlling"],
                       check=True, capture_output=True, text=True, timeout=300)
    assert "CPU restatement" in r.stdout and "controlling species of the Ros3 trace" in r.stdout, r.stdout
    rows = [l.split() for l in r.stdout.split("\n") if l.strip().startswith("gross turnover")]
    assert rows and all(np.isfinite(float(x[2])) and float(x[2]) > 0 for x in rows), r.stdout


def test_flux_needs_a_device():
    """Without a GPU a well-formed call raises 'no HIP device' (there is no CPU path), through both wrappers."""
    import torch
    from mistra_amd import chem
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = load_golden("gas")
    V, F, K = g["var_in"][:1], g["fix"][:1], g["rconst"][:1]
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_flux("gas", V, F, K, 0.0, 10.0)
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_flux_cells("gas", V, F, K, 0.0, 10.0, None, None, np.full((1, 1), 1.0e-25), np.full((1, 1), 1.0e-3))
