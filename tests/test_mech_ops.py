"""The operators without a GPU (mistra_chem_jac_pattern, the refusals of mistra_chem_ops_ex / _device), the restatement on the oracle's
primitives the GPU tests compare with (tests/mech_ops_py.py) on crafted zero-pivot cases, and the reference-side measurement behind the bound on the solves
(tests/mech_ops_bounds.py).  The kernel itself is held in tests/test_gpu_mech_ops.py."""
import ctypes as C

import numpy as np
import pytest

import mech_ops_bounds as MB
import mech_ops_py as MO
from conftest import MECHS

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}


@pytest.fixture(scope="module")
def lib():
    from mistra_amd import chem
    return chem.lib()


def _err(lib):
    return lib.mistra_chem_last_error().decode()


@pytest.mark.parametrize("mech", MECHS)
def test_jac_pattern_is_the_tables(lib, mech):
    """mistra_chem_jac_pattern: LU_CROW, LU_ICOL, LU_DIAG of the mechanism's table plus 1, every diagonal slot on its own column; needs no device"""
    from mistra_amd import chem, mechtab
    t = mechtab.load(mech)
    crow, icol, diag = chem.jac_pattern(mech)
    assert crow.dtype == icol.dtype == diag.dtype == np.int32
    assert np.array_equal(crow, np.asarray(t.crow) + 1) and np.array_equal(icol, np.asarray(t.icol) + 1) and np.array_equal(diag, np.asarray(t.diag) + 1)
    assert crow.shape == (t.nvar + 1,) and icol.shape == (t.nnz,) and diag.shape == (t.nvar,)
    assert np.array_equal(icol[diag - 1], np.arange(1, t.nvar + 1))
    assert crow[0] == 1 and crow[-1] == t.nnz + 1
    # each pointer may be null
    assert lib.mistra_chem_jac_pattern(MID[mech], None, None, None) == 0


def _call(lib, device, mech=0, ncell=2, vdot=True, jvs=True, nshift=1, shift=True, fun_rhs=0, nrhs=1, rhs=True, x=True, ising=True, shift_values=None):
    nvar, nfix, nreact, nnz = (102, 3, 331, 1110)
    n = max(ncell, 1)
    a = {k: np.zeros(s) for k, s in (("var", n * nvar), ("fix", n * nfix), ("rct", n * nreact), ("vdot", n * nvar), ("jvs", n * nnz),
                                     ("rhs", max(nrhs, 1) * n * nvar), ("x", (max(nrhs, 0) + 2) * n * nvar))}
    sh = np.ones(max(nshift, 1)) if shift_values is None else np.asarray(shift_values, np.float64)
    isg = np.zeros(n, np.int32)
    p = lambda on, arr, t=_dp: arr.ctypes.data_as(t) if on else None
    if device:      # (host memory handed to the device entry: every refusal tested here comes before the pointers are looked at)
        v = lambda on, arr: C.c_void_p(arr.ctypes.data) if on else None
        return lib.mistra_chem_ops_device(mech, ncell, v(1, a["var"]), v(1, a["fix"]), v(1, a["rct"]), v(vdot, a["vdot"]), v(jvs, a["jvs"]), nshift,
                                          v(shift, sh), fun_rhs, nrhs, v(rhs, a["rhs"]), v(x, a["x"]), v(ising, isg), None)
    return lib.mistra_chem_ops_ex(mech, ncell, p(1, a["var"]), p(1, a["fix"]), p(1, a["rct"]), p(vdot, a["vdot"]), p(jvs, a["jvs"]), nshift, p(shift, sh),
                                  fun_rhs, nrhs, p(rhs, a["rhs"]), p(x, a["x"]), p(ising, isg, _ip))


REFUSALS = [
    (dict(vdot=False, jvs=False, x=False), "nothing is asked for"),
    (dict(fun_rhs=0, nrhs=0), "without a right-hand side"),
    (dict(nrhs=257), "MISTRA_OPS_MAX_RHS"),
    (dict(nrhs=2, rhs=False), "null rhs"),
    (dict(ising=False), "null ising"),
    (dict(shift=False), "null shift"),
    (dict(nshift=3, ncell=2), "nshift"),
    (dict(nshift=0), "nshift"),
]


@pytest.mark.parametrize("device", (False, True), ids=("ex", "device"))
@pytest.mark.parametrize("args,text", REFUSALS, ids=[t for _, t in REFUSALS[:-1]] + ["nshift 0"])
def test_refusals_come_before_any_device(lib, device, args, text):
    """every refusal of the header returns non-zero with its own text — not the text of a library that looked for a device and found none"""
    assert _call(lib, device, **args) != 0
    e = _err(lib)
    assert text in e and "mistra_chem_ops" in e, e
    assert "HIP" not in e and "mistra_chem_init" not in e, e


def test_nonfinite_shift_is_refused_by_the_host_form(lib):
    for bad in (np.nan, np.inf, -np.inf):
        assert _call(lib, False, nshift=2, shift_values=[1.0, bad]) != 0
        e = _err(lib)
        assert "shift[1] is not finite" in e, e


@pytest.mark.parametrize("device", (False, True), ids=("ex", "device"))
@pytest.mark.parametrize("mid", (3, 4))
def test_user_slots_have_no_operator_entries(lib, device, mid):
    for rc in (_call(lib, device, mech=mid), lib.mistra_chem_jac_pattern(mid, None, None, None)):
        assert rc != 0
        e = _err(lib)
        if lib.mistra_chem_user_mechs() > mid - 3:
            assert "user mechanism slot %d" % (mid - 3) in e and "has no operator entries" in e, e
        else:      # a library built without that slot
            assert "unknown mechanism id" in e, e


def test_python_front_refuses_without_a_device():
    """chem.ops on numpy arrays hands the library's refusal on (the arguments are checked before a device is looked for)"""
    from mistra_amd import chem
    V, F, K = (x[:2] for x in MO.column_cells("gas"))
    with pytest.raises(chem.MistraChemError, match="nothing is asked for"):
        chem.ops("gas", V, F, K, want_vdot=False, want_jvs=False)
    with pytest.raises(chem.MistraChemError, match="without a right-hand side"):
        chem.ops("gas", V, F, K, shift=1.0)
    with pytest.raises(chem.MistraChemError, match="nshift"):
        chem.ops("gas", V, F, K, shift=[1.0, 2.0, 3.0], fun_rhs=True)


# ---- the restatement
@pytest.mark.parametrize("mech", MECHS)
def test_restatement_matrix_and_zero_pivots(mech, oracles):
    """jvs -> A is (-jvs) with the shift added once on the diagonal slots (fill-in slots: -0.0, a fill-in diagonal: shift itself); ising is
    Oracle.decomp's code: 0 at the integrator's shift, i + 1 for shift = J(i,i) of a low and a high row, the first zero diagonal for shift = 0"""
    orc = oracles[mech]
    crow, icol, diag = MO.pattern(mech)
    V, F, K = (x[0] for x in MO.column_cells(mech))
    sh = 1.0 / (1.0e-3 * MO.GAMMA1)
    vdot, jvs, a, x, ising = MO.ops(orc, diag, V, F, K, sh, [V], fun_rhs=True)
    assert ising == 0 and x.shape == (2, orc.nvar) and np.isfinite(x).all()
    off = np.ones(orc.nnz, bool)
    off[diag] = False
    assert a[off].tobytes() == (-jvs[off]).tobytes() and a[diag].tobytes() == (-jvs[diag] + sh).tobytes()
    assert np.array_equal(vdot, orc.fun(V, F, K))
    for b, xr in zip((vdot, V), x):
        assert MO.backward_error(a, crow, icol, xr, b) <= MB.OMEGA_BOUND[mech]
    nz = np.flatnonzero(jvs[diag] != 0.0)
    for i in (nz[1], nz[-2]):
        _, _, a, x, ising = MO.ops(orc, diag, V, F, K, jvs[diag[i]], [V])
        assert a[diag[i]] == 0.0 and ising == 1 + min(np.flatnonzero(a[diag] == 0.0)) and ising <= i + 1
        assert x.shape == (1, orc.nvar) and x.tobytes() == np.zeros_like(x).tobytes()
    _, _, a, _, ising = MO.ops(orc, diag, V, F, K, 0.0, [V])
    zero = np.flatnonzero(a[diag] == 0.0)
    assert ising == (zero[0] + 1 if zero.size else 0)


# ---- the bound
@pytest.mark.parametrize("mech", MECHS)
def test_recorded_oracle_omega_is_not_below_the_measurement(mech):
    """the oracle's own worst backward error over the final case list and its six variants, re-measured: the recorded figure (a tenth of the kernel's
    bound) is not below it, and is not padded either"""
    got = MB.measure_oracle(mech)
    print("%s: oracle worst omega %.3e, recorded %.3e, kernel bound %.3e" % (mech, got, MB.ORACLE_OMEGA[mech], MB.OMEGA_BOUND[mech]))
    assert got <= MB.ORACLE_OMEGA[mech] <= 1.05 * got
    assert MB.OMEGA_BOUND[mech] == 10.0 * MB.ORACLE_OMEGA[mech]
    assert len(MB.cells(mech)[0]) == MB.NCELLS and len(MB.shifts()) == 4
