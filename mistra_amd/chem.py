"""Host-side mirror of the reference's integrator interface over the C ABI (include/mistra_chem.h).

The reference exposes, per mechanism x in {g, a, t}, `SUBROUTINE INTEGRATE_x(TIN, TOUT)` working on
`COMMON /GDATA_x/ C(NSPEC), RCONST(NREACT), ...` (gas.f:710, gas_Global.h:29-58 | aer.f:1408 | tot.f:2812).
Here the same call takes the arrays explicitly and handles any number of cells:

    integrate("tot", var, fix, rconst, tin=0.0, tout=10.0) -> IntegrateResult(var, ierr, stats)

`var`, `fix`, `rconst` are cell-major arrays [ncell, NVAR|NFIX|NREACT]: numpy arrays go through the host-buffer
entry point, torch CUDA tensors stay on the device (`mistra_chem_integrate_device`, asynchronous on the current
torch stream).  There is no CPU implementation in this package: without the HIP library and a GPU the calls raise.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from .mechtab import MECH_IDS, MECH_NAMES

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MISTRA_CHEM_LIB", os.path.join(_PKG, "lib", "libmistra_chem.so"))   # override: diagnostic builds

USER_IDS = {"user0": 3, "user1": 4}      # the user mechanism slots (include/mistra_chem.h: MISTRA_MECH_USER0, _USER1)


class _Dims(dict):
    """(NVAR, NFIX, NREACT, LU_NONZERO) by mechanism name; the sizes of a user slot's table are asked of the library the first time."""

    def __missing__(self, name):
        mid, name = _mech_id(name)
        n = [C.c_int32(0) for _ in range(4)]
        _check(lib().mistra_chem_dims(mid, *(C.byref(x) for x in n)))
        self[name] = tuple(x.value for x in n)
        return self[name]


DIMS = _Dims({"gas": (102, 3, 331, 1110), "aer": (257, 5, 979, 6579), "tot": (417, 7, 1627, 13503)})
STAT_NAMES = ("Nfun", "Njac", "Nstp", "Nacc", "Nrej", "Ndec", "Nsol", "Nsng")   # COMMON /Statistics/, gas.f:913
IERR_TEXT = {1: "success", -6: "too many steps", -7: "step size too small", -8: "matrix repeatedly singular"}

IntegrateResult = namedtuple("IntegrateResult", "var ierr stats")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None
_inited_device = None


class MistraChemError(RuntimeError):
    pass


def lib():
    """The C-ABI library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MistraChemError("HIP library %s is missing: run `python -m mistra_amd.build` (or __graft_entry__.build())"
                                  % LIB_PATH)
        try:
            # PyTorch ships its own libamdhip64 / libhsa-runtime64.  Loaded first, the library below binds to those by soname and the
            # process has ONE HIP runtime; loaded after this library (which then has pulled in /opt/rocm's), the process has two,
            # and the one that initialises second sees no device (found with __graft_entry__.build() followed by smoke()).
            import torch  # noqa: F401
        except ImportError:      # a caller without PyTorch (numpy buffers only): the system runtime alone
            pass
        L = C.CDLL(LIB_PATH)
        L.mistra_chem_init.argtypes = [C.c_int]
        L.mistra_chem_init_devices.argtypes = [C.c_int, _ip]
        L.mistra_chem_integrate_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _ip, _ip, _dp]
        L.mistra_chem_integrate_env_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _ip, _ip, _dp]
        L.mistra_chem_integrate_common_status.argtypes = [C.c_int, C.c_void_p, _dp, _dp, _ip, _dp, _dp, _ip]
        L.mistra_chem_finalize.restype = None
        L.mistra_chem_dims.argtypes = [C.c_int, _ip, _ip, _ip, _ip]
        L.mistra_chem_integrate.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _ip, _ip]
        L.mistra_chem_integrate_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                                   C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mistra_chem_integrate_device_hstart.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                                          C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p]
        L.mistra_chem_rates_env_size.argtypes = [C.c_int]
        L.mistra_chem_update_rconst.argtypes = [C.c_int, C.c_int, _dp, _dp]
        L.mistra_chem_update_rconst_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mistra_chem_integrate_common.argtypes = [C.c_int, C.c_void_p, _dp, _dp]
        L.mistra_chem_singular_rows.argtypes = [C.c_int, C.c_int, _ip]
        vp = C.c_void_p
        L.mistra_chem_set_species_maps.argtypes = [C.c_int, C.c_int, _ip, _ip, C.c_int, _ip, _ip]
        L.mistra_chem_drive_dims.argtypes = [C.c_int, _ip, _ip, _ip, _ip]
        L.mistra_chem_pack_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mistra_chem_unpack_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mistra_chem_budgets_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, vp, vp, vp]
        L.mistra_chem_rates_env_from_c_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp]
        L.mistra_chem_fast_k_mt_device.argtypes = [C.c_int, C.c_int, vp, vp, _ip, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mistra_chem_henry_device.argtypes = [C.c_int, C.c_int, vp, vp, vp]
        L.mistra_chem_equil_co_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "mistra_chem_v_mean_device"):      # (see below: older builds in same-box A/B runs)
            L.mistra_chem_v_mean_device.argtypes = [C.c_int, C.c_int, vp, vp, vp]
        if hasattr(L, "mistra_chem_st_coeff_device"):
            L.mistra_chem_st_coeff_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        L.mistra_chem_drive_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "mistra_chem_drive"):      # (an older build of the library loaded for a same-box A/B, tools/ab_many.sh, does not have these)
            L.mistra_chem_drive.argtypes = [C.c_int, C.c_int, _ip, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _ip, _ip, _dp, _dp, C.c_int,
                                            _ip, _dp, _dp]
            L.mistra_chem_debug_set_max_steps.argtypes = [C.c_int]
        if hasattr(L, "mistra_chem_drive_begin"):
            L.mistra_chem_drive_begin.argtypes = L.mistra_chem_drive.argtypes
            L.mistra_chem_drive_end.argtypes = [C.c_int]
        if hasattr(L, "mistra_chem_set_options"):
            L.mistra_chem_check_options.argtypes = [C.c_int, _ip, _dp, _dp, _dp, C.c_double, _ip, _dp, _ip]
            L.mistra_chem_set_options.argtypes = [C.c_int, _ip, _dp, _dp, _dp, _ip]
            L.mistra_chem_get_options.argtypes = [C.c_int, _ip, _ip, _dp, _dp, _dp]
        if hasattr(L, "mistra_chem_set_step_reuse"):
            L.mistra_chem_set_step_reuse.argtypes = [C.c_int, C.c_int]
            L.mistra_chem_get_step_reuse.argtypes = [C.c_int]
            L.mistra_chem_get_step_memory.argtypes = [C.c_int, C.c_int, _dp]
            L.mistra_chem_set_step_memory.argtypes = [C.c_int, C.c_int, _dp]
            L.mistra_chem_integrate_hstart_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _ip, _ip, _dp, _dp]
        if hasattr(L, "mistra_chem_rosenbrock_ex"):
            L.mistra_chem_rosenbrock_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip, _dp, _ip, _ip, _dp]
            L.mistra_chem_rosenbrock_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, _dp, _dp, _dp, _ip, vp, vp, vp, vp, vp, vp]
            L.mistra_chem_method_table.argtypes = [C.c_int, C.POINTER(C.c_int), _dp, _dp, _dp, _dp, _dp, _ip, _dp]
            L.mistra_chem_rosenbrock_trace_ex.argtypes = L.mistra_chem_rosenbrock_ex.argtypes + [C.c_int, _dp, _ip, _ip, _ip]
            L.mistra_chem_rosenbrock_trace_device.argtypes = L.mistra_chem_rosenbrock_device.argtypes + [C.c_int, vp, vp, vp, vp]
            L.mistra_chem_rosenbrock_cells_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, C.c_int, _dp, _ip, _dp, _ip,
                                                          _ip, _dp]
            L.mistra_chem_rosenbrock_cells_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, vp, vp, C.c_int, _dp, _ip, vp, vp, vp,
                                                              vp, vp, vp]
            L.mistra_chem_rosenbrock_trace_cells_ex.argtypes = L.mistra_chem_rosenbrock_cells_ex.argtypes + [C.c_int, _dp, _ip, _ip, _ip]
            L.mistra_chem_rosenbrock_trace_cells_device.argtypes = L.mistra_chem_rosenbrock_cells_device.argtypes + [C.c_int, vp, vp, vp, vp]
            L.mistra_chem_cell_atol_device.argtypes = [C.c_int, C.c_int, vp, C.c_double, C.c_double, vp, vp]
        if hasattr(L, "mistra_chem_rosenbrock_series_ex"):
            L.mistra_chem_rosenbrock_series_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip, C.c_int, _dp, _dp, _ip, _ip, _dp]
            L.mistra_chem_rosenbrock_series_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, _dp, _dp, _dp, _dp, _ip, vp, vp, vp, vp, C.c_int, vp, vp]
            L.mistra_chem_rosenbrock_series_cells_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _ip, C.c_int, _dp,
                                                                 _dp, _ip, _ip, _dp]
            L.mistra_chem_rosenbrock_series_cells_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, _dp, vp, vp, C.c_int, _dp, _ip, vp, vp, vp, vp,
                                                                     C.c_int, vp, vp]
        if hasattr(L, "mistra_chem_rosenbrock_series_rates_ex"):      # the series entries' lists with rconst_legs, fix_legs behind rconst
            for form in ("ex", "device", "cells_ex", "cells_device"):
                at = getattr(L, "mistra_chem_rosenbrock_series_" + form).argtypes
                getattr(L, "mistra_chem_rosenbrock_series_rates_" + form).argtypes = at[:5] + [C.c_int, C.c_int] + at[5:]
                if hasattr(L, "mistra_chem_rosenbrock_series_linrates_" + form):      # ... with fix_legs behind rconst_nodes
                    getattr(L, "mistra_chem_rosenbrock_series_linrates_" + form).argtypes = at[:5] + [C.c_int] + at[5:]
                if hasattr(L, "mistra_chem_rosenbrock_series_flux_" + form):          # ... the series with rates' list with flux_series behind it
                    getattr(L, "mistra_chem_rosenbrock_series_flux_" + form).argtypes = at[:5] + [C.c_int, C.c_int] + at[5:] + [vp if "device" in form else _dp]
        if hasattr(L, "mistra_chem_rosenbrock_flux_ex"):
            L.mistra_chem_rosenbrock_flux_ex.argtypes = L.mistra_chem_rosenbrock_ex.argtypes + [_dp]
            L.mistra_chem_rosenbrock_flux_device.argtypes = L.mistra_chem_rosenbrock_device.argtypes + [vp]
            L.mistra_chem_rosenbrock_flux_cells_ex.argtypes = L.mistra_chem_rosenbrock_cells_ex.argtypes + [_dp]
            L.mistra_chem_rosenbrock_flux_cells_device.argtypes = L.mistra_chem_rosenbrock_cells_device.argtypes + [vp]
        if hasattr(L, "mistra_chem_rosenbrock_dense_ex"):
            L.mistra_chem_rosenbrock_dense_ex.argtypes = L.mistra_chem_rosenbrock_ex.argtypes + [C.c_int, _dp, _dp, _ip]
            L.mistra_chem_rosenbrock_dense_device.argtypes = L.mistra_chem_rosenbrock_device.argtypes + [C.c_int, _dp, vp, vp]
            L.mistra_chem_rosenbrock_dense_cells_ex.argtypes = L.mistra_chem_rosenbrock_cells_ex.argtypes + [C.c_int, _dp, _dp, _ip]
            L.mistra_chem_rosenbrock_dense_cells_device.argtypes = L.mistra_chem_rosenbrock_cells_device.argtypes + [C.c_int, _dp, vp, vp]
        if hasattr(L, "mistra_chem_ops_ex"):
            L.mistra_chem_jac_pattern.argtypes = [C.c_int, _ip, _ip, _ip]
            L.mistra_chem_ops_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip]
            L.mistra_chem_ops_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]
        if hasattr(L, "mistra_chem_rosenbrock_replay_ex"):      # (hsteps, nsteps as addresses: host arrays, or device arrays for the device entries' rows per cell)
            table = [C.c_int, C.c_int, vp, vp]
            L.mistra_chem_rosenbrock_replay_ex.argtypes = L.mistra_chem_rosenbrock_ex.argtypes[:11] + table + [_dp, _ip, _ip, _dp, _dp]
            L.mistra_chem_rosenbrock_replay_cells_ex.argtypes = L.mistra_chem_rosenbrock_cells_ex.argtypes[:12] + table + [_dp, _ip, _ip, _dp, _dp]
            L.mistra_chem_rosenbrock_replay_device.argtypes = L.mistra_chem_rosenbrock_device.argtypes[:11] + table + [vp, vp, vp, vp, vp, vp]
            L.mistra_chem_rosenbrock_replay_cells_device.argtypes = L.mistra_chem_rosenbrock_cells_device.argtypes[:12] + table + [vp, vp, vp, vp, vp, vp]
        if hasattr(L, "mistra_chem_set_policy"):
            L.mistra_chem_set_policy.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
            L.mistra_chem_check_policy.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
            L.mistra_chem_clear_policy.argtypes = [C.c_int]
            L.mistra_chem_get_policy.argtypes = [C.c_int, _ip, _ip, _dp, _dp]
        if hasattr(L, "mistra_chem_user_mechs"):
            L.mistra_chem_mech_name.restype = C.c_char_p
            L.mistra_chem_mech_name.argtypes = [C.c_int]
        L.mistra_chem_last_error.restype = C.c_char_p
        L.mistra_chem_describe.restype = C.c_char_p
        L.mistra_chem_describe.argtypes = [C.c_int]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MistraChemError(lib().mistra_chem_last_error().decode())


def init(device=0):
    """Select the GPU, load mechanism tables and upload the kernel schedules (idempotent per device).  A device that
    init_devices() already set up is left as it is."""
    global _inited_device
    if _inited_device is not None and (device == _inited_device or (isinstance(_inited_device, tuple) and device in _inited_device)):
        return
    _check(lib().mistra_chem_init(int(device)))
    _inited_device = device


def init_devices(devices):
    """Several GPUs in one process (mistra_chem_init_devices): `devices` = a count or a list of HIP device indices.  Host-buffer
    calls are then split into one block of cells per device; device-buffer calls run where their tensors live."""
    global _inited_device
    ids = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
    arr = (C.c_int32 * len(ids))(*ids)
    _check(lib().mistra_chem_init_devices(len(ids), arr))
    _inited_device = tuple(ids)


def finalize():
    global _inited_device
    if _lib is not None:
        _lib.mistra_chem_finalize()
    _inited_device = None


def describe(mech):
    return lib().mistra_chem_describe(_mech_id(mech)[0]).decode()


def user_mechs():
    """The names of the user mechanism slots this library was built with (mistra_chem_user_mechs, mistra_chem_mech_name): ids 3 and 4."""
    L = lib()
    if not hasattr(L, "mistra_chem_user_mechs"):      # (an older build loaded for a same-box A/B)
        return []
    return [L.mistra_chem_mech_name(3 + i).decode() for i in range(L.mistra_chem_user_mechs())]


def _mech_id(mech):
    """-> (mechanism id, name).  "gas" | "aer" | "tot" | 0..2, and for a user slot its table's name, "user0" / "user1", or 3 / 4."""
    if isinstance(mech, str):
        if mech in MECH_IDS:
            return MECH_IDS[mech], mech
        users = user_mechs()
        if mech in USER_IDS and USER_IDS[mech] - 3 < len(users):
            return USER_IDS[mech], users[USER_IDS[mech] - 3]
        if mech in users:
            return 3 + users.index(mech), mech
        raise MistraChemError("unknown mechanism %r (this library has gas, aer, tot%s)" % (mech, "".join(", " + u for u in users)))
    mid = int(mech)
    if mid < len(MECH_NAMES):
        return mid, MECH_NAMES[mid]
    users = user_mechs()
    if mid - 3 < len(users):
        return mid, users[mid - 3]
    raise MistraChemError("unknown mechanism id %d" % mid)


def integrate(mech, var, fix, rconst, tin=0.0, tout=10.0, device=None):
    """INTEGRATE_x over a batch of cells.  numpy in -> numpy out (synchronous); torch CUDA tensors in -> torch
    tensors out on the same device, enqueued on the current torch stream."""
    mid, name = _mech_id(mech)
    nvar, nfix, nreact, _ = DIMS[name]
    try:
        import torch
        is_torch = isinstance(var, torch.Tensor)
    except ImportError:      # pragma: no cover
        is_torch = False
    if is_torch:
        return _integrate_torch(mid, name, var, fix, rconst, tin, tout)
    if device is not None or _inited_device is None:      # host data: whatever device(s) the library already runs on
        init(0 if device is None else device)
    v = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
    ncell = v.shape[0]
    f = np.ascontiguousarray(fix, np.float64).reshape(ncell, nfix)
    r = np.ascontiguousarray(rconst, np.float64).reshape(ncell, nreact)
    out = np.empty_like(v)
    ierr = np.zeros(ncell, np.int32)
    stats = np.zeros((ncell, 8), np.int32)
    _check(lib().mistra_chem_integrate(mid, ncell, v.ctypes.data_as(_dp), f.ctypes.data_as(_dp), r.ctypes.data_as(_dp),
                                      float(tin), float(tout), out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip),
                                      stats.ctypes.data_as(_ip)))
    return IntegrateResult(out, ierr, stats)


def integrate_ex(mech, var, fix, rconst, tin=0.0, tout=10.0, env=None, hstart=None):
    """mistra_chem_integrate_ex on host buffers: what `integrate` returns plus t_h [ncell, 3] — per cell the exit time (-> TIN,
    gas.f:769), the last accepted step (-> STEPMIN, gas.f:770) and H when the integrator returned.  This is the call the batched
    Fortran surface makes (shim/mistra_kpp_shim.f90: INTEGRATE_BATCH_x); with several devices initialised (init_devices) the
    library cuts the batch into one block per device.  hstart [ncell]: OPT-IN first step size per cell, e.g. t_h[:, 1] of the previous
    call (mistra_chem_integrate_hstart_ex; entries <= 0: the reference's value)."""
    mid, name = _mech_id(mech)
    nvar, nfix, nreact, _ = DIMS[name]
    v = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
    ncell = v.shape[0]
    if hstart is not None:
        hs = np.ascontiguousarray(hstart, np.float64)
        if hs.shape != (ncell,):
            raise MistraChemError("hstart: %d entries expected, one per cell" % ncell)
    if _inited_device is None:
        init(0)
    f = np.ascontiguousarray(fix, np.float64).reshape(ncell, nfix)
    if env is not None:      # mistra_chem_integrate_env_ex: the rate evaluator's inputs instead of the rate constants
        r = np.ascontiguousarray(env, np.float64).reshape(ncell, -1)
        assert r.shape[1] == lib().mistra_chem_rates_env_size(mid)
    else:
        r = np.ascontiguousarray(rconst, np.float64).reshape(ncell, nreact)
    out = np.empty_like(v)
    ierr = np.zeros(ncell, np.int32)
    stats = np.zeros((ncell, 8), np.int32)
    th = np.zeros((ncell, 3))
    if hstart is not None:
        rp, ep = (None, r.ctypes.data_as(_dp)) if env is not None else (r.ctypes.data_as(_dp), None)
        _check(lib().mistra_chem_integrate_hstart_ex(mid, ncell, v.ctypes.data_as(_dp), f.ctypes.data_as(_dp), rp, ep, float(tin), float(tout),
                                                     out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip),
                                                     th.ctypes.data_as(_dp), hs.ctypes.data_as(_dp)))
        return IntegrateResult(out, ierr, stats), th
    _check((lib().mistra_chem_integrate_env_ex if env is not None else lib().mistra_chem_integrate_ex)(mid, ncell, v.ctypes.data_as(_dp), f.ctypes.data_as(_dp), r.ctypes.data_as(_dp),
                                         float(tin), float(tout), out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip),
                                         stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp)))
    return IntegrateResult(out, ierr, stats), th


def singular_rows(mech, cell):
    """Rows (1-based) of the zero pivots cell `cell` of the last host-buffer integrate call met (include/mistra_chem.h:
    mistra_chem_singular_rows); meaningful for the first min(Nsng, 8) entries."""
    mid, _ = _mech_id(mech)
    rows = np.zeros(8, np.int32)
    _check(lib().mistra_chem_singular_rows(mid, int(cell), rows.ctypes.data_as(_ip)))
    return rows


def device_count():
    return lib().mistra_chem_device_count()


def _integrate_torch(mid, name, var, fix, rconst, tin, tout, out=None, ierr=None, stats=None, texit_hexit=None, hstart=None):
    import torch
    nvar, nfix, nreact, _ = DIMS[name]
    if not var.is_cuda:
        raise MistraChemError("torch tensors must live on the GPU (there is no CPU path); pass numpy arrays for host data")
    dev = var.device.index or 0
    init(dev)
    for x, n in ((var, nvar), (fix, nfix), (rconst, nreact)):
        if x.dtype != torch.float64 or not x.is_contiguous() or x.shape[-1] != n or x.device != var.device:
            raise MistraChemError("expected contiguous float64 [ncell,%d] tensors on one device" % n)
    ncell = var.numel() // nvar
    if fix.numel() != ncell * nfix or rconst.numel() != ncell * nreact:
        raise MistraChemError("cell counts of var / fix / rconst differ")
    out = torch.empty_like(var) if out is None else out
    ierr = torch.empty(ncell, dtype=torch.int32, device=var.device) if ierr is None else ierr
    stats = torch.empty((ncell, 8), dtype=torch.int32, device=var.device) if stats is None else stats
    stream = torch.cuda.current_stream(var.device).cuda_stream
    _check(lib().mistra_chem_integrate_device_hstart(mid, ncell, var.data_ptr(), fix.data_ptr(), rconst.data_ptr(), float(tin),
                                                    float(tout), out.data_ptr(), ierr.data_ptr(), stats.data_ptr(),
                                                    None if texit_hexit is None else texit_hexit.data_ptr(),
                                                    None if hstart is None else hstart.data_ptr(), C.c_void_p(stream)))
    return IntegrateResult(out, ierr, stats)


def update_rconst(mech, env):
    """Update_RCONST_x for a batch of cells (gas.f:275): env [ncell, rates_env_size] -> rconst [ncell, NREACT].  numpy in ->
    numpy out; torch CUDA tensor in -> torch tensor out, on torch's current stream.  Entry names of env: mistra_amd/mech/<mech>.rates_env.json."""
    mid, name = _mech_id(mech)
    nreact = DIMS[name][2]
    try:
        import torch
        is_torch = isinstance(env, torch.Tensor)
    except ImportError:      # pragma: no cover
        is_torch = False
    if is_torch:
        init(env.device.index or 0)
        ne = lib().mistra_chem_rates_env_size(mid)
        if env.dtype != torch.float64 or not env.is_contiguous() or env.shape[-1] != ne:
            raise MistraChemError("expected a contiguous float64 [ncell,%d] tensor" % ne)
        out = torch.empty((env.numel() // ne, nreact), dtype=torch.float64, device=env.device)
        stream = torch.cuda.current_stream(env.device).cuda_stream
        _check(lib().mistra_chem_update_rconst_device(mid, out.shape[0], env.data_ptr(), out.data_ptr(), C.c_void_p(stream)))
        return out
    if _inited_device is None:
        init(0)
    ne = lib().mistra_chem_rates_env_size(mid)
    e = np.ascontiguousarray(env, np.float64).reshape(-1, ne if ne else 1)
    out = np.empty((e.shape[0], nreact))
    _check(lib().mistra_chem_update_rconst(mid, e.shape[0], e.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


# ---- Rosenbrock_x's options (include/mistra_chem.h: mistra_chem_set_options).  INTEGRATE_x's own: gas.f:739-746
BASE_IPAR = (0, 1, 0, 2)           # IPAR(1:4): time dependent, scalar tolerances, 100000 steps, Ros3
BASE_RPAR = (0.0, 0.0, 1.0e-3)     # RPAR(1:3): Hmin 0, Hmax the interval, Hstart 1e-3
BASE_RTOL, BASE_ATOL = 1.0e-3, 1.0e-25
Options = namedtuple("Options", "ipar rpar atol rtol")
ResolvedOptions = namedtuple("ResolvedOptions", "ierr hmin hmax hstart facmin facmax facrej facsafe max_steps autonomous vector")


def _option_args(name, ipar, rpar, atol, rtol):
    """IPAR(20), RPAR(20), AbsTol(NVAR), RelTol(NVAR) from what the caller gave: None = INTEGRATE_x's value, a shorter ipar / rpar is padded
    with zeros, a scalar tolerance fills the vector."""
    nvar = DIMS[name][0]
    ip, rp = np.zeros(20, np.int32), np.zeros(20, np.float64)
    for out, given, base, what in ((ip, ipar, BASE_IPAR, "ipar"), (rp, rpar, BASE_RPAR, "rpar")):
        v = np.atleast_1d(np.asarray(base if given is None else given))
        if v.ndim != 1 or v.size > 20:
            raise MistraChemError("%s: at most 20 entries, as Rosenbrock_x takes them" % what)
        if what == "ipar" and not np.all(np.equal(np.mod(v, 1), 0)):
            raise MistraChemError("ipar: integers expected")
        out[:v.size] = v
    tol = []
    for given, base, what in ((atol, BASE_ATOL, "atol"), (rtol, BASE_RTOL, "rtol")):
        v = np.asarray(base if given is None else given, np.float64)
        if v.ndim == 0:
            v = np.full(nvar, float(v))
        if v.shape != (nvar,):
            raise MistraChemError("%s: a scalar or %d entries (NVAR of %s) expected" % (what, nvar, name))
        tol.append(np.ascontiguousarray(v))
    return ip, rp, tol[0], tol[1]


def check_options(mech, ipar=None, rpar=None, atol=None, rtol=None, interval=10.0):
    """Rosenbrock_x's decode of its options (gas.f:936-1053) without a GPU -> ResolvedOptions: ierr = 1 or the IERR it would return (-1 .. -5, the
    other fields are then None), else Hmin, Hmax, Hstart for a call over `interval`, the four factors, Max_no_steps, autonomous, vector.  A valid
    method that is not built (anything but Ros3) raises."""
    mid, name = _mech_id(mech)
    ip, rp, at, rt = _option_args(name, ipar, rpar, atol, rtol)
    ierr, r, i = C.c_int32(0), np.zeros(7), np.zeros(3, np.int32)
    _check(lib().mistra_chem_check_options(mid, ip.ctypes.data_as(_ip), rp.ctypes.data_as(_dp), at.ctypes.data_as(_dp), rt.ctypes.data_as(_dp),
                                           float(interval), C.byref(ierr), r.ctypes.data_as(_dp), i.ctypes.data_as(_ip)))
    if ierr.value != 1:
        return ResolvedOptions(ierr.value, *([None] * 10))
    return ResolvedOptions(1, *[float(x) for x in r], int(i[0]), bool(i[1]), bool(i[2]))


def set_options(mech, ipar=None, rpar=None, atol=None, rtol=None):
    """Rosenbrock_x's IPAR, RPAR, AbsTol, RelTol for every later integrate call of `mech` (mistra_chem_set_options), instead of the values
    INTEGRATE_x hard-codes; None = INTEGRATE_x's value for that argument.  Options Rosenbrock_x would refuse, or a method that is not built, raise
    and leave the previous ones in force."""
    mid, name = _mech_id(mech)
    ip, rp, at, rt = _option_args(name, ipar, rpar, atol, rtol)
    if _inited_device is None:
        init(0)
    ierr = C.c_int32(0)
    _check(lib().mistra_chem_set_options(mid, ip.ctypes.data_as(_ip), rp.ctypes.data_as(_dp), at.ctypes.data_as(_dp), rt.ctypes.data_as(_dp),
                                         C.byref(ierr)))


def clear_options(mech):
    """Back to INTEGRATE_x's values for `mech`."""
    mid, _ = _mech_id(mech)
    if _inited_device is None:
        return
    _check(lib().mistra_chem_set_options(mid, None, None, None, None, None))


def get_options(mech):
    """-> Options(ipar[20], rpar[20], atol[NVAR], rtol[NVAR]) in force for `mech` (the tolerances as the integrator uses them), or None."""
    mid, name = _mech_id(mech)
    nvar = DIMS[name][0]
    is_set, ip, rp, at, rt = C.c_int32(0), np.zeros(20, np.int32), np.zeros(20), np.zeros(nvar), np.zeros(nvar)
    _check(lib().mistra_chem_get_options(mid, C.byref(is_set), ip.ctypes.data_as(_ip), rp.ctypes.data_as(_dp), at.ctypes.data_as(_dp),
                                         rt.ctypes.data_as(_dp)))
    return Options(ip, rp, at, rt) if is_set.value else None


# ---- Rosenbrock_x itself, batched, with all five methods and the options travelling with the call (include/mistra_chem.h: mistra_chem_rosenbrock_ex)
METHOD_NAMES = {1: "Ros2", 2: "Ros3", 3: "Ros4", 4: "Rodas3", 5: "Rodas4"}
MethodTable = namedtuple("MethodTable", "S A C M E gamma newf elo")


def method_table(method):
    """The tables the kernels are compiled with for IPAR(4) = `method` (1 Ros2, 2 Ros3, 3 Ros4, 4 Rodas3, 5 Rodas4; 0 = 3 as in Rosenbrock_x) ->
    MethodTable(S, A[S(S-1)/2], C[S(S-1)/2], M[S], E[S], gamma[S], newf[S] (bool), elo).  Needs no GPU."""
    s, elo = C.c_int(0), C.c_double(0.0)
    a, c, m, e, g, nf = np.zeros(15), np.zeros(15), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6, np.int32)
    _check(lib().mistra_chem_method_table(int(method), C.byref(s), a.ctypes.data_as(_dp), c.ctypes.data_as(_dp), m.ctypes.data_as(_dp),
                                          e.ctypes.data_as(_dp), g.ctypes.data_as(_dp), nf.ctypes.data_as(_ip), C.byref(elo)))
    n, low = s.value, s.value * (s.value - 1) // 2
    return MethodTable(n, a[:low].copy(), c[:low].copy(), m[:n].copy(), e[:n].copy(), g[:n].copy(), nf[:n].astype(bool), elo.value)


# ---- the integrator policy (include/mistra_chem.h: mistra_chem_set_policy): opt-in, per mechanism; what the integrate family and the column driver
#      run instead of Ros3 and the options' AbsTol
Policy = namedtuple("Policy", "method atol_rel atol_floor")


def _policy_args(method, atol_rel, atol_floor):
    if isinstance(method, str):
        by_name = {v.lower(): k for k, v in METHOD_NAMES.items()}
        if method.lower() not in by_name:
            raise MistraChemError("policy: unknown method %r (%s)" % (method, ", ".join(METHOD_NAMES.values())))
        method = by_name[method.lower()]
    return int(method), 0.0 if atol_rel is None else float(atol_rel), float(atol_floor)


def check_policy(mech, method=2, atol_rel=None, atol_floor=1.0e-25):
    """The checks of set_policy alone (mistra_chem_check_policy): raises with the library's text where set_policy would.  Needs no GPU."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_check_policy(mid, *_policy_args(method, atol_rel, atol_floor)))


def set_policy(mech, method=2, atol_rel=None, atol_floor=1.0e-25):
    """The integrator policy of `mech` (mistra_chem_set_policy) for every later integrate call and column step: `method` 1 .. 5 or a METHOD_NAMES
    string (2 / "Ros3" keeps the method), `atol_rel` None or 0 = the options' AbsTol, else AbsTol = max(atol_floor, atol_rel * max|VAR|) per cell.
    Everything else stays the options in force.  The rosenbrock* calls and debug_first_step ignore it."""
    mid, _ = _mech_id(mech)
    args = _policy_args(method, atol_rel, atol_floor)
    _check(lib().mistra_chem_check_policy(mid, *args))      # (a refusal needs no device)
    if _inited_device is None:
        init(0)
    _check(lib().mistra_chem_set_policy(mid, *args))


def clear_policy(mech):
    """No policy for `mech`: Ros3 and the options' AbsTol, as without these calls."""
    mid, _ = _mech_id(mech)
    if _inited_device is None:
        return
    _check(lib().mistra_chem_clear_policy(mid))


def get_policy(mech):
    """-> Policy(method, atol_rel, atol_floor) in force for `mech` (atol_rel 0.0 = none), or None.  Needs no GPU."""
    mid, _ = _mech_id(mech)
    is_set, method, factor, floor = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
    _check(lib().mistra_chem_get_policy(mid, C.byref(is_set), C.byref(method), C.byref(factor), C.byref(floor)))
    return Policy(method.value, factor.value, floor.value) if is_set.value else None


# ---- the front every Rosenbrock_x function shares: the cell arrays described once (_front), the tolerance arguments (_tol_args), the trace arrays
#      (_trace_arrays).  A family function is then what is particular to it: its extra arrays and which library entry it calls.
def _is_torch(x):
    try:
        import torch
        return isinstance(x, torch.Tensor)
    except ImportError:      # pragma: no cover
        return False


class _Front:
    """The cell arrays of a call: torch CUDA tensors (torch: the module; the device entries, on torch's current stream) or numpy arrays (torch None: the
    host entries).  ptrs: var, fix, rconst as the entries take them; hstart: None or the checked array; nlf, nlr: the blocks of fix and rconst."""

    def __init__(self, name, torch, var, fix, rconst, hstart, ncell, nlf, nlr):
        self.name, self.torch, self.var, self.hstart, self.ncell, self.nlf, self.nlr = name, torch, var, hstart, ncell, nlf, nlr
        self.device = var.device if torch else None
        self.ptrs = (self.ptr(var), self.ptr(fix), self.ptr(rconst))
        self.stream = C.c_void_p(torch.cuda.current_stream(var.device).cuda_stream) if torch else None
        self.form = "device" if torch else "ex"

    def ptr(self, x):
        if x is None:
            return None
        return x.data_ptr() if self.torch else x.ctypes.data_as(_ip if x.dtype == np.int32 else _dp)

    def new(self, shape, dtype="float64", zero=False):
        """an array of the cells' kind; a host array is zeroed in any case, a tensor where the entry leaves part of it unwritten"""
        if self.torch:
            return (self.torch.zeros if zero else self.torch.empty)(shape, dtype=getattr(self.torch, dtype), device=self.device)
        return np.zeros(shape, getattr(np, dtype))

    def results(self, rows=None, out=None):
        """-> out, ierr, stats, th of one call (rows None) or of the `rows` legs of a series; th holds 2 entries per cell on the device, 3 on the host"""
        lead = () if rows is None else (rows,)
        nvar = DIMS[self.name][0]
        if not self.torch:
            out = np.empty(lead + (self.ncell, nvar))
        elif out is None:
            out = self.torch.empty_like(self.var) if rows is None else self.new(lead + (self.ncell, nvar))
        elif out.dtype != self.torch.float64 or not out.is_contiguous() or out.numel() != rows * self.ncell * nvar or out.device != self.device:
            raise MistraChemError("out: a contiguous float64 [nleg, ncell, %d] tensor on the cells' device expected" % nvar)
        return out, self.new(lead + (self.ncell,), "int32"), self.new(lead + (self.ncell, 8), "int32"), self.new(lead + (self.ncell, 2 if self.torch else 3))


def _front(name, var, fix, rconst, hstart, host_hstart=False, init_host=False, blocks=None):
    """var, fix, rconst [ncell, .] and hstart [ncell] checked -> _Front.  A tensor var selects the device entries, and the library is brought up on its
    device; numpy arrays select the host entries, whose arguments the library checks before it looks for a device: no init() in front of them unless
    init_host.  host_hstart: the host entry takes hstart (else it goes with the device entry).  blocks(fix, rconst) -> (nlf, nlr): fix and rconst may
    hold several blocks [nl, ncell, .] (the series with rates)."""
    nvar, nfix, nreact, _ = DIMS[name]
    torch = None
    if _is_torch(var):
        import torch
        if not var.is_cuda:
            raise MistraChemError("torch tensors must live on the GPU (there is no CPU path); pass numpy arrays for host data")
        init(var.device.index or 0)
        for x, n in ((var, nvar), (fix, nfix), (rconst, nreact)):
            if not _is_torch(x) or x.dtype != torch.float64 or not x.is_contiguous() or x.shape[-1] != n or x.device != var.device:
                raise MistraChemError("expected contiguous float64 [%sncell,%d] tensors on one device" % ("..., " if blocks else "", n))
        ncell = var.numel() // nvar
        if hstart is not None and (hstart.dtype != torch.float64 or not hstart.is_contiguous() or hstart.numel() != ncell or hstart.device != var.device):
            raise MistraChemError("hstart: a contiguous float64 tensor of %d entries on the cells' device expected" % ncell)
    else:
        if hstart is not None and not host_hstart:
            raise MistraChemError("hstart goes with the device entry: pass torch CUDA tensors (host buffers: rpar[2] is the first step size of every cell)")
        if init_host and _inited_device is None:
            init(0)
        var = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
        ncell = var.shape[0]
        fix, rconst = np.ascontiguousarray(fix, np.float64), np.ascontiguousarray(rconst, np.float64)
        if not blocks:
            fix, rconst = fix.reshape(ncell, nfix), rconst.reshape(ncell, nreact)
        if hstart is not None:
            hstart = np.ascontiguousarray(hstart, np.float64).reshape(-1)
            if hstart.size != ncell:
                raise MistraChemError("hstart: %d entries expected" % ncell)
    nlf, nlr = blocks(fix, rconst) if blocks else (1, 1)
    size = (lambda x: x.numel()) if torch else (lambda x: x.size)
    if size(fix) != nlf * ncell * nfix or size(rconst) != nlr * ncell * nreact:
        raise MistraChemError("cell counts of var / fix / rconst differ")
    return _Front(name, torch, var, fix, rconst, hstart, ncell, nlf, nlr)


def _options(name, cells, ipar, rpar, atol, rtol):
    """_option_args for a call whose tolerances are the shared pair (cells false) or come in rows per cell (the pair is then INTEGRATE_x's, unread)"""
    return _option_args(name, ipar, rpar, None if cells else atol, None if cells else rtol)


def _tol_args(fr, opts, cells, atol, rtol):
    """The tolerance and option arguments of an entry, opts from _options: the shared pair, or with cells the rows atol, rtol [ncell, ntol] of the
    cells' kind -> (atol, rtol[, ntol], rpar, ipar) as the entry takes them"""
    ip, rp, at, rt = opts
    popts = (rp.ctypes.data_as(_dp), ip.ctypes.data_as(_ip))
    if not cells:
        return (at.ctypes.data_as(_dp), rt.ctypes.data_as(_dp)) + popts
    if fr.torch:
        for x in (atol, rtol):
            if not _is_torch(x) or x.dtype != fr.torch.float64 or not x.is_contiguous() or x.ndim != 2 or x.shape[0] != fr.ncell or x.device != fr.device:
                raise MistraChemError("atol / rtol: contiguous float64 [ncell, 1] or [ncell, NVAR] tensors on the cells' device expected")
        if atol.shape != rtol.shape:
            raise MistraChemError("atol and rtol differ in shape")
    else:
        atol, rtol = np.ascontiguousarray(atol, np.float64), np.ascontiguousarray(rtol, np.float64)
        if atol.ndim != 2 or atol.shape[0] != fr.ncell or rtol.shape != atol.shape:
            raise MistraChemError("atol / rtol: [ncell, 1] or [ncell, NVAR] arrays of one shape expected")
    return (fr.ptr(atol), fr.ptr(rtol), int(atol.shape[1])) + popts


def _trace_arrays(fr, cap, ctrl, trace_d, trace_i):
    """The log arrays of a trace entry, the caller's or new ones of the cells' kind -> (the entry's trace arguments, the Trace of views into them)"""
    cap = int(cap)
    rows, ncell = max(cap, 0), fr.ncell
    td = fr.new((ncell, rows, 4), zero=True) if trace_d is None else trace_d
    ti = fr.new((ncell, rows, 2), "int32", zero=True) if trace_i is None else trace_i
    for x, dt, k in ((td, "float64", 4), (ti, "int32", 2)):
        if fr.torch:
            if x.dtype != getattr(fr.torch, dt) or not x.is_contiguous() or x.numel() != ncell * rows * k or x.device != fr.device:
                raise MistraChemError("trace_d / trace_i: contiguous float64 [ncell, cap, 4] / int32 [ncell, cap, 2] tensors on the cells' device expected")
        elif not isinstance(x, np.ndarray) or x.dtype != getattr(np, dt) or not x.flags.c_contiguous or x.size != ncell * rows * k:
            raise MistraChemError("trace_d / trace_i: C-contiguous float64 [ncell, cap, 4] / int32 [ncell, cap, 2] arrays expected")
    td, ti = td.reshape(ncell, rows, 4), ti.reshape(ncell, rows, 2)
    nt = fr.new((ncell,), "int32")
    ct = fr.new((ncell, DIMS[fr.name][0]), "int32", zero=True) if ctrl else None
    args = (cap, fr.ptr(td) if rows else None, fr.ptr(ti) if rows else None, fr.ptr(nt), fr.ptr(ct))
    return args, (Trace(td[..., 0], td[..., 1], td[..., 2], td[..., 3], ti[..., 0], ti[..., 1], nt, ct),)


def _ros_single(stem, mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, cells, extra=None, init_host=False):
    """One call through mistra_chem_<stem>[_cells]_ex / _device -> (IntegrateResult, t_h) + what the family adds.  extra(front) -> (the entry's arguments
    behind the plain call's, the results behind rosenbrock's pair)"""
    mid, name = _mech_id(mech)
    opts = _options(name, cells, ipar, rpar, atol, rtol)
    fr = _front(name, var, fix, rconst, hstart, init_host=init_host)
    tol = _tol_args(fr, opts, cells, atol, rtol)
    out, ierr, stats, th = fr.results()
    args, more = extra(fr) if extra else ((), ())
    tail = (fr.ptr(fr.hstart), fr.stream) if fr.torch else ()
    entry = getattr(lib(), "mistra_chem_%s_%s%s" % (stem, "cells_" if cells else "", fr.form))
    _check(entry(mid, fr.ncell, *fr.ptrs, float(tstart), float(tend), *tol, fr.ptr(out), fr.ptr(ierr), fr.ptr(stats), fr.ptr(th), *tail, *args))
    return (IntegrateResult(out, ierr, stats), th) + more


def rosenbrock(mech, var, fix, rconst, tstart, tend, ipar=None, rpar=None, atol=None, rtol=None, hstart=None):
    """Rosenbrock_x(Y, Tstart, Tend, AbsTol, RelTol, RPAR, IPAR, IERR) over a batch of cells, any of its five methods (ipar[3]); the options are this
    call's alone — None = INTEGRATE_x's value — and the ones in force (set_options) are neither read nor changed.  numpy arrays: the host entry,
    -> (IntegrateResult, t_h [ncell, 3]) as integrate_ex; torch CUDA tensors: the device entry on torch's current stream, -> (IntegrateResult,
    texit_hexit [ncell, 2]), hstart [ncell] (a tensor, device entry only): first step size per cell, entries <= 0 = rpar[2].  Options Rosenbrock_x
    refuses do not raise: every cell's ierr is its code (-1 .. -5), var comes back unchanged, stats and t_h are zero."""
    return _ros_single("rosenbrock", mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, False, init_host=True)


# ---- the step-control trace (include/mistra_chem.h: mistra_chem_rosenbrock_trace_ex / _device)
# t, h, err, share [ncell, cap]; species, code [ncell, cap] int32; n [ncell] int32: the TRUE number of attempts; ctrl [ncell, NVAR] int32 or None
Trace = namedtuple("Trace", "t h err share species code n ctrl")


def rosenbrock_trace(mech, var, fix, rconst, tstart, tend, ipar=None, rpar=None, atol=None, rtol=None, hstart=None, cap=256, ctrl=True,
                     trace_d=None, trace_i=None):
    """rosenbrock() (Ros3 only) run by the kernel that also records every attempt of the step control -> rosenbrock's tuple + a Trace.  Per
    attempt: t (start of the step), h (as attempted), err, the species (1-based, 0 = none) with the largest term of the error norm's sum and its
    share of NVAR*err**2, code = accepted + 2 * zero pivots of the attempt.  cap: records kept per cell; n counts all attempts, records past cap
    are dropped, rows past min(n, cap) are as they were (zeros, or what the caller's trace_d [ncell, cap, 4] / trace_i [ncell, cap, 2] held).
    ctrl: whether the per-species count of controlled attempts is wanted.  The Trace's arrays are views of the log arrays, of the inputs' kind."""
    return _ros_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, (cap, ctrl, trace_d, trace_i), False)


# ---- tolerances per cell (include/mistra_chem.h: mistra_chem_rosenbrock_cells_ex / _device, their trace forms, mistra_chem_cell_atol_device)
def _ros_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, trace, cells=True):
    """rosenbrock_cells (trace None) and rosenbrock_trace_cells (trace = (cap, ctrl, trace_d, trace_i)); cells false: rosenbrock_trace"""
    if trace is None:
        return _ros_single("rosenbrock", mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, cells)
    return _ros_single("rosenbrock_trace", mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, cells, lambda fr: _trace_arrays(fr, *trace))


def rosenbrock_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart=None):
    """rosenbrock() with tolerances PER CELL: atol, rtol shaped (ncell, 1) or (ncell, NVAR), cell c integrates with row c.  ipar[1] = 0 (vector
    tolerances) needs NVAR columns; scalar tolerances read column 0 alone, whatever the width.  numpy arrays: the host entry; torch CUDA tensors
    (the tolerances too, read by the kernel in stream order): the device entry.  ipar, rpar: None = INTEGRATE_x's values.  IERR = -5 is a result per
    cell: a cell whose row Rosenbrock_x would refuse comes back unchanged with ierr = -5 and zero stats / t_h, the others run."""
    return _ros_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, None)


def rosenbrock_trace_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart=None, cap=256, ctrl=True, trace_d=None, trace_i=None):
    """rosenbrock_trace() with tolerances per cell as rosenbrock_cells takes them; a cell refused with -5 has n = 0 and its log rows untouched."""
    return _ros_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, (cap, ctrl, trace_d, trace_i))


# ---- the reaction flux (include/mistra_chem.h: mistra_chem_rosenbrock_flux_ex / _device and their cells forms)
def _ros_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, cells, ts=None):
    """rosenbrock_flux (cells False: the shared pair) and rosenbrock_flux_cells (cells True: atol, rtol [ncell, ntol]); ts set: the dense-output entries
    (rosenbrock_dense / rosenbrock_dense_cells), which return samples [ns, ncell, NVAR] and nout [ncell] where the flux entries return the flux"""
    if ts is not None:      # a host array whatever the cells are: it travels with the call's options
        ts = np.ascontiguousarray(ts, np.float64).reshape(-1)

    def extra(fr):
        nvar, _, nreact, _ = DIMS[fr.name]
        if ts is None:
            flux = fr.new((fr.ncell, nreact))
            return (fr.ptr(flux),), (flux,)
        samples, nout = fr.new((ts.size, fr.ncell, nvar)), fr.new((fr.ncell,), "int32")
        return (int(ts.size), ts.ctypes.data_as(_dp), fr.ptr(samples), fr.ptr(nout)), (samples, nout)

    return _ros_single("rosenbrock_flux" if ts is None else "rosenbrock_dense", mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, cells, extra)


def rosenbrock_flux(mech, var, fix, rconst, tstart, tend, ipar=None, rpar=None, atol=None, rtol=None, hstart=None):
    """rosenbrock() run by the kernel that also integrates every reaction's rate over the call -> rosenbrock's tuple + flux [ncell, NREACT]:
    flux[r] = sum over the accepted steps of (0.5 * Direction * H) * (A_r(Y_n) + A_r(Y_n+1)), A_r the product Fun_x forms.  The first two results
    are bit for bit rosenbrock()'s.  A refused call, and a call that makes no accepted step, return zeros.  Not for a user mechanism slot."""
    return _ros_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, False)


def rosenbrock_flux_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart=None):
    """rosenbrock_flux() with tolerances per cell as rosenbrock_cells takes them; a cell refused with -5 has a flux row of zeros."""
    return _ros_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, True)


# ---- dense output (include/mistra_chem.h: mistra_chem_rosenbrock_dense_ex / _device and their cells forms)
def rosenbrock_dense(mech, var, fix, rconst, tstart, tend, ts, ipar=None, rpar=None, atol=None, rtol=None, hstart=None):
    """rosenbrock() run by the kernel that also leaves the state at the sample times ts (a host array: finite, strictly monotone from tstart towards
    tend, tstart excluded, tend allowed) -> rosenbrock's tuple + samples [ns, ncell, NVAR] + nout [ncell].  The call itself is not changed by looking:
    the first two results are bit for bit rosenbrock()'s.  A sample is the cubic Hermite interpolant between the two accepted states around it
    (INTEGRATION.md 4o); nout[c] samples were reached (fewer than ns after IERR < 0), the rows behind them are zeros.  numpy arrays go to the host entry,
    torch CUDA tensors to the device entry on the current stream.  Not for a user mechanism slot."""
    return _ros_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, False, ts)


def rosenbrock_dense_cells(mech, var, fix, rconst, tstart, tend, ts, ipar, rpar, atol, rtol, hstart=None):
    """rosenbrock_dense() with tolerances per cell as rosenbrock_cells takes them; a cell refused with -5 has nout = 0 and rows of zeros."""
    return _ros_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, hstart, True, ts)


# ---- a series: several output times in one call (include/mistra_chem.h: mistra_chem_rosenbrock_series_ex / _device and their cells forms)
SERIES_MAX_LEGS = 4096      # MISTRA_SERIES_MAX_LEGS
# var [nleg, ncell, NVAR]; ierr [nleg, ncell]; stats [nleg, ncell, 8]; t_h [nleg, ncell, 3] (host: Texit, Hexit, H) or [nleg, ncell, 2] (device)
SeriesResult = namedtuple("SeriesResult", "var ierr stats t_h")


def rosenbrock_series(mech, var, fix, rconst, times, ipar=None, rpar=None, atol=None, rtol=None, hstart=None, carry_h=False, out=None):
    """nleg = len(times) - 1 calls of Rosenbrock_x in one launch: leg k integrates from times[k] to times[k+1] on the state leg k-1 left, with the
    state, FIX and the rate constants on chip throughout -> SeriesResult of per-leg arrays, bit for bit what rosenbrock() / rosenbrock_cells() called
    leg by leg return.  times: finite, strictly ascending or descending.  A 2-D atol / rtol ([ncell, 1] or [ncell, NVAR]) selects the cells form.
    numpy arrays: the host entry; torch CUDA tensors: the device entry on torch's current stream.  hstart [ncell]: first step per cell of leg 0,
    entries <= 0 = rpar[2].  carry_h: a later leg starts with the previous leg's Hexit of the cell where that is > 0, instead of rpar[2].  out
    (device entry): a [nleg, ncell, NVAR] tensor to receive the states; var may be one leg's block of it.  Options Rosenbrock_x refuses are results
    in every leg, as for rosenbrock()."""
    return _series_rates(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart, carry_h, out, False, rates=False)


def rosenbrock_series_rates(mech, var, fix, rconst, times, ipar=None, rpar=None, atol=None, rtol=None, hstart=None, carry_h=False, out=None):
    """rosenbrock_series() with FIX and the rate constants of the leg's own: Update_RCONST_x + INTEGRATE_x, nleg = len(times) - 1 times, in one launch
    (include/mistra_chem.h: mistra_chem_rosenbrock_series_rates_ex / _device and their cells forms).  fix and rconst: 2-D [ncell, .] (one block shared
    by all legs) or 3-D [nleg, ncell, .] (leg k integrates with block k; a leading 1 is the shared block), each on its own -> SeriesResult, bit for
    bit what rosenbrock() / rosenbrock_cells() called leg by leg with leg k's rows return.  rconst [nleg, ncell, NREACT] is what update_rconst over
    nleg*ncell env rows, leg-major, returns, reshaped or not.  Everything else as rosenbrock_series(): numpy arrays go to the host entry, torch CUDA
    tensors to the device entry on torch's current stream (fix and rconst are read at the head of every leg: leave them untouched until the stream has
    passed the call, and they may not overlap out); a 2-D atol / rtol selects the cells form."""
    return _series_rates(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart, carry_h, out, False)


def rosenbrock_series_linrates(mech, var, fix, rconst_nodes, times, ipar=None, rpar=None, atol=None, rtol=None, hstart=None, carry_h=False, out=None):
    """rosenbrock_series_rates() with rate constants LINEAR IN TIME over each leg (include/mistra_chem.h: mistra_chem_rosenbrock_series_linrates_ex /
    _device and their cells forms).  rconst_nodes: 3-D [nleg + 1, ncell, NREACT], block k the rate constants AT times[k]: what
    update_rconst over (nleg + 1)*ncell env rows, node-major, returns.  Inside leg k every function evaluation reads R0 + ((tau - times[k]) * w) * (R1 - R0)
    at its own time tau, w = 1/(times[k+1] - times[k]), and with ipar[0] = 0 the stages add H*gamma_i * Fun(Y, FIX, dR/dt), the exact dFdT.  fix: 2-D
    (shared) or 3-D [nleg, ncell, NFIX], piecewise constant.  Everything else as rosenbrock_series_rates() -> SeriesResult; equal node blocks give that
    function's results on the shared block, up to the sign of a zero."""
    return _series_rates(mech, var, fix, rconst_nodes, times, ipar, rpar, atol, rtol, hstart, carry_h, out, True)


# rosenbrock_series_rates' result with the reaction flux of every leg: flux [nleg, ncell, NREACT]
SeriesFluxResult = namedtuple("SeriesFluxResult", "var ierr stats t_h flux")


def rosenbrock_series_flux(mech, var, fix, rconst, times, ipar=None, rpar=None, atol=None, rtol=None, hstart=None, carry_h=False, out=None):
    """rosenbrock_series_rates() run by the kernels that also integrate every reaction's rate over each leg: a budget time series in one launch
    (include/mistra_chem.h: mistra_chem_rosenbrock_series_flux_ex / _device).  fix and rconst as rosenbrock_series_rates
    takes them: one block [ncell, .] shared by all legs, or one per leg [nleg, ncell, .], each on its own -> SeriesFluxResult: that function's result,
    bit for bit, plus flux [nleg, ncell, NREACT], block k exactly what rosenbrock_flux() returns for the call that leg k is (from times[k] to times[k+1]
    on the state leg k-1 left, with leg k's rows and the first step the series gives the leg).  No leg's sum is carried into the next; a refused call,
    and in the cells form a refused cell, has rows of zeros in every leg.  numpy arrays go to the host entry, torch CUDA tensors to the device entry on
    torch's current stream; a 2-D atol / rtol selects the cells form.  Not for a user mechanism slot, and there is no form with rate constants linear
    in time."""
    return _series_rates(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart, carry_h, out, False, True)


def rosenbrock_series_flux_cells(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart=None, carry_h=False, out=None):
    """rosenbrock_series_flux() with tolerances per cell, atol / rtol [ncell, 1] or [ncell, NVAR] as rosenbrock_cells takes them; a cell refused with -5
    has a flux row of zeros in every leg, its neighbours are not affected."""
    if getattr(atol, "ndim", 0) != 2 or getattr(rtol, "ndim", 0) != 2:
        raise MistraChemError("atol / rtol: [ncell, 1] or [ncell, NVAR] arrays of one shape expected")
    return _series_rates(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart, carry_h, out, False, True)


def _series_rates(mech, var, fix, rconst, times, ipar, rpar, atol, rtol, hstart, carry_h, out, lin, flux=False, rates=True):
    """rosenbrock_series_rates (lin false), rosenbrock_series_linrates (lin true: rconst holds the nleg + 1 node blocks, and the entries take no count
    of them) and rosenbrock_series_flux (flux true: the entries take flux_series behind the series with rates' arguments); rates false:
    rosenbrock_series, whose entries take one block of fix and of rconst and no counts"""
    mid, name = _mech_id(mech)
    nvar, _, nreact, _ = DIMS[name]
    cells = atol is not None and rtol is not None and getattr(atol, "ndim", 0) == 2 and getattr(rtol, "ndim", 0) == 2
    opts = _options(name, cells, ipar, rpar, atol, rtol)
    tm = np.ascontiguousarray(times, np.float64).reshape(-1)
    nleg = tm.size - 1
    rows = max(nleg, 0)

    def legs(x, what):      # the number of blocks of fix / rconst: the library refuses one that is neither 1 nor nleg, by its text
        if x.ndim not in (2, 3):
            raise MistraChemError("%s: a 2-D [ncell, .] array (shared by all legs) or a 3-D [nleg, ncell, .] one expected" % what)
        return 1 if x.ndim == 2 else int(x.shape[0])

    def nodes(x):           # (lin) the node blocks: exactly nleg + 1 of them; the library takes no count
        if x.ndim != 3 or int(x.shape[0]) != rows + 1:
            raise MistraChemError("rconst_nodes: a 3-D [nleg + 1, ncell, NREACT] array expected, block k the rate constants at times[k] (nleg = %d)" % nleg)
        return rows + 1

    fr = _front(name, var, fix, rconst, hstart, host_hstart=True,
                blocks=(lambda f, r: (legs(f, "fix"), nodes(r) if lin else legs(r, "rconst"))) if rates else None)
    tol = _tol_args(fr, opts, cells, atol, rtol)
    res, ierr, stats, th = fr.results(rows, out)
    fl = fr.new((rows, fr.ncell, nreact)) if flux else None
    counts = ((() if lin else (fr.nlr,)) + (fr.nlf,)) if rates else ()
    results = (fr.ptr(res), fr.ptr(ierr), fr.ptr(stats), fr.ptr(th))
    start = (int(bool(carry_h)), fr.ptr(fr.hstart))
    tail = results + start + (fr.stream,) if fr.torch else start + results      # (the two forms' own order)
    stem = "series" + ("_linrates" if lin else "_flux" if flux else "_rates" if rates else "")
    entry = getattr(lib(), "mistra_chem_rosenbrock_%s_%s%s" % (stem, "cells_" if cells else "", fr.form))
    _check(entry(mid, fr.ncell, *fr.ptrs, *counts, nleg, tm.ctypes.data_as(_dp), *tol, *tail, *((fr.ptr(fl),) if flux else ())))
    res = res.view(rows, fr.ncell, nvar) if fr.torch else res
    return SeriesFluxResult(res, ierr, stats, th, fl) if flux else SeriesResult(res, ierr, stats, th)


def cell_atol(mech, var, factor, floor):
    """AbsTol from each cell's own state -> [ncell, 1]: max(floor, factor * max_i |var[c, i]|), NaN entries ignored, a cell with no positive entry
    gets floor.  torch CUDA tensors: the device kernel on torch's current stream (the result feeds rosenbrock_cells without leaving the device);
    numpy arrays: the same formula on the host, bit for bit what the kernel gives."""
    mid, name = _mech_id(mech)
    nvar = DIMS[name][0]
    factor, floor = float(factor), float(floor)
    if _is_torch(var):
        import torch
        if not var.is_cuda or var.dtype != torch.float64 or not var.is_contiguous() or var.shape[-1] != nvar:
            raise MistraChemError("expected a contiguous float64 [ncell,%d] tensor on the GPU" % nvar)
        ncell = var.numel() // nvar
        out = torch.empty((ncell, 1), dtype=torch.float64, device=var.device)
        stream = torch.cuda.current_stream(var.device).cuda_stream
        args = (mid, ncell, var.data_ptr(), factor, floor, out.data_ptr(), C.c_void_p(stream))
        init(var.device.index or 0)
        _check(lib().mistra_chem_cell_atol_device(*args))
        return out
    for x, what in ((factor, "factor"), (floor, "floor")):
        if not (np.isfinite(x) and x > 0.0):
            raise MistraChemError("cell_atol: %s must be finite and positive" % what)
    v = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
    with np.errstate(invalid="ignore", over="ignore"):
        m = factor * np.fmax.reduce(np.abs(v), axis=1)
    return np.where(m > floor, m, floor).reshape(-1, 1)


# ---- OPT-IN: every layer's step size carried from one column step to the next (include/mistra_chem.h: mistra_chem_set_step_reuse)
def set_step_reuse(mech, on=True):
    """Step reuse of drive_host for `mech`: each layer starts at the last accepted step size of its previous column step of this mechanism instead
    of INTEGRATE_x's 1e-3.  Host state: works before init and without a GPU.  Switching forgets the memory."""
    _check(lib().mistra_chem_set_step_reuse(_mech_id(mech)[0], int(bool(on))))


def get_step_reuse(mech):
    return bool(lib().mistra_chem_get_step_reuse(_mech_id(mech)[0]))


def get_step_memory(mech, n):
    """-> the step memory of `mech`, float64 [n]: per model layer k = 1..n the step size its next column step starts at, 0 = none."""
    if _inited_device is None:
        init(0)
    h = np.zeros(int(n))
    _check(lib().mistra_chem_get_step_memory(_mech_id(mech)[0], int(n), h.ctypes.data_as(_dp)))
    return h


def set_step_memory(mech, h):
    """Puts a saved step memory back (a restart): h [n], one entry per model layer, 0 = none.  Call it after set_step_reuse(mech, True)."""
    if _inited_device is None:
        init(0)
    a = np.ascontiguousarray(h, np.float64)
    if a.ndim != 1:
        raise MistraChemError("the step memory is one entry per model layer")
    _check(lib().mistra_chem_set_step_memory(_mech_id(mech)[0], a.size, a.ctypes.data_as(_dp)))


def debug_set_max_steps(n=0):
    """Test hook: Max_no_steps of the integrator (0 = the reference's 100000); makes IERR = -6 reachable (include/mistra_chem.h)."""
    _check(lib().mistra_chem_debug_set_max_steps(int(n)))


# ---- the operators: KPP's building blocks at a state the caller gives (include/mistra_chem.h: mistra_chem_ops_ex / _device)
OPS_MAX_RHS = 256      # MISTRA_OPS_MAX_RHS
OpsResult = namedtuple("OpsResult", "vdot jvs x ising")


def jac_pattern(mech):
    """-> (crow [NVAR+1], icol [LU_NONZERO], diag [NVAR]), KPP's LU_CROW, LU_ICOL and LU_DIAG, 1-based: slot k of jvs is entry (row with
    crow[row-1] <= k+1 < crow[row], icol[k]) of the Jacobian.  Needs no device."""
    mid, name = _mech_id(mech)
    L = lib()
    if mid >= 3:      # (a user slot: refused by the library with the slot's text)
        _check(L.mistra_chem_jac_pattern(mid, None, None, None))
    nvar, _, _, nnz = DIMS[name]
    crow, icol, diag = np.zeros(nvar + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nvar, np.int32)
    _check(L.mistra_chem_jac_pattern(mid, crow.ctypes.data_as(_ip), icol.ctypes.data_as(_ip), diag.ctypes.data_as(_ip)))
    return crow, icol, diag


def ops(mech, var, fix, rconst, want_vdot=True, want_jvs=False, shift=None, rhs=None, fun_rhs=False, vdot=None, jvs=None, x=None, ising=None):
    """Fun_x, Jac_SP_x and solves with A = shift*I - J at the state given, per cell, without integrating -> OpsResult(vdot, jvs, x, ising); what is
    not asked for is None.
      want_vdot   vdot [ncell, NVAR] = Fun_x
      want_jvs    jvs [ncell, LU_NONZERO] = Jac_SP_x in KPP's slot order (jac_pattern), fill-in slots +0.0
      shift       set: the solve.  A number or one entry (shared by all cells), or [ncell].  x [fun_rhs + nrhs, ncell, NVAR]: the cell's own vdot as
                  right-hand side (fun_rhs: row 0), then the rows of rhs [nrhs, ncell, NVAR] ([ncell, NVAR]: one row).  ising [ncell]: KppDecomp_x's IER,
                  the first row (1-based) whose diagonal of A is exactly zero, else 0; such a cell's rows of x are +0.0.
    numpy arrays go to the host entry, torch CUDA tensors to the device entry on the current stream (shift then a tensor of 1 or ncell entries, or a
    number).  vdot, jvs, x, ising: the caller's own output arrays (contiguous, at least the size named above; the call writes the leading part and
    nothing else).  Not for a user mechanism slot."""
    mid, name = _mech_id(mech)
    nvar, nfix, nreact, nnz = DIMS[name]
    L = lib()
    solve = shift is not None
    tt = _is_torch(var)
    if tt:
        import torch
        if not var.is_cuda:
            raise MistraChemError("torch tensors must live on the GPU (there is no CPU path); pass numpy arrays for host data")
        for a, n in ((var, nvar), (fix, nfix), (rconst, nreact)):
            if a.dtype != torch.float64 or not a.is_contiguous() or a.shape[-1] != n or a.device != var.device:
                raise MistraChemError("expected contiguous float64 [ncell,%d] tensors on one device" % n)
        ncell = var.numel() // nvar
        if fix.numel() != ncell * nfix or rconst.numel() != ncell * nreact:
            raise MistraChemError("cell counts of var / fix / rconst differ")
    else:
        var = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
        ncell = var.shape[0]
        fix = np.ascontiguousarray(fix, np.float64).reshape(ncell, nfix)
        rconst = np.ascontiguousarray(rconst, np.float64).reshape(ncell, nreact)

    def own(a, dtype, what):      # a caller's input / output array as it stands
        if tt:
            if not _is_torch(a) or a.dtype != dtype or not a.is_contiguous() or a.device != var.device:
                raise MistraChemError("%s: a contiguous %s tensor on the cells' device expected" % (what, dtype))
        elif not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
            raise MistraChemError("%s: a C-contiguous numpy array of %s expected" % (what, np.dtype(dtype).name))
        return a

    f64, i32 = (torch.float64, torch.int32) if tt else (np.float64, np.int32)

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=var.device) if tt else np.zeros(shape, dtype)

    def size(a):
        return a.numel() if tt else a.size

    def out_array(given, want, shape, dtype, what):
        if not want:
            return None, None
        if given is None:
            a = new(shape, dtype)
            return a, a
        a = own(given, dtype, what)
        n = int(np.prod(shape))
        if size(a) < n:
            raise MistraChemError("%s: at least %d entries expected" % (what, n))
        return a, a.reshape(-1)[:n].reshape(shape)

    nrhs = 0
    if solve and rhs is not None:
        rhs = own(rhs if tt else np.ascontiguousarray(rhs, np.float64), f64, "rhs")
        if size(rhs) % (ncell * nvar if ncell else 1) or (ncell == 0 and size(rhs)):
            raise MistraChemError("rhs: [nrhs, ncell, NVAR] expected")
        nrhs = size(rhs) // (ncell * nvar) if ncell else 0
    nrow = (1 if fun_rhs else 0) + nrhs
    if solve:
        if not tt:
            shift = np.ascontiguousarray(shift, np.float64).reshape(-1)
        elif not _is_torch(shift):
            shift = torch.tensor([float(shift)], dtype=torch.float64, device=var.device)
        else:
            shift = own(shift.reshape(-1), f64, "shift")
        nshift = size(shift)
    else:
        nshift = 1
    vd_a, vd = out_array(vdot, want_vdot, (ncell, nvar), f64, "vdot")
    jv_a, jv = out_array(jvs, want_jvs, (ncell, nnz), f64, "jvs")
    # (a solve without a right-hand side is the library's to refuse: the array still has to exist)
    x_a, xv = out_array(x, solve, (max(nrow, 0), ncell, nvar), f64, "x")
    is_a, isv = out_array(ising, solve, (ncell,), i32, "ising")
    if solve and x_a is not None and size(x_a) == 0:
        x_a = new((1,), f64)
    if solve and size(is_a) == 0:
        is_a = new((1,), i32)
    if tt:
        init(var.device.index or 0)
        _check(L.mistra_chem_ops_device(mid, ncell, _p(var), _p(fix), _p(rconst), _p(vd_a), _p(jv_a), int(nshift), _p(shift) if solve else None,
                                        1 if fun_rhs else 0, int(nrhs), _p(rhs) if nrhs else None, _p(x_a), _p(is_a), _stream(var)))
    else:
        def hp(a, t=_dp):
            return None if a is None else a.ctypes.data_as(t)
        # (the arguments are checked by the library before it looks for a device: no init() in front of them)
        _check(L.mistra_chem_ops_ex(mid, ncell, hp(var), hp(fix), hp(rconst), hp(vd_a), hp(jv_a), int(nshift), hp(shift) if solve else None,
                                    1 if fun_rhs else 0, int(nrhs), hp(rhs) if nrhs else None, hp(x_a), hp(is_a, _ip)))
    return OpsResult(vd, jv, xv, isv)


def fun(mech, var, fix, rconst):
    """Fun_x per cell -> vdot [ncell, NVAR]"""
    return ops(mech, var, fix, rconst, True, False).vdot


def jac_sp(mech, var, fix, rconst):
    """Jac_SP_x per cell -> jvs [ncell, LU_NONZERO] in KPP's slot order (jac_pattern)"""
    return ops(mech, var, fix, rconst, False, True).jvs


def linsolve(mech, var, fix, rconst, shift, rhs=None, fun_rhs=False):
    """(shift*I - J) x = b per cell, J = Jac_SP_x at the state given; b: the cell's own Fun_x (fun_rhs), then the rows of rhs -> (x, ising)"""
    r = ops(mech, var, fix, rconst, False, False, shift=shift, rhs=rhs, fun_rhs=fun_rhs)
    return r.x, r.ising


# ---- the replay (include/mistra_chem.h: mistra_chem_rosenbrock_replay_ex / _device and their cells forms)
def accepted_steps(trace_d, trace_i, ntrace):
    """The accepted steps of a step-control trace as a replay's table: trace_d [ncell, cap, 4], trace_i [ncell, cap, 2] and ntrace [ncell] as the trace
    entries fill them (numpy arrays) -> (hsteps [ncell, cap], nsteps [ncell] int32): per cell the H of the records whose code has bit 0 set, in order,
    padded with zeros.  Records past the log's capacity were never written: a cell whose ntrace exceeds it is refused, its sequence is not whole."""
    td, ti = np.asarray(trace_d, np.float64), np.asarray(trace_i, np.int32)
    nt = np.atleast_1d(np.asarray(ntrace, np.int64))
    if td.ndim != 3 or td.shape[2] != 4 or ti.shape != td.shape[:2] + (2,) or nt.shape != td.shape[:1]:
        raise MistraChemError("accepted_steps: trace_d [ncell, cap, 4], trace_i [ncell, cap, 2] and ntrace [ncell] expected")
    ncell, cap = td.shape[:2]
    hsteps, nsteps = np.zeros((ncell, cap)), np.zeros(ncell, np.int32)
    for c in range(ncell):
        if nt[c] > cap:
            raise MistraChemError("accepted_steps: cell %d made %d attempts, the log holds %d: trace it again with a larger cap" % (c, nt[c], cap))
        h = td[c, :nt[c], 1][(ti[c, :nt[c], 1] & 1) == 1]
        hsteps[c, :h.size] = h
        nsteps[c] = h.size
    return hsteps, nsteps


def _ros_replay(mech, var, fix, rconst, tstart, tend, hsteps, nsteps, ipar, rpar, atol, rtol, err_log, cells):
    mid, name = _mech_id(mech)
    opts = _options(name, cells, ipar, rpar, atol, rtol)
    L = lib()
    if not hasattr(L, "mistra_chem_rosenbrock_replay_ex"):
        raise MistraChemError("this build of the library has no replay entries")
    fr = _front(name, var, fix, rconst, None)
    ncell, torch = fr.ncell, fr.torch
    # the table: hp, npt as the entry takes them
    if torch:
        if _is_torch(hsteps) != _is_torch(nsteps):
            raise MistraChemError("hsteps and nsteps: both numpy arrays (one shared sequence) or both tensors on the cells' device (a row per cell)")
        if _is_torch(hsteps):      # rows per cell, read by the kernel in stream order
            if hsteps.dtype != torch.float64 or not hsteps.is_contiguous() or hsteps.ndim != 2 or hsteps.device != fr.device:
                raise MistraChemError("hsteps: a contiguous float64 [ncell, cap] tensor on the cells' device expected")
            if nsteps.dtype != torch.int32 or not nsteps.is_contiguous() or nsteps.ndim != 1 or nsteps.device != fr.device:
                raise MistraChemError("nsteps: a contiguous int32 [ncell] tensor on the cells' device expected")
            hrows, cap = int(hsteps.shape[0]), int(hsteps.shape[1])
            if nsteps.numel() != hrows:
                raise MistraChemError("hsteps has %d rows, nsteps %d entries" % (hrows, nsteps.numel()))
            if hrows == 1 and ncell == 1:      # (one cell: the library takes the table as the shared, host form)
                hsteps, nsteps = hsteps.cpu().numpy(), nsteps.cpu().numpy()
    if not _is_torch(hsteps):
        hs = None if hsteps is None else np.ascontiguousarray(hsteps, np.float64)
        if hs is not None and hs.ndim == 1:
            hs = hs.reshape(1, -1)
        ns = None if nsteps is None else np.ascontiguousarray(np.atleast_1d(nsteps), np.int32)
        if (hs is not None and hs.ndim != 2) or (ns is not None and ns.ndim != 1) or (torch and (hs is None or ns is None)):
            raise MistraChemError("hsteps [hrows, cap] and nsteps [hrows] expected")
        hrows = int(ns.size) if ns is not None else int(hs.shape[0]) if hs is not None else 1
        cap = int(hs.shape[1]) if hs is not None else 0
        if hs is not None and ns is not None and hs.shape[0] != hrows:
            raise MistraChemError("hsteps has %d rows, nsteps %d entries" % (hs.shape[0], hrows))
        if torch and hs is not None and ns is not None and hrows == ncell and ncell > 1:
            # rows per cell (what accepted_steps returns): the device entry reads them on the device, so they go up
            hsteps, nsteps = torch.tensor(hs, device=fr.device), torch.tensor(ns, device=fr.device)
        else:      # one shared row travels with the call; any other row count is the library's to refuse, before it looks at the addresses
            hp = None if hs is None or not (cap or torch) else hs.ctypes.data_as(C.c_void_p)
            npt = None if ns is None else ns.ctypes.data_as(C.c_void_p)
    if _is_torch(hsteps):
        hp, npt = hsteps.data_ptr(), nsteps.data_ptr()
    if err_log is None:
        err_log = fr.new((ncell, cap), zero=True)
    if torch:
        if err_log.dtype != torch.float64 or not err_log.is_contiguous() or err_log.numel() != ncell * cap or err_log.device != fr.device:
            raise MistraChemError("err_log: a contiguous float64 [ncell, cap] tensor on the cells' device expected")
    elif not isinstance(err_log, np.ndarray) or err_log.dtype != np.float64 or not err_log.flags.c_contiguous or err_log.size != ncell * cap:
        raise MistraChemError("err_log: a C-contiguous float64 [ncell, cap] array expected")
    tol = _tol_args(fr, opts, cells, atol, rtol)
    out, ierr, stats, th = fr.results()
    entry = getattr(L, "mistra_chem_rosenbrock_replay_%s%s" % ("cells_" if cells else "", fr.form))
    _check(entry(mid, ncell, *fr.ptrs, float(tstart), float(tend), *tol, cap, hrows, hp, npt, fr.ptr(out), fr.ptr(ierr), fr.ptr(stats), fr.ptr(th),
                 fr.ptr(err_log) if cap else None, *((fr.stream,) if torch else ())))
    return IntegrateResult(out, ierr, stats), th, err_log.reshape(ncell, cap)


def rosenbrock_replay(mech, var, fix, rconst, tstart, tend, hsteps, nsteps, ipar=None, rpar=None, atol=None, rtol=None, err_log=None):
    """Ros3 along a prescribed step sequence, every step accepted (mistra_chem_rosenbrock_replay_ex / _device) -> (IntegrateResult, t_h, err_log
    [ncell, cap]: Rosenbrock_x's Err of every step made).  hsteps [hrows, cap], nsteps [hrows], hrows = 1 (a 1-D hsteps is one row: the sequence shared
    by all cells) or ncell (see accepted_steps).  numpy cell data: the host entry, the table numpy too.  torch CUDA tensors: the device entry on torch's
    current stream; a shared sequence stays numpy (it travels with the call), rows per cell are tensors on the cells' device — a numpy table of rows per cell, as
    accepted_steps returns it, is uploaded first.  Of the options the call
    reads ipar[0], ipar[1], ipar[3] (must be 2, Ros3) and the tolerances; rpar is decoded and ignored.  err_log: the caller's array, entries past a
    cell's count stay as they are.  Replaying the accepted steps of rosenbrock_trace() under its arguments repeats that call bit for bit."""
    return _ros_replay(mech, var, fix, rconst, tstart, tend, hsteps, nsteps, ipar, rpar, atol, rtol, err_log, False)


def rosenbrock_replay_cells(mech, var, fix, rconst, tstart, tend, hsteps, nsteps, ipar, rpar, atol, rtol, err_log=None):
    """rosenbrock_replay() with tolerances per cell as rosenbrock_cells takes them; a cell refused with -5 makes no step, its err_log row is untouched."""
    return _ros_replay(mech, var, fix, rconst, tstart, tend, hsteps, nsteps, ipar, rpar, atol, rtol, err_log, True)


Sensitivities = namedtuple("Sensitivities", "dy var max_err ierr nsteps")


def sensitivity_cells(name, var, fix, rconst, params, eps):
    """The 2P+1 cells of one internal-differentiation launch: cell 0 the base cell, cells 2k+1 / 2k+2 with parameter k at p*(1 + eps) / p*(1 - eps) ->
    (var, fix, rconst [2P+1, .], p [P]).  params: ("var", i) | ("rconst", j) | ("fix", k), 0-based.  A parameter whose value is 0 is refused."""
    nvar, nfix, nreact, _ = DIMS[name]
    base = {"var": np.asarray(var, np.float64).reshape(nvar), "fix": np.asarray(fix, np.float64).reshape(nfix),
            "rconst": np.asarray(rconst, np.float64).reshape(nreact)}
    if not (np.isfinite(eps) and eps > 0.0):
        raise MistraChemError("sensitivities: eps must be finite and positive")
    P = len(params)
    cells = {k: np.repeat(v[None, :], 2 * P + 1, axis=0) for k, v in base.items()}
    p = np.zeros(P)
    for k, par in enumerate(params):
        if len(par) != 2 or par[0] not in base or not 0 <= int(par[1]) < base[par[0]].size:
            raise MistraChemError("sensitivities: parameter %d is %r: (\"var\", i), (\"rconst\", j) or (\"fix\", k) inside the mechanism's sizes expected" % (k, par))
        what, i = par[0], int(par[1])
        p[k] = base[what][i]
        if p[k] == 0.0 or not np.isfinite(p[k]):
            raise MistraChemError("sensitivities: parameter %d, %s[%d], is %r: a relative perturbation needs a finite value other than 0" % (k, what, i, p[k]))
        cells[what][2 * k + 1, i] = p[k] * (1.0 + eps)
        cells[what][2 * k + 2, i] = p[k] * (1.0 - eps)
    return cells["var"], cells["fix"], cells["rconst"], p


def sensitivities(mech, var, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, params, eps=1.0e-6, cap=4096):
    """Internal numerical differentiation of one cell (host arrays): one traced call of the base cell, then ONE replay launch of 2P+1 cells — the base
    cell and p*(1 +- eps) for each parameter — along the traced call's accepted steps, shared -> Sensitivities: dy [P, NVAR] = (y+ - y-) / (2*eps*p),
    var [NVAR] the replayed base state (the traced call's, bit for bit), max_err the largest Err over the perturbed cells' steps (above 1: the frozen
    sequence no longer meets the tolerance for some copy — take a smaller eps), ierr [2P+1] of the replay, nsteps.  params: ("var", i), ("rconst", j),
    ("fix", k), 0-based; a parameter that is 0 is refused.  The traced call's refusals and errors raise: there is no sequence to freeze."""
    mid, name = _mech_id(mech)
    v, f, r, p = sensitivity_cells(name, var, fix, rconst, params, eps)
    res, _, tr = rosenbrock_trace(mech, v[:1], f[:1], r[:1], tstart, tend, ipar=ipar, rpar=rpar, atol=atol, rtol=rtol, cap=cap, ctrl=False)
    if int(res.ierr[0]) != 1:
        raise MistraChemError("sensitivities: the base cell's call returned IERR = %d: no step sequence to freeze" % int(res.ierr[0]))
    td = np.stack([tr.t, tr.h, tr.err, tr.share], axis=-1)
    ti = np.stack([tr.species, tr.code], axis=-1)
    hsteps, nsteps = accepted_steps(td, ti, tr.n)
    rep, _, err = rosenbrock_replay(mech, v, f, r, tstart, tend, hsteps[0], nsteps[:1], ipar=ipar, rpar=rpar, atol=atol, rtol=rtol)
    y = rep.var
    n = int(nsteps[0])
    dy = (y[1::2] - y[2::2]) / (2.0 * eps * p)[:, None]
    max_err = float(np.max(err[1:, :n])) if n and len(params) else 0.0
    return Sensitivities(dy, y[0].copy(), max_err, rep.ierr.copy(), n)


FirstStep = namedtuple("FirstStep", "fcn0 ghimj lu r k1 k2 k3 err h var ierr stats")


def debug_first_step(mech, var, fix, rconst, tin=0.0, tout=10.0, hstart=None):
    """Test hook (include/mistra_chem.h: mistra_chem_debug_first_step_ex): the kernel's dump variant on host arrays -> FirstStep, per cell the
    intermediate results of the first attempt of the first step (Fcn0, Ghimj as prepared, the factors in the kernel's form, 1/U(k,k), K1..K3,
    the error norm, H) and var, ierr, stats of the integration that variant carried to its end.  hstart [ncell]: first step size per cell."""
    mid, name = _mech_id(mech)
    nvar, nfix, nreact, nnz = DIMS[name]
    if _inited_device is None:
        init(0)
    v = np.ascontiguousarray(var, np.float64).reshape(-1, nvar)
    ncell = v.shape[0]
    f = np.ascontiguousarray(fix, np.float64).reshape(ncell, nfix)
    r = np.ascontiguousarray(rconst, np.float64).reshape(ncell, nreact)
    h = None if hstart is None else np.ascontiguousarray(hstart, np.float64).reshape(ncell)
    dump = np.zeros((ncell, 5 * nvar + 2 * nnz + 2))
    out, ierr, stats = np.empty_like(v), np.zeros(ncell, np.int32), np.zeros((ncell, 8), np.int32)
    L = lib()
    L.mistra_chem_debug_first_step_ex.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip, _ip]
    _check(L.mistra_chem_debug_first_step_ex(mid, ncell, v.ctypes.data_as(_dp), f.ctypes.data_as(_dp), r.ctypes.data_as(_dp), float(tin), float(tout),
                                             None if h is None else h.ctypes.data_as(_dp), dump.ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                                             ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip)))
    parts, o = [], 0
    for ln in (nvar, nnz, nnz, nvar, nvar, nvar, nvar, 1, 1):
        parts.append(dump[:, o:o + ln])
        o += ln
    return FirstStep(*parts, out, ierr, stats)


def integrate_into(mech, var, fix, rconst, out, ierr, stats, tin=0.0, tout=10.0, texit_hexit=None, hstart=None):
    """Device path with caller-owned output tensors (no allocation inside the timed region of bench.py).  texit_hexit
    [ncell, 2]: exit time and last step size per cell (what INTEGRATE_x leaves in TIN and STEPMIN).  hstart [ncell]: OPT-IN
    first step size per cell instead of the reference's 1e-3 (include/mistra_chem.h: mistra_chem_integrate_device_hstart)."""
    mid, name = _mech_id(mech)
    return _integrate_torch(mid, name, var, fix, rconst, tin, tout, out, ierr, stats, texit_hexit, hstart)


# ---- the hand-over halves of x_drive on the device (include/mistra_chem.h).  torch CUDA tensors, float64, contiguous,
#      cell-major; everything runs on torch's current stream.
def set_species_maps(mech, gas_m2k, gas_k2m, rad_m2k, rad_k2m):
    """The model's species index maps for one mechanism (module gas_common: gas_m2k_x(1:2,j), gas_k2m_x(j), rad_*; 1-based)."""
    mid, _ = _mech_id(mech)
    if _inited_device is None:
        init(0)
    a = [np.ascontiguousarray(x, np.int32) for x in (gas_m2k, gas_k2m, rad_m2k, rad_k2m)]
    _check(lib().mistra_chem_set_species_maps(mid, len(a[1]), a[0].ctypes.data_as(_ip), a[1].ctypes.data_as(_ip), len(a[3]),
                                              a[2].ctypes.data_as(_ip), a[3].ctypes.data_as(_ip)))


def drive_dims(mech):
    """(j2, j6, nkc, nbgs): dimensions of sl1(j2,nkc,n), sion1(j6,nkc,n) and of bgs(2,nbgs,n)"""
    mid, _ = _mech_id(mech)
    v = [C.c_int32() for _ in range(4)]
    _check(lib().mistra_chem_drive_dims(mid, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pack(mech, s1, s3, sl1, sion1, scal, var, fix):
    """x_drive up to Update_RCONST_x: var, fix (in/out: entries the driver does not set keep their content) from the layer arrays; sl1 / sion1
    are clamped in place where the driver does (aer, tot)."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_pack_device(mid, var.shape[0], _p(s1), _p(s3), _p(sl1), _p(sion1), _p(scal), _p(var), _p(fix), _stream(var)))


def unpack(mech, var, s1, s3, sl1, sion1):
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_unpack_device(mid, var.shape[0], _p(var), _p(s1), _p(s3), _p(sl1), _p(sion1), _stream(var)))


def budgets(mech, var, fix, rconst, dt, bg=None, bgs=None):
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_budgets_device(mid, var.shape[0], _p(var), _p(fix), _p(rconst), float(dt), _p(bg), _p(bgs), _stream(var)))


def rates_env_from_c(mech, var, fix, env):
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_rates_env_from_c_device(mid, var.shape[0], _p(var), _p(fix), _p(env), _stream(var)))


def drive(mech, s1, s3, sl1, sion1, scal, env, var, fix, tin, dt, ierr, stats, texit_hexit=None, bg=None, bgs=None):
    """One x_drive per layer for a batch of layers, device-resident: pack -> rates -> INTEGRATE_x(tin, tin + dt) -> budgets -> hand-over."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_drive_device(mid, var.shape[0], _p(s1), _p(s3), _p(sl1), _p(sion1), _p(scal), _p(env), _p(var), _p(fix), float(tin),
                                          float(dt), _p(ierr), _p(stats), _p(texit_hexit), _p(bg), _p(bgs), _stream(var)))


def drive_host(mech, layer, s1, s3, sl1, sion1, scal, env, tin, dt, bg=None, bg_level=None, bgs=None, want_c=False, begin_only=False):
    """mistra_chem_drive: one x_drive per layer for the layers `layer` (k, 1-based) of the model arrays in HOST memory — numpy float64,
    C-contiguous, s1 [n, j1], s3 [n, j5], sl1 [n, nkc*j2], sion1 [n, nkc*j6], bg [nlev, nrxn, 2], bgs [n, 122, 2], updated in place; scal
    [nlayer, 6], env [nlayer, nenv] per layer of the batch.  -> (ierr, stats, t_h[, c_packed]).  begin_only: mistra_chem_drive_begin — the call returns
    with the work enqueued, the outputs are valid after drive_host_end(mech)."""
    mid, name = _mech_id(mech)
    lay = np.ascontiguousarray(layer, np.int32)
    nl = lay.size
    for a in (s1, s3, sl1, sion1) + ((bg,) if bg is not None else ()) + ((bgs,) if bgs is not None else ()):
        if a.dtype != np.float64 or not a.flags.c_contiguous:
            raise MistraChemError("model arrays must be C-contiguous float64 (they are updated in place)")
    sc, ev = np.ascontiguousarray(scal, np.float64), np.ascontiguousarray(env, np.float64)
    ierr, stats, th = np.zeros(nl, np.int32), np.zeros((nl, 8), np.int32), np.zeros((nl, 3))
    nvar, nfix, _, _ = DIMS[name]
    cp = np.zeros((nl, nvar + nfix)) if want_c else None
    lev = np.ascontiguousarray(bg_level, np.int32) if bg_level is not None else None
    P = lambda a: None if a is None else a.ctypes.data_as(_dp)
    fn = lib().mistra_chem_drive_begin if begin_only else lib().mistra_chem_drive
    _check(fn(mid, nl, lay.ctypes.data_as(_ip), s1.shape[0], P(s1), P(s3), P(sl1), P(sion1), P(sc), P(ev), float(tin), float(dt),
              ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), P(th), P(bg), 0 if bg is None else bg.shape[1],
              None if lev is None else lev.ctypes.data_as(_ip), P(bgs), P(cp)))
    out = (ierr, stats, th, cp) if want_c else (ierr, stats, th)
    return out + ((lay, sc, ev, lev),) if begin_only else out      # (begin_only: the inputs ride along so that they outlive the call)


def drive_host_end(mech):
    """mistra_chem_drive_end: waits for the step drive_host(..., begin_only=True) issued for this mechanism and scatters its results."""
    _check(lib().mistra_chem_drive_end(_mech_id(mech)[0]))


def fast_k_mt(mech, ff, rq, kw, ka, ifeed, nkc_l, cw, cm, freep, alpha, vmean, xkmt, t=None, p=None, vt=None):
    """fast_k_mt_a (aer) / fast_k_mt_t (tot) for a batch of layers: xkmt [nlayer, nkc, NSPEC] and, when given, the sedimentation velocity
    vt [nlayer, nkc] (needs t, p [nlayer]) updated in place (include/mistra_chem.h)."""
    mid, _ = _mech_id(mech)
    kwa = np.ascontiguousarray(kw, np.int32)
    _check(lib().mistra_chem_fast_k_mt_device(mid, xkmt.shape[0], _p(ff), _p(rq), kwa.ctypes.data_as(_ip), int(kwa.size), int(ka), int(ifeed), int(nkc_l),
                                              _p(cw), _p(cm), _p(freep), _p(alpha), _p(vmean), _p(xkmt), _p(t), _p(p), _p(vt), _stream(xkmt)))


def henry(mech, tt, out):
    """henry_a (aer) / henry_t (tot) for a batch of layers: out [nlayer, NSPEC] <- tt [nlayer] (include/mistra_chem.h)."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_henry_device(mid, out.shape[0], _p(tt), _p(out), _stream(out)))


def v_mean(mech, tt, out):
    """v_mean_a (aer) / v_mean_t (tot) for a batch of layers: out [nlayer, NSPEC] <- tt [nlayer] (include/mistra_chem.h)."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_v_mean_device(mid, out.shape[0], _p(tt), _p(out), _stream(out)))


def dry_rates(tt, freep, rcd, vmean4=None, henry4=None):
    """dry_rates_a / dry_rates_t (vmean4 [nlayer, 4] given) or dry_rates_g (henry4 [nlayer, 4] given, returned updated) for a batch of layers
    -> xkmtd [nlayer, 2, 4], xeq [nlayer] (, henry4); numpy arrays (host-buffer entry, include/mistra_chem.h)."""
    L = lib()
    if not hasattr(L, "_dry_rates_typed"):
        L.mistra_chem_dry_rates.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        L._dry_rates_typed = True
    gas = vmean4 is None
    f8 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    tt, freep, rcd, vmean4 = f8(tt), f8(freep), f8(rcd), f8(vmean4)
    h = None if henry4 is None else np.array(henry4, np.float64, order="C", copy=True)
    nl = tt.shape[0]
    xk, xeq = np.full((nl, 2, 4), np.nan), np.full(nl, np.nan)
    P = lambda a: None if a is None else a.ctypes.data_as(_dp)
    _check(L.mistra_chem_dry_rates(int(gas), nl, P(tt), P(freep), P(rcd), P(vmean4), P(xk), P(xeq), P(h)))
    return (xk, xeq, h) if gas else (xk, xeq)


def pin_host(a):
    """Registers the memory of a C-contiguous numpy array for direct transfers by the host-buffer entries (include/mistra_chem.h: mistra_chem_pin_host).
    The array must stay alive, and must not be resized, until unpin_host(a)."""
    assert a.flags["C_CONTIGUOUS"]
    L = lib()
    L.mistra_chem_pin_host.argtypes = [C.c_void_p, C.c_size_t]
    _check(L.mistra_chem_pin_host(a.ctypes.data, a.nbytes))


def unpin_host(a):
    L = lib()
    L.mistra_chem_unpin_host.argtypes = [C.c_void_p]
    _check(L.mistra_chem_unpin_host(a.ctypes.data))


def cw_rc(ff, rq, e, kw, ka, ifeed, feu=None, cloud=None, crys4=None, dry=False):
    """cw_rc (dry=False: -> rc, cw, cm, conv2 [nlayer, 4], below [nlayer]) or dry_cw_rc (dry=True: -> rcd, cwd [nlayer, 2]) for a batch of layers;
    numpy arrays in and out (host-buffer entry, include/mistra_chem.h)."""
    L = lib()
    if not hasattr(L, "_cw_rc_typed"):
        L.mistra_chem_cw_rc.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, C.c_int, C.c_int, _dp, _ip, _dp, _dp, _dp, _dp, _dp, _ip]
        L._cw_rc_typed = True
    ff = np.ascontiguousarray(ff, np.float64)
    nl, nka, nkt = ff.shape
    nb = 2 if dry else 4
    f8 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    rq, e, feu, crys4 = f8(rq), f8(e), f8(feu), f8(crys4)
    kw = np.ascontiguousarray(kw, np.int32)
    cl = None if cloud is None else np.ascontiguousarray(cloud, np.int32)
    rc, cw, cm, cv = (np.full((nl, nb), np.nan) for _ in range(4))
    below = np.full(nl, -1, np.int32)
    P = lambda a, t=_dp: None if a is None else a.ctypes.data_as(t)
    _check(L.mistra_chem_cw_rc(nl, nkt, nka, int(bool(dry)), P(ff), P(rq), P(e), P(kw, _ip), int(ka), int(ifeed), P(feu), P(cl, _ip), P(crys4), P(rc), P(cw),
                               P(cm), P(cv), P(below, _ip)))
    return (rc, cw) if dry else (rc, cw, cm, cv, below)


def st_coeff(mech, env, out, lp_joyce14bc=False, lp_buxmann15alph=False):
    """st_coeff_a (aer) / st_coeff_t (tot) for a batch of layers: out [nlayer, NSPEC] <- env [nlayer, 5] = t, cw(1), cm(1), sion1(13,1), sion1(14,1)
    (include/mistra_chem.h)."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_st_coeff_device(mid, out.shape[0], int(bool(lp_joyce14bc)), int(bool(lp_buxmann15alph)), _p(env), _p(out), _stream(out)))


def equil_co(mech, tt, conv2, xgamma, xkef, xkeb):
    """equil_co_a (aer) / equil_co_t (tot) for a batch of layers: xkef, xkeb [nlayer, nkc, NSPEC] updated in place from tt [nlayer],
    conv2 [nlayer, nkc], xgamma [nlayer, nkc, j6] (include/mistra_chem.h)."""
    mid, _ = _mech_id(mech)
    _check(lib().mistra_chem_equil_co_device(mid, xkef.shape[0], xkef.shape[1], xgamma.shape[2], _p(tt), _p(conv2), _p(xgamma), _p(xkef), _p(xkeb), _stream(xkef)))
