"""Every slot of the kernel table on the GPU (-m gpu), each as the FIRST user of its own configuration flag (capi.cpp: MechDesc::unit,
DeviceState::lds_configured).  What the entries compute is held by their own modules at larger sizes; this one is aimed at a wrong slot or a shared
flag: a kernel whose dynamic LDS was never configured fails its launch (tot: far above the 64 KiB default), a slot that points at another kernel gives
other bits.  Two cells per launch (one workgroup per cell, block index above 0 covered), 16 launches per mechanism, one process."""
import numpy as np
import pytest

import ros_methods_py as RM
from conftest import MECHS, load_golden

pytestmark = pytest.mark.gpu
METHODS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def chem():
    """a library initialised anew: no kernel of any mechanism is configured yet"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.finalize()
    c.init(0)
    return c


def _np(res, leg=None):
    """(var, ierr, stats) of a result's tensors as numpy arrays, after a synchronisation; leg: that leg of a series"""
    import torch
    torch.cuda.synchronize()
    out = tuple(x.cpu().numpy() for x in (res.var, res.ierr, res.stats))
    return out if leg is None else tuple(x[leg] for x in out)


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, got[1].tolist(), want[1].tolist(), got[2].tolist(), want[2].tolist())
    assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), what


@pytest.mark.parametrize("mech", MECHS)
def test_every_slot_as_the_first_user_of_its_flag(chem, mech):
    """flux (VARIANT 6) of methods 1 .. 5, then a one-leg series (5) of each, then the plain call (3; Ros3: the product unit's options kernel) of each,
    then the trace (4, Ros3): every call returns with IERR 1 in both cells, and VAR, IERR and the statistics of the flux call, the series leg and the
    trace call are the plain call's of that method, byte for byte"""
    import torch
    g = load_golden(mech)
    dev = torch.device("cuda", 0)
    V, F, K = (torch.tensor(np.ascontiguousarray(g[k][:2]), device=dev) for k in ("var_in", "fix", "rconst"))
    sets = {m: RM.method_set(mech, "m%d" % m)[:4] for m in METHODS}
    flux = {m: _np(chem.rosenbrock_flux(mech, V, F, K, 0.0, 10.0, *sets[m])[0]) for m in METHODS}
    series = {m: _np(chem.rosenbrock_series(mech, V, F, K, [0.0, 10.0], *sets[m]), leg=0) for m in METHODS}
    plain = {m: _np(chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *sets[m])[0]) for m in METHODS}
    trace = _np(chem.rosenbrock_trace(mech, V, F, K, 0.0, 10.0, *sets[2])[0])
    for m in METHODS:
        assert plain[m][0].shape == (2, V.shape[1]) and np.isfinite(plain[m][0]).all(), m
        for what, got in (("plain", plain[m]), ("flux", flux[m]), ("series", series[m])) + ((("trace", trace),) if m == 2 else ()):
            assert (got[1] == 1).all(), (what, m, got[1].tolist())
            _same(got, plain[m], (what, m))
    # (the five methods are five kernels: no two give the same state)
    assert len({plain[m][0].tobytes() for m in METHODS}) == len(METHODS)
