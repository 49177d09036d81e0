"""TEST INFRASTRUCTURE — a series of Rosenbrock_x calls with the reaction flux of every leg (mistra_chem_rosenbrock_series_flux_ex)
restated on the CPU: tests/ros_series_rates_py.py's chain (chain_rates) driven with tests/ros_flux_py.py's restatement of Rosenbrock_x with the flux as
the call.  No numerics of its own: leg k's flux row is what that call returns for the leg, nothing is carried from one leg's sum into the next.

The sets and the ramp are tests/ros_series_rates_py.py's (SET_NAMES, ramp, series_set, leg_rows): the integration's parity with the compiled reference
is carried by that module's fixture, and the flux is defined by an entry that exists."""
import numpy as np

import ros_flux_py as RF
import ros_series_rates_py as SR
from ros_series_rates_py import FAILING_SETS, MECHS, SET_NAMES, TIMES, leg_rows, ramp, series_set  # noqa: F401


def chain_flux(o, diag, var, s, fix_legs, k_legs):
    """One cell through the legs of `s` with the leg's rows (fix_legs / k_legs: [nleg, .] of the cell, or [.] shared)
    -> (VAR [nleg, NVAR], IERR [nleg], IPAR(11:18) [nleg, 8], Texit [nleg], Hexit [nleg], flux [nleg, NREACT], leg start states [nleg, NVAR],
        RPAR of every leg [nleg, 20])"""
    flux, start, rpars = [], [], []

    def call(y, f, k, rpar, t0, t1):
        r = RF.rosenbrock(o, diag, y, f, k, s.ipar, rpar, s.atol, s.rtol, t0, t1)
        flux.append(np.array(r[5]))
        start.append(np.array(y))
        rpars.append(np.array(rpar, np.float64))
        return r[:5]
    out = SR.chain_rates(call, var, s, fix_legs, k_legs)
    return out + (np.array(flux), np.array(start), np.array(rpars))


_restated = {}


def restated(mech, names=SET_NAMES):
    """{set name: (VAR [nleg, 3, NVAR], IERR [nleg, 3], IPAR(11:18) [nleg, 3, 8], Texit [nleg, 3], Hexit [nleg, 3], flux [nleg, 3, NREACT],
    leg start states [nleg, 3, NVAR], RPAR of every leg [nleg, 3, 20])} of the chained restatement on the ramp; computed once per (mechanism, set) and
    shared by the tests"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o = diag = rows = None
    out = {}
    for name in names:
        key = (mech, name)
        if key not in _restated:
            if o is None:
                o, diag, rows = Oracle(mech), mechtab.load(mech).diag, ramp(mech)
            V, LF, LK = rows
            s, _, _ = series_set(mech, name)
            F, K = leg_rows(name, mech, LF, LK)
            cells = [chain_flux(o, diag, V[c], s, F[:, c] if F.ndim == 3 else F[c], K[:, c] if K.ndim == 3 else K[c]) for c in range(V.shape[0])]
            _restated[key] = tuple(np.stack([cell[i] for cell in cells], axis=1) for i in range(8))
        out[name] = _restated[key]
    return out
