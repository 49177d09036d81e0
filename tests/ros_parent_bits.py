"""TEST INFRASTRUCTURE — the calls behind tests/golden/parent_bits_<mech>.npz: the step-control trace and the operators through the host entries on cells
0, n/2, n-1 of integrate_<mech>.npz with INTEGRATE_x's options.  The fixtures hold what the library gave on an MI355X at the commit before the trace units
gained the replay kernel; tests/test_gpu_ros_replay.py holds the library to those bytes (the trace units are compiled with one more kernel in them, and the
host side of these entries — the argument block, the launch tables — changed with it)."""
import numpy as np

import ros_options_py as R
import ros_trace_py as RT

CAP = 256
SHIFT = 1.0 / (1.0e-3 * R.ROS_GAMMA[0])      # ros_PrepareMatrix_x's shift of a first step of INTEGRATE_x


def compute(chem, mech, golden):
    """-> {name: array} of one mechanism, numpy arrays as the host entries fill them"""
    c = list(RT.cells_of(golden["var_in"].shape[0]))
    V, F, K = (np.ascontiguousarray(golden[k][c]) for k in ("var_in", "fix", "rconst"))
    res, th, tr = chem.rosenbrock_trace(mech, V, F, K, R.TIN, R.TOUT, *RT.trace_set(mech, "base"), cap=CAP)
    rhs = np.ascontiguousarray(np.stack([V, V[::-1]]))      # two caller rows per cell: [2, ncell, NVAR]
    ops = chem.ops(mech, V, F, K, want_vdot=True, want_jvs=True, shift=np.array([SHIFT, 2.0 * SHIFT, -SHIFT]), rhs=rhs, fun_rhs=True)
    n = int(np.max(tr.n))
    assert n <= CAP
    return {"trace_var": res.var, "trace_ierr": res.ierr, "trace_stats": res.stats, "trace_th": th, "trace_n": tr.n, "trace_ctrl": tr.ctrl,
            "trace_t": np.ascontiguousarray(tr.t[:, :n]), "trace_h": np.ascontiguousarray(tr.h[:, :n]), "trace_err": np.ascontiguousarray(tr.err[:, :n]),
            "trace_share": np.ascontiguousarray(tr.share[:, :n]), "trace_species": np.ascontiguousarray(tr.species[:, :n]),
            "trace_code": np.ascontiguousarray(tr.code[:, :n]), "ops_vdot": ops.vdot, "ops_jvs": ops.jvs, "ops_x": ops.x, "ops_ising": ops.ising}
