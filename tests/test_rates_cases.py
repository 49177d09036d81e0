"""The edge cases of tests/rates_cases.py on the CPU: (a) the restated rate laws (oracle/rates_py.py) against what the COMPILED REFERENCE made of the same
vectors (tests/golden/rates_edges_<mech>.npz, tests/golden/make_rates_edges_golden.py), bit for bit; (b) the edge table: every guard, clamp and
threshold is reached by a case of every mechanism that calls the law, counted inside the wrapped laws; (c) every program fits the evaluator's operand
stack; (d) the bound of the toleranced device comparison follows the restatement's own movement (tests/parity_bounds.py, section G).  The same cases
run on the device in tests/test_gpu_rates_edges.py."""
import json
import math
import os
import re

import numpy as np
import pytest

import liq_cases
import parity_bounds as pb
import rates_cases as rc
from conftest import REPO
from oracle import rates_py


@pytest.mark.parametrize("mech", rc.MECHS)
def test_cases_are_the_fixtures_inputs_and_few(mech):
    c, fx = rc.cases(mech), rc.fixture(mech)
    assert len(c["names"]) <= rc.MAX_CASES
    assert list(fx["names"]) == c["names"]
    assert rc.same_bits(fx["env"], c["env"]), "tests/golden/rates_edges_%s.npz was made from other cases: run tests/golden/make_rates_edges_golden.py" % mech
    path = os.path.join(rc.GOLD, "rates_edges_%s.npz" % mech)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(rc.GOLD, "rates_%s.npz" % mech))
    # a case differs from its ordinary vector in exactly the entries it names
    _, slot, _ = rc.env_info(mech)
    base = rc.ordinary(mech)
    for i, over in enumerate(c["over"]):
        diff = {int(k) for k in np.nonzero(~((c["env"][i] == base[c["base"][i]]) & (np.signbit(c["env"][i]) == np.signbit(base[c["base"][i]]))))[0]}
        assert diff <= {slot[n] for n in over}, c["names"][i]
    assert np.isfinite(base).all() and not (base[:, [i for i, n in enumerate(rc.env_info(mech)[0]) if not n.startswith("xhet")]] == 0.0).any()


@pytest.mark.parametrize("mech", rc.MECHS)
def test_restated_rate_laws_equal_the_compiled_reference_on_every_edge(mech):
    """(a) bit for bit, the sign of every zero included, NaN in the same places.  This is where MAX's treatment of a NaN was learnt: the compiled
    reference returns NaN for max(0.d0, NaN) (fdhet*) and 0 for max(NaN, 0.d0) (uplim, uplip)."""
    got, want = rc.restated(mech), rc.fixture(mech)["rconst"]
    for i, name in enumerate(rc.cases(mech)["names"]):
        assert rc.same_bits(got[i], want[i]), "%s, case %r: reactions %s" % (
            mech, name, np.nonzero(~((got[i] == want[i]) | (np.isnan(got[i]) & np.isnan(want[i]))))[0][:8].tolist())
    assert np.isnan(want).any() and (want == 0.0).any()


@pytest.mark.parametrize("mech", rc.MECHS)
def test_every_edge_is_reached(mech):
    """(b) the edge table.  A case that stops reaching its edge — a redrawn fixture row, a regenerated table — fails here by name."""
    reach = rc.reach(mech)
    edges = rc.applicable(mech) + list(rc.VECTOR_EDGES)
    print("%s: %d cases, %d edges" % (mech, len(rc.cases(mech)["names"]), len(edges)))      # (pytest -s shows the table)
    for e in edges:
        print("  %-84s %2d case(s): %s" % (e, len(reach[e]), ", ".join(reach[e][:3]) + (" ..." if len(reach[e]) > 3 else "")))
    missed = [e for e in edges if not reach[e]]
    assert not missed, "%s: no case reaches %s" % (mech, missed)
    # the edges a mechanism cannot have are exactly those of laws it does not call
    assert {e for e in rc.EDGES if e not in edges} == {e for e, (ls, _) in rc.EDGES.items() if not rc.laws(mech) & set(ls)}
    # an edge with a vector of its own is reached by that vector (the rest of it is ordinary: a failure names the edge)
    own = {"fbck2 ck = 0": "fbck2 ck=0", "flsc6 b = 1e-15": "flsc6 b=1e-15", "flsc6 b = 1e-15 + 1 ulp": "flsc6 b=1e-15+ulp", "fdhet yhenry = 0": "fdhet yhenry=0",
           "fdhet C(HNO3) = 0": "fdhet C(HNO3)=0", "fdhet yxeq + 1e-2 = 0": "fdhet yxeq=-1e-2", "te = 180 K": "te=180", "te = 330 K": "te=330"}
    for e, case in own.items():
        if e in edges:
            assert case in reach[e], (e, reach[e])
    # on how many vectors the clamped laws are evaluated with a live guard (the issue's open count): every case whose cvv* are positive
    for law in ("uplim", "uplip", "uparp"):
        if law in rc.laws(mech):
            assert len(reach["%s guard > 0, result non-zero" % law]) >= len(rc.cases(mech)["names"]) // 2


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_what_the_tables_put_out_of_an_inputs_reach(mech):
    """dmin2's and dmin3's arguments are literals (rates_cases' docstring): both sides of dmin2's threshold and the threshold itself are among them, dmin3's
    are all above 2e10.  Every other guarded argument is a bare input."""
    f = rc.feeds(mech)
    assert ("dmin2", 0) not in f and ("dmin3", 0) not in f
    lit = {"dmin2": set(), "dmin3": set()}
    for prog in rc.table(mech)["programs"]:
        for i, t in enumerate(prog):
            if t[0] == "call" and t[1] in lit:
                assert prog[i - 1][0] == "num"
                lit[t[1]].add(float(prog[i - 1][1]))
    assert min(lit["dmin2"]) < 1.0e10 < max(lit["dmin2"]) and 1.0e10 in lit["dmin2"]
    assert min(lit["dmin3"]) == 4.0e10 > 2.0e10
    nb = 2 if mech == "aer" else 4
    for law, gi in list(rc._GUARDED.items()) + [("uparm", 4)]:
        assert f[(law, gi)] == tuple("cvv%d" % k for k in range(1, nb + 1)), (law, f.get((law, gi)))
    assert f[("uplim", 2)] == f[("uplip", 1)] == f[("flsc6", 1)] == f[("uparm", 3)] and len(f[("uplim", 2)]) == nb


def test_library_laws_are_the_laws_that_call_the_library():
    """rates_cases.LIBRARY_LAWS, the one list behind "bit for bit" and "to the bound", against a count of the exp / pow / log10 calls each law makes on an
    ordinary vector (every law of every table, the two of st_coeff included)."""
    class Counting(liq_cases.MathShim):
        def __init__(self):
            self.n = 0

        def exp(self, x): self.n += 1; return math.exp(x)
        def pow(self, a, b): self.n += 1; return math.pow(a, b)
        def log10(self, x): self.n += 1; return math.log10(x)
        def log(self, x): self.n += 1; return math.log(x)
        def sqrt(self, x): self.n += 1; return math.sqrt(x)

    seen = {}
    shim = Counting()
    saved = dict(rates_py.FUNCS)

    def wrap(law, fn):
        def w(e, *a):
            before = shim.n
            r = fn(e, *a)
            seen[law] = seen.get(law, 0) + shim.n - before
            return r
        return w
    try:
        rates_py.math = shim
        for law, fn in saved.items():
            rates_py.FUNCS[law] = wrap(law, fn)
        for mech in rc.MECHS:
            rc.evaluate(mech, rc.ordinary(mech)[0])
        for mech in ("aer", "tot"):
            for jo, bu in liq_cases.STC_SWITCHES:
                rates_py.st_coeff_layer(liq_cases.stc_table(mech), jo, bu, liq_cases.stc_cases(mech)[0][0])
    finally:
        rates_py.math = math
        rates_py.FUNCS.clear()
        rates_py.FUNCS.update(saved)
    assert set(seen) == set(saved), set(saved) - set(seen)
    assert {law for law, n in seen.items() if n} == set(rc.LIBRARY_LAWS)
    for mech in rc.MECHS:
        plain, libfree, lib = rc.program_kinds(mech)
        assert plain.sum() > 100 and lib.sum() > 100 and (plain ^ libfree ^ lib).all() and not (plain & lib).any()
    assert rc.program_kinds("gas")[1].sum() >= 8 and rc.program_kinds("aer")[1].sum() >= 80 and rc.program_kinds("tot")[1].sum() >= 160


def test_every_program_fits_the_evaluators_operand_stack():
    """(c) the device evaluator's stack is a fixed column of kRatesStackDepth doubles per thread (mistra_amd/csrc/rates.hpp)."""
    hpp = open(os.path.join(REPO, "mistra_amd", "csrc", "rates.hpp")).read()
    depth = int(re.search(r"constexpr int kRatesStackDepth = (\d+);", hpp).group(1))
    assert depth == rc.STACK_DEPTH
    assert "stack_cells[kRatesStackDepth][256]" in open(os.path.join(REPO, "mistra_amd", "csrc", "rates.hip")).read()
    found = {}
    for mech in rc.MECHS:
        found[mech + ".rates"] = rc.stack_depth(rc.table(mech)["programs"])
    for mech in ("aer", "tot"):
        tab = json.load(open(os.path.join(REPO, "mistra_amd", "mech", mech + ".stcoeff.json")))
        found[mech + ".stcoeff"] = max(rc.stack_depth(v["programs"]) for v in tab["variants"])
    print("deepest operand stack:", found)
    assert all(0 < d <= depth for d in found.values()), found
    assert max(found.values()) == 8 and found["tot.rates"] == 7      # what the header's comment says of the shipped tables


def test_bound_of_the_device_comparison_follows_the_restatements_own_movement():
    """(d) tests/parity_bounds.py, section G: RATES_EDGES_RTOL = max(RATES_EDGES_FLOOR, 10 x the spread measured here)."""
    for mech in rc.MECHS:
        s, n = rc.spread(mech)
        print("%s: %d entries of library programs move by at most %.3e under last-place freedom of exp / pow / log10" % (mech, n, s))
        assert n > 1000
        pb.check_constant("RATES_EDGES_RTOL[%s]" % mech, pb.RATES_EDGES_RTOL[mech], s, floor=pb.RATES_EDGES_FLOOR)
        # no entry's movement is unbounded by cancellation: nothing is left to a looser comparison (the issue allows up to 2 % such entries; there are none)
        assert 10.0 * s <= pb.RATES_EDGES_RTOL[mech]
