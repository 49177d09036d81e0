"""Edge cases for Update_RCONST_x: input vectors that sit ON the guards of the rate laws (oracle/rates_py.py; the device's are in
mistra_amd/csrc/rates.hip), one edge per vector, and the book-keeping that proves each edge is reached.  The cases of tests/test_rates_cases.py (CPU:
the restatement against the compiled reference's fixture, the edge table, the operand-stack depth, the bound) and of tests/test_gpu_rates_edges.py
(the device evaluator against the same fixture).  Plain module, no GPU; everything is cached and read-only like tests/liq_cases.py.

Every case starts from an ORDINARY vector: a daytime row of tests/golden/rates_<mech>.npz with every switch on (xhal, xiod, xliq*; xhet* = 0) and
every exact zero among the concentrations, water contents and transfer coefficients replaced by the column's first non-zero value, so that the
programs around an edge are non-zero and a wrong branch shows in the result.  A case overrides entries BY NAME (mistra_amd/mech/<mech>.rates_env.json).
Which entry feeds which argument of which law is traced from the programs (feeds): an argument that is a bare `var` / `arr` token.  Every threshold
input is therefore an env entry or a literal of the table, never the result of exp / pow: device and reference take the same branch by construction.

What the tables do NOT let an input reach (feeds() shows the argument is a literal in every program of every mechanism):
  dmin2   its argument is one of eleven literals: 5.5e9 .. 7.7e9 (below 1e10), 1e10 itself (6 of 28 calls in aer, 12 of 56 in tot) and
          1.1e10 .. 1.9e10 (above).  All three sides of the threshold are therefore reached on EVERY vector, and none can be moved by an input.
  dmin3   its argument is the literal 4e10 or 4.4e10: always clipped at 2e10.  The unclipped branch cannot be reached with the shipped tables;
          the nearest reachable case is the smaller literal, 4e10, which every vector evaluates.  (The branch itself is the same comparison as
          dmin2's, whose two sides are both reached.)
tests/test_rates_cases.py holds these statements about the literals, so a regenerated table that changes them fails there."""
import functools
import json
import math
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import rates_py      # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MECHS = ("gas", "aer", "tot")
MAX_CASES = 64
STACK_DEPTH = 12          # mistra_amd/csrc/rates.hpp: kRatesStackDepth (tests/test_rates_cases.py reads the header and holds the two equal)
NBASE = 3                 # ordinary vectors per mechanism; consecutive cases share one (the fixture stays small: rows repeat within deflate's window)

# the rate laws that call exp, pow or log10.  The one list: everything else a table calls is LIBRARY-FREE (comparisons, + - * / only) and is
# compared bit for bit; tests/test_rates_cases.py counts the library calls each law makes and holds this list to that count.
LIBRARY_LAWS = frozenset(("farr", "farr_sp", "atk_3", "atk_3f", "shno3", "fbck", "fbckj", "fbck2", "sp_23", "fcn", "dms_add", "farr2", "fliq_60",
                          "uparm", "uparp", "exp", "a_n2o5"))


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


@functools.lru_cache(maxsize=None)
def table(mech):
    return json.load(open(os.path.join(REPO, "mistra_amd", "mech", mech + ".rates.json")))


@functools.lru_cache(maxsize=None)
def env_info(mech):
    """-> (names, {name: index}, fslot)"""
    ev = json.load(open(os.path.join(REPO, "mistra_amd", "mech", mech + ".rates_env.json")))
    return tuple(ev["env"]), {n: i for i, n in enumerate(ev["env"])}, tuple(ev["fslot"])


def _token_name(t):
    return t[1] if t[0] == "var" else "%s(%s)" % (t[1], ",".join(str(i) for i in t[2:]))


def walk(prog):
    """-> (deepest operand stack of a postfix program, [(law, [env name | None per argument])]): None where the argument is not a bare input"""
    st, deepest, calls = [], 0, []
    for t in prog:
        k = t[0]
        if k == "num":
            st.append(None)
        elif k in ("var", "arr"):
            st.append(_token_name(t))
        elif k == "neg":
            assert st
            st[-1] = None
        elif k == "call":
            n = t[2]
            assert len(st) >= n
            calls.append((t[1], st[len(st) - n:] if n else []))
            del st[len(st) - n:]
            st.append(None)
        else:
            assert k in "+-*/" and len(st) >= 2
            st.pop()
            st[-1] = None
        deepest = max(deepest, len(st))
    assert len(st) == 1
    return deepest, calls


def stack_depth(programs):
    return max(walk(p)[0] for p in programs)


@functools.lru_cache(maxsize=None)
def feeds(mech):
    """{(law, argument index): sorted env names that are that argument somewhere in the mechanism's programs}"""
    out = {}
    for prog in table(mech)["programs"]:
        for law, args in walk(prog)[1]:
            for i, a in enumerate(args):
                if a is not None:
                    out.setdefault((law, i), set()).add(a)
    return {k: tuple(sorted(v)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def laws(mech):
    return frozenset(law for prog in table(mech)["programs"] for law, _ in walk(prog)[1])


def library_free_laws(mech):
    return laws(mech) - LIBRARY_LAWS


@functools.lru_cache(maxsize=None)
def program_kinds(mech):
    """-> (plain [nreact]: no call at all, libfree: calls, all of them library-free, lib: at least one library call)"""
    called = [set(law for law, _ in walk(p)[1]) for p in table(mech)["programs"]]
    plain = np.array([not c for c in called])
    lib = np.array([bool(c & LIBRARY_LAWS) for c in called])
    return _freeze((plain, ~plain & ~lib, lib))


def fs_names(mech, key, count):
    """env names behind `count` consecutive positions of the slot list from FS[key] on (what the laws read from COMMON themselves)"""
    names, _, fslot = env_info(mech)
    return [names[fslot[rates_py.FS[key] + k]] for k in range(count) if fslot[rates_py.FS[key] + k] >= 0]


# ---------------------------------------------------------------------------------------------------------------- the ordinary vectors
@functools.lru_cache(maxsize=None)
def ordinary(mech):
    """[NBASE, nenv]: the first daytime rows of the seeded fixture, switches on, no exact zero among the physical inputs"""
    names, slot, _ = env_info(mech)
    g = np.load(os.path.join(GOLD, "rates_%s.npz" % mech))["env"]
    ph = [i for i, n in enumerate(names) if n.startswith("ph_rat")]
    rows = [k for k in range(g.shape[0]) if g[k, ph].all()][:NBASE]
    assert len(rows) == NBASE
    out = g[rows].copy()
    for i, n in enumerate(names):
        if n.startswith(("xhal", "xiod", "xliq")):
            out[:, i] = 1.0
        elif n.startswith("xhet"):
            out[:, i] = 0.0
        elif (out[:, i] == 0.0).any():
            nz = g[:, i][g[:, i] != 0.0]
            assert len(nz)
            out[out[:, i] == 0.0, i] = nz[0]
    return _freeze(out)


# ---------------------------------------------------------------------------------------------------------------- the cases
NEG_C = -1.0e-12          # a concentration as the integrator hands it back after a small undershoot
NEG_CVV = -1.0e9


def _case_list(mech):
    """[(case name, {env name: value})]"""
    names, slot, fslot = env_info(mech)
    L = laws(mech)
    f = feeds(mech)
    cases = [("ordinary", {})]
    grp = lambda prefix: [n for n in names if re.match(prefix + r"\d*$", n)]
    cvv = grp("cvv")
    for n in cvv:
        cases += [("%s=0" % n, {n: 0.0}), ("%s=-0.0" % n, {n: -0.0}), ("%s<0" % n, {n: NEG_CVV})]
    if cvv:
        cases += [("cvv*=0", {n: 0.0 for n in cvv}), ("cvv*=-0.0", {n: -0.0 for n in cvv}), ("cvv*<0", {n: NEG_CVV for n in cvv})]
    # the concentrations under uplim's max(c,0) and uplip's max(b,0) (the same entries also are uparm's guarded d and flsc6's b)
    clamp = sorted(set(f.get(("uplim", 2), ())) | set(f.get(("uplip", 1), ())))
    assert all(n.startswith("c(") for n in clamp)
    for n in clamp:
        cases += [("%s<0" % n, {n: NEG_C}), ("%s=-0.0" % n, {n: -0.0})]
    ck = f.get(("fbck2", 5), ())
    assert ck == ("conv1",)
    cases += [("fbck2 ck=0", {"conv1": 0.0}), ("fbck2 ck=-0.0", {"conv1": -0.0})]
    b6 = f.get(("flsc6", 1), ())
    if b6:
        cases += [("flsc6 b=1e-15", {n: 1.0e-15 for n in b6}), ("flsc6 b=1e-15+ulp", {n: math.nextafter(1.0e-15, 1.0) for n in b6}),
                  ("flsc6 b=0", {n: 0.0 for n in b6})]
    if L & {"fhet_t", "fhet_da", "fhet_dt"}:
        nb = sum(1 for k in range(4) if fslot[rates_py.FS["H2OL"] + k] >= 0)
        h2ol, clm, brm = fs_names(mech, "H2OL", nb), fs_names(mech, "CLM", nb), fs_names(mech, "BRM", nb)
        ycwd = fs_names(mech, "YCWD", 2)
        xliq, xhet = grp("xliq"), grp("xhet")
        allv = lambda ns, v: {n: v for n in ns}
        cases.append(("hetT: H2OL=CLM=BRM=0", {**allv(h2ol, 0.0), **allv(clm, 0.0), **allv(brm, 0.0)}))
        cases.append(("hetT<0: CLM<0", {**allv(h2ol, 1.0), **allv(clm, -1.0), **allv(brm, 0.0)}))              # 1 - 500 + 0
        cases.append(("hetT=0: CLM<0", {**allv(h2ol, 500.0), **allv(clm, -1.0), **allv(brm, 0.0)}))            # 500 - 500 + 0, exact
        cases.append(("YCWD=0 dry xhal=0", {**allv(ycwd, 0.0), **allv(xhet, 1.0), "xhal": 0.0}))                # dry branch: hetT = 55.55*0*1e3 = 0
        cases.append(("YCWD=0 dry xhal=1", {**allv(ycwd, 0.0), **allv(xhet, 1.0)}))
        for hal in (0.0, 1.0):
            for liq in (0.0, 1.0):
                for het in (0.0, 1.0):
                    cases.append(("xhal=%d xliq=%d xhet=%d" % (hal, liq, het), {"xhal": hal, **allv(xliq, liq), **allv(xhet, het)}))
    else:
        cases.append(("YCWD=0", {n: 0.0 for n in fs_names(mech, "YCWD", 2)}))
    chno3, yh, yxeq = fs_names(mech, "C_HNO3", 1)[0], fs_names(mech, "YHENRY_HNO3", 1)[0], fs_names(mech, "YXEQ_HNO3", 1)[0]
    cases += [("fdhet C(HNO3)=0", {chno3: 0.0}), ("fdhet yhenry=0", {yh: 0.0}), ("fdhet yxeq=-1e-2", {yxeq: -1.0e-2}),
              ("fdhet x1+x2<0", {chno3: 1.0e-14, yh: 1.0, yxeq: 1.0, **{n: 1.0e-7 for n in fs_names(mech, "C_HNO3L", 2)}})]
    cases += [("te=180", {"te": 180.0}), ("te=330", {"te": 330.0}), ("night", {n: 0.0 for n in names if n.startswith("ph_rat")})]
    # a NaN in the concentration under a max(.,0) (aer, tot: uplim / uplip; gas: C(HNO3) under fdhetg's max(0, x1+x2)), +Inf in a transfer coefficient
    cases.append(("NaN in a concentration", {(clamp[0] if clamp else chno3): math.nan}))
    if clamp:
        cases.append(("NaN in C(HNO3)", {chno3: math.nan}))      # ... and under fdhet*'s max(0, x1+x2), where the NaN is MAX's SECOND argument
    cases.append(("+Inf in a yxkmt", {(fs_names(mech, "YXKMT_N2O5", 1) or fs_names(mech, "YXKMTD_HNO3", 1))[0]: math.inf}))
    return cases


@functools.lru_cache(maxsize=None)
def cases(mech):
    """-> dict(names [ncase], env [ncase, nenv], base [ncase]: which ordinary vector, over [ncase]: the overrides)"""
    _, slot, _ = env_info(mech)
    cl = _case_list(mech)
    assert len(cl) <= MAX_CASES and len({n for n, _ in cl}) == len(cl)
    base = ordinary(mech)
    env = np.empty((len(cl), base.shape[1]))
    which = np.empty(len(cl), np.int32)
    for i, (_, over) in enumerate(cl):
        which[i] = i * NBASE // len(cl)
        env[i] = base[which[i]]
        for n, v in over.items():
            env[i, slot[n]] = v
    return _freeze(dict(names=[n for n, _ in cl], env=env, base=which, over=[dict(o) for _, o in cl]))


def fixture(mech):
    return np.load(os.path.join(GOLD, "rates_edges_%s.npz" % mech))


def evaluate(mech, env):
    names, slot, fslot = env_info(mech)
    return rates_py.evaluate(table(mech), slot, env, list(fslot))


@functools.lru_cache(maxsize=None)
def restated(mech):
    """[ncase, nreact] of the restatement with the host libm"""
    return _freeze(np.stack([evaluate(mech, e) for e in cases(mech)["env"]]))


def same_bits(a, b):
    """bit for bit outside NaN (the sign of a zero included), NaN in the same places (a NaN's sign and payload are not part of the comparison)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ---------------------------------------------------------------------------------------------------------------- which case reaches which edge
def _hett(e, a0, dry):
    h2oa = (rates_py.K5555 * e.at("YCWD", a0 - 1)) * 1.0e3 if dry else e.at("H2OL", a0 - 1)
    return (h2oa + 5.0e2 * e.at("CLM", a0 - 1)) + 3.0e5 * e.at("BRM", a0 - 1), h2oa


def _neg0(x):
    return x == 0.0 and math.copysign(1.0, x) < 0.0


def _pos0(x):
    return x == 0.0 and math.copysign(1.0, x) > 0.0


_GUARDED = {"uplim": 3, "uplip": 2, "uparp": 3, "fliq_60": 3, "flsc4": 2, "flsc5": 2}      # law: the argument its `> 0` guard reads (a cvv*)
_FHET_D = ("fhet_da", "fhet_dt")
_FDHET = ("fdhetg", "fdheta", "fdhett")


def _fhet_d_setting(hal, liq, het):
    def pred(e, a, r):
        if (e.at("XHAL") != 0.0) != hal or (a[0] != 0.0) != liq or (a[1] != 0.0) != het:
            return False
        allowed = liq and (hal or (int(a[3]) == 1 and int(a[4]) == 1))
        return r != 0.0 if allowed else r == 0.0      # non-zero where the law allows it (the N2O5 + H2O path survives xhal = 0), else exactly 0
    return pred


def _fdhet_x(e, a):
    """x1, x2 of the HNO3 branch as the law forms them"""
    na = int(a[0])
    yx = e.at("YXKMTD_HNO3", na - 1)
    x1 = yx * e.at("YCWD", na - 1)
    den = e.at("YXEQ_HNO3") + 1.0e-2
    if e.has("C_NO3ML"):
        caq = ((e.at("C_HNO3L", na - 1) + e.at("C_NO3ML", na - 1)) * 1.0e-2) / den if den != 0.0 else 0.0
    else:
        caq = ((e.at("C_HNO3L", na - 1) * 1.5e3) * 1.0e-2) / den if den != 0.0 else math.inf
    x2 = ((-yx) / (e.at("C_HNO3") * e.at("YHENRY_HNO3"))) * caq if e.at("C_HNO3") != 0.0 and e.at("YHENRY_HNO3") != 0.0 else 0.0
    return x1, x2


def _edges():
    """{edge name: (laws, predicate(env, args, result))}: an edge is REACHED by a case if the predicate holds in one call of one of its laws"""
    E = {}
    for law, gi in _GUARDED.items():
        E["%s guard = 0" % law] = ((law,), lambda e, a, r, gi=gi: _pos0(a[gi]) and r == 0.0)
        E["%s guard = -0.0" % law] = ((law,), lambda e, a, r, gi=gi: _neg0(a[gi]) and r == 0.0)
        E["%s guard < 0" % law] = ((law,), lambda e, a, r, gi=gi: a[gi] < 0.0 and r == 0.0)
        E["%s guard > 0, result non-zero" % law] = ((law,), lambda e, a, r, gi=gi: a[gi] > 0.0 and r != 0.0)
    E["uparm d (a concentration) < 0"] = (("uparm",), lambda e, a, r: a[3] < 0.0 and r == 0.0)
    E["uparm d = -0.0"] = (("uparm",), lambda e, a, r: _neg0(a[3]) and r == 0.0)
    E["uplim max(c,0) clamps c < 0"] = (("uplim",), lambda e, a, r: a[2] < 0.0 and a[3] > 0.0 and r == a[0])
    E["uplim c = -0.0"] = (("uplim",), lambda e, a, r: _neg0(a[2]) and a[3] > 0.0 and r == a[0])
    E["uplim c is NaN"] = (("uplim",), lambda e, a, r: a[2] != a[2] and a[3] > 0.0 and r == a[0])      # MAX(NaN, 0.d0) is 0 in the reference
    E["uplip max(b,0) clamps b < 0"] = (("uplip",), lambda e, a, r: a[1] < 0.0 and a[2] > 0.0 and r == a[0] * (a[2] * a[2]))
    E["uplip b = -0.0"] = (("uplip",), lambda e, a, r: _neg0(a[1]) and a[2] > 0.0 and r == a[0] * (a[2] * a[2]))
    E["uplip b is NaN"] = (("uplip",), lambda e, a, r: a[1] != a[1] and a[2] > 0.0 and r == a[0] * (a[2] * a[2]))
    E["fbck2 ck = 0"] = (("fbck2",), lambda e, a, r: _pos0(a[5]) and r == 0.0)
    E["fbck2 ck = -0.0"] = (("fbck2",), lambda e, a, r: _neg0(a[5]) and r == 0.0)
    E["dmin2 a < 1e10 (literal)"] = (("dmin2",), lambda e, a, r: a[0] < 1.0e10 and r == a[0])
    E["dmin2 a = 1e10 (literal)"] = (("dmin2",), lambda e, a, r: a[0] == 1.0e10 and r == 1.0e10)
    E["dmin2 a > 1e10 (literal)"] = (("dmin2",), lambda e, a, r: a[0] > 1.0e10 and r == 1.0e10)
    E["dmin3 a = 4e10, the nearest literal to 2e10 (clipped; unclipped is unreachable)"] = (("dmin3",), lambda e, a, r: a[0] == 4.0e10 and r == 2.0e10)
    E["flsc6 b = 1e-15"] = (("flsc6",), lambda e, a, r: a[1] == 1.0e-15 and r == 0.0)
    E["flsc6 b = 1e-15 + 1 ulp"] = (("flsc6",), lambda e, a, r: a[1] == math.nextafter(1.0e-15, 1.0) and r != 0.0)
    E["flsc6 b = 0"] = (("flsc6",), lambda e, a, r: _pos0(a[1]) and r == 0.0)
    E["flsc6 b < 0"] = (("flsc6",), lambda e, a, r: a[1] < 0.0 and r == 0.0)
    E["fhet_t hetT = 0, all of H2OL CLM BRM 0"] = (("fhet_t",), lambda e, a, r: _hett(e, int(a[0]), False)[0] == 0.0 and e.at("H2OL", int(a[0]) - 1) == 0.0 and r == 0.0)
    E["fhet_t hetT < 0"] = (("fhet_t",), lambda e, a, r: _hett(e, int(a[0]), False)[0] < 0.0 and r == 0.0)
    E["fhet_t hetT = 0 by cancellation"] = (("fhet_t",), lambda e, a, r: _hett(e, int(a[0]), False)[0] == 0.0 and e.at("H2OL", int(a[0]) - 1) != 0.0 and r == 0.0)
    wet = lambda a: a[0] != 0.0 and a[1] == 0.0
    E["fhet_d wet, hetT = 0, all of H2OL CLM BRM 0"] = (_FHET_D, lambda e, a, r: wet(a) and e.at("XHAL") != 0.0 and _hett(e, int(a[2]), False)[0] == 0.0 and e.at("H2OL", int(a[2]) - 1) == 0.0 and r == 0.0)
    E["fhet_d wet, hetT < 0"] = (_FHET_D, lambda e, a, r: wet(a) and e.at("XHAL") != 0.0 and _hett(e, int(a[2]), False)[0] < 0.0 and r == 0.0)
    E["fhet_d wet, hetT = 0 by cancellation"] = (_FHET_D, lambda e, a, r: wet(a) and e.at("XHAL") != 0.0 and _hett(e, int(a[2]), False)[0] == 0.0 and e.at("H2OL", int(a[2]) - 1) != 0.0 and r == 0.0)
    E["fhet_d dry, YCWD = 0, xhal = 0: hetT = 0"] = (_FHET_D, lambda e, a, r: a[0] != 0.0 and a[1] != 0.0 and e.at("XHAL") == 0.0 and e.at("YCWD", int(a[2]) - 1) == 0.0 and r == 0.0)
    E["fhet_d dry, YCWD = 0, xhal = 1"] = (_FHET_D, lambda e, a, r: a[0] != 0.0 and a[1] != 0.0 and e.at("XHAL") != 0.0 and e.at("YCWD", int(a[2]) - 1) == 0.0 and r == 0.0)
    for hal in (False, True):
        for liq in (False, True):
            for het in (False, True):
                E["fhet_d xhal=%d xliq=%d xhet=%d" % (hal, liq, het)] = (_FHET_D, _fhet_d_setting(hal, liq, het))
    E["fdhet YCWD = 0"] = (_FDHET, lambda e, a, r: e.at("YCWD", int(a[0]) - 1) == 0.0 and r == 0.0)
    E["fdhet C(HNO3) = 0"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and e.at("C_HNO3") == 0.0 and r == _fdhet_x(e, a)[0] != 0.0)
    E["fdhet yhenry = 0"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and e.at("YHENRY_HNO3") == 0.0 and e.at("C_HNO3") != 0.0 and r == _fdhet_x(e, a)[0] != 0.0)
    E["fdhet yxeq + 1e-2 = 0"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and e.at("YXEQ_HNO3") + 1.0e-2 == 0.0)
    E["fdhet x1 + x2 < 0, clamped"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and math.isfinite(sum(_fdhet_x(e, a))) and sum(_fdhet_x(e, a)) < 0.0 and _pos0(r))
    E["fdhet x1 + x2 > 0"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and sum(_fdhet_x(e, a)) > 0.0 and r > 0.0)
    E["fdhet x1 + x2 is NaN"] = (_FDHET, lambda e, a, r: int(a[1]) == 1 and math.isnan(sum(_fdhet_x(e, a))) and r != r)      # MAX(0.d0, NaN) is NaN in the reference
    E["te = 180 K"] = (("farr",), lambda e, a, r: e[1] == 180.0 and math.isfinite(r))
    E["te = 330 K"] = (("farr",), lambda e, a, r: e[1] == 330.0 and math.isfinite(r))
    return E


EDGES = _edges()
# edges that only the input vector shows (no law sees them as an argument): name -> predicate(mech, env row, rconst row)
VECTOR_EDGES = {
    "night: every ph_rat 0": lambda mech, e, r: not any(e[i] for i, n in enumerate(env_info(mech)[0]) if n.startswith("ph_rat")),
    "a NaN input, NaN rate constants": lambda mech, e, r: bool(np.isnan(e).any() and np.isnan(r).any()),
    "+Inf input, non-finite rate constants": lambda mech, e, r: bool(np.isposinf(e).any() and (~np.isfinite(r)).any()),
    "-0.0 input": lambda mech, e, r: bool(((e == 0.0) & np.signbit(e)).any()),
}
# which NaN edge belongs to which mechanism: the NaN sits under uplim / uplip where the mechanism has them, else under fdhetg's max
NAN_EDGES = {"gas": ("fdhet x1 + x2 is NaN",), "aer": ("uplim c is NaN", "uplip b is NaN", "fdhet x1 + x2 is NaN"),
             "tot": ("uplim c is NaN", "uplip b is NaN", "fdhet x1 + x2 is NaN")}


def applicable(mech):
    """the edges of EDGES the mechanism can reach: it calls one of the edge's laws (and the NaN edges as NAN_EDGES places them)"""
    L = laws(mech)
    out = []
    for name, (ls, _) in EDGES.items():
        if not L & set(ls):
            continue
        if name.endswith("is NaN") and name not in NAN_EDGES[mech]:
            continue
        out.append(name)
    return out


class counting_funcs:
    """with counting_funcs(mech) as hit: rates_py.FUNCS wrapped; hit[edge] counts the calls in which the edge's predicate held"""

    def __init__(self, mech):
        self.mech = mech
        self.hit = {n: 0 for n in EDGES}

    def __enter__(self):
        self.saved = dict(rates_py.FUNCS)
        by_law = {}
        for name, (ls, pred) in EDGES.items():
            for law in ls:
                by_law.setdefault(law, []).append((name, pred))
        for law, fn in self.saved.items():
            if law in by_law:
                rates_py.FUNCS[law] = self._wrap(fn, by_law[law])
        return self.hit

    def _wrap(self, fn, preds):
        def wrapped(e, *a):
            r = fn(e, *a)
            for name, pred in preds:
                if pred(e, a, r):
                    self.hit[name] += 1
            return r
        return wrapped

    def __exit__(self, *exc):
        rates_py.FUNCS.clear()
        rates_py.FUNCS.update(self.saved)


@functools.lru_cache(maxsize=None)
def reach(mech):
    """{edge: [names of the cases that reach it]} over EDGES and VECTOR_EDGES"""
    c = cases(mech)
    out = {n: [] for n in list(EDGES) + list(VECTOR_EDGES)}
    for name, env in zip(c["names"], c["env"]):
        with counting_funcs(mech) as hit:
            r = evaluate(mech, env)
        for n, k in hit.items():
            if k:
                out[n].append(name)
        for n, pred in VECTOR_EDGES.items():
            if pred(mech, env, r):
                out[n].append(name)
    return out


# ---------------------------------------------------------------------------------------------------------------- last-place freedom of the library
def spread(mech):
    """-> (worst relative movement of the restatement over the cases when exp, pow and log10 return the next double up, or down: over the programs that
    hold a library call, NaN, infinite and exactly-zero entries left out; number of entries measured)"""
    from liq_cases import shimmed_math, movement
    nominal = restated(mech)
    lib = program_kinds(mech)[2]
    keep = np.isfinite(nominal[:, lib]) & (nominal[:, lib] != 0.0)
    worst = 0.0
    for up in (True, False):
        with shimmed_math(up):
            moved = np.stack([evaluate(mech, e) for e in cases(mech)["env"]])[:, lib]
        assert np.array_equal(np.isfinite(moved) & (moved != 0.0), keep)
        worst = max(worst, movement(nominal[:, lib][keep], moved[keep]))
    return worst, int(keep.sum())


# ---------------------------------------------------------------------------------------------------------------- batch shapes
BATCH_NCELL = (1, 63, 64, 65, 129, 148, 6401, 12801, 131073)      # 12 801: the one size at which gas (cap 21) splits between its cap and 1


def launch_gy(ncell, nreact):
    """launch_update_rconst's rule (mistra_amd/csrc/rates.hip): the reactions are cut into 4 * gy chunks"""
    gx = (ncell + 63) // 64
    gy = 1 if gx >= 2048 else (2048 + gx - 1) // gx
    return min(gy, (nreact + 15) // 16)
