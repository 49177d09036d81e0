"""The one list of kernel units (mistra_amd/build.py: kernel_units): its counts and members, that build_lib compiles and checks exactly that list, that
a unit which does not exist cannot be expressed, and the stand-alone probe of the host-buffer entries' cell split (tests/probe/cell_split_probe.cpp)."""
import os
import subprocess

import pytest

from mistra_amd import build as B

ALL_FIVE = {(m, k) for m in (0, 1, 2) for k in (1, 2, 3, 4, 5)}


def test_counts_and_members_per_variant():
    """12 method units (no Ros3: the product unit's), 3 trace units (Ros3 alone), 15 series and 15 flux units, one unit per user slot, the product unit"""
    per = {v: sorted((u.mech, u.method) for u in B.VARIANT_UNITS if u.variant == v) for v in (3, 4, 5, 6)}
    assert {v: len(p) for v, p in per.items()} == {3: 12, 4: 3, 5: 15, 6: 15}
    assert set(per[3]) == {(m, k) for m in (0, 1, 2) for k in (1, 3, 4, 5)}
    assert set(per[4]) == {(m, 2) for m in (0, 1, 2)}
    assert set(per[5]) == ALL_FIVE and set(per[6]) == ALL_FIVE
    assert len(B.VARIANT_UNITS) == 45 and {u.variant for u in B.VARIANT_UNITS} == {3, 4, 5, 6}
    for n in (0, 1, 2):
        units = B.kernel_units(n)
        assert len(units) == len(set(units)) == 1 + 45 + n
        assert units.count(B.PRODUCT) == 1 and [u.mech for u in units if u.variant == "user"] == list(range(n))
        assert [u for u in units if u.variant not in ("product", "user")] == B.VARIANT_UNITS


def test_object_names_sources_and_flags():
    built = [B.unit_build(u) for u in B.kernel_units(2)]
    names = [name for _, name, _ in built]
    assert len(set(names)) == len(names) and all(n.endswith(".o") for n in names)
    assert not set(names) & {os.path.splitext(s)[0] + ".o" for s in B.SOURCES} and "capi_noslots.o" not in names
    assert B.unit_build(B.PRODUCT) == (B.PRODUCT_SOURCE, "ros3_kernel.o", [])
    for u in B.VARIANT_UNITS:
        assert B.unit_build(u)[0] == B.UNIT_SOURCE
        assert B.unit_build(u)[2] == ["-DMISTRA_UNIT_VARIANT=%d" % u.variant, "-DMISTRA_UNIT_MECH=%d" % u.mech, "-DMISTRA_UNIT_METHOD=%d" % u.method]
    assert B.unit_build(B.Unit("user", 1, None))[0] == B.USER_SOURCE and "-DMISTRA_USER_SLOT=1" in B.unit_build(B.Unit("user", 1, None))[2]
    assert all(os.path.exists(os.path.join(B.CSRC, src)) for src, _, _ in built)


@pytest.mark.parametrize("unit", [(3, 0, 2), (3, 2, 2), (4, 0, 1), (4, 1, 5), (4, 2, 3), (5, 0, 0), (6, 1, 6), (2, 0, 2), (7, 0, 2), (5, 3, 2),
                                  ("user", 2, None), ("user", 0, 2), ("product", 0, None), ("series", 0, 2)])
def test_a_unit_that_does_not_exist_cannot_be_expressed(unit):
    """VARIANT 3 / Ros3 (that kernel lives in the product unit), VARIANT 4 / any other method, and everything out of range: unit_build raises, and with
    it whatever goes through it (the listing command of the ring report and of tools/isa_compare.py)"""
    with pytest.raises(ValueError, match="no kernel unit"):
        B.unit_build(B.Unit(*unit))
    with pytest.raises(ValueError, match="no kernel unit"):
        B.unit_listing_cmd(B.Unit(*unit), "x.s")
    with pytest.raises(ValueError, match="no kernel unit"):
        B.ring_register_report(unit=B.Unit(*unit))


@pytest.mark.parametrize("n_user", (2, 0))
def test_build_lib_compiles_and_checks_exactly_the_list(n_user, monkeypatch, tmp_path):
    """compile and report functions replaced by recorders (no hipcc run): every unit of the list, and nothing else, is compiled from its source with its
    flags into its object, is submitted to the ring report and its listing to the hazard report, and is linked; the library without user slots
    is linked from everything but the user units"""
    cmds, reported, scanned = [], [], []
    monkeypatch.setattr(B, "OBJDIR", str(tmp_path / "build"))
    monkeypatch.setattr(B, "LIBDIR", str(tmp_path / "lib"))
    monkeypatch.setattr(B, "hipcc", lambda: "hipcc")
    monkeypatch.setattr(B, "prepare_user_mechs", lambda force=False, verbose=False: (n_user, []))
    monkeypatch.setattr(B, "_run", lambda cmd, verbose=False: cmds.append(cmd))
    monkeypatch.setattr(B, "ring_register_report", lambda isa_path=None, unit=B.PRODUCT: reported.append(unit) or {"__isa_text__": repr(tuple(unit))})
    monkeypatch.setattr(B, "isa_hazard_report", lambda text: scanned.append(text) or [])
    B.build_lib(force=True)
    units = B.kernel_units(n_user)
    compiles = {os.path.basename(c[c.index("-o") + 1]): c for c in cmds if "-c" in c}
    links = [c for c in cmds if "-shared" in c]
    host = {os.path.splitext(s)[0] + ".o" for s in B.SOURCES} | ({"capi_noslots.o"} if n_user else set())
    assert len(compiles) == len([c for c in cmds if "-c" in c]) and len(compiles) + len(links) == len(cmds)
    assert set(compiles) == {B.unit_build(u)[1] for u in units} | host
    for u in units:
        src, name, flags = B.unit_build(u)
        c = compiles[name]
        assert c[c.index("-c") + 1] == os.path.join(B.CSRC, src) and all(f in c for f in flags), u
        assert [f for f in c if f.startswith("-DMISTRA_UNIT_") or f.startswith("-DMISTRA_USER_SLOT")] == [f for f in flags if not f.startswith(("-I", "-DMISTRA_USER_MECHS"))], u
    assert sorted(reported, key=repr) == sorted(units, key=repr) and sorted(scanned) == sorted(repr(tuple(u)) for u in units)
    objs = lambda c: {os.path.basename(f) for f in c if f.endswith(".o")}
    assert len(links) == (2 if n_user else 1)
    assert objs(links[0]) == set(compiles) - {"capi_noslots.o"} and links[0][links[0].index("-o") + 1] == B.LIB
    if n_user:
        user = {B.unit_build(u)[1] for u in units if u.variant == "user"}
        assert len(user) == n_user and objs(links[1]) == set(compiles) - user - {"capi.o"} and links[1][links[1].index("-o") + 1] == B.LIB_NOSLOTS


def test_a_hazard_in_any_unit_stops_the_link(monkeypatch, tmp_path):
    """the last unit of the list is checked like the first: a finding in it raises and nothing is linked"""
    cmds = []
    last = B.kernel_units(2)[-1]
    monkeypatch.setattr(B, "OBJDIR", str(tmp_path / "build"))
    monkeypatch.setattr(B, "LIBDIR", str(tmp_path / "lib"))
    monkeypatch.setattr(B, "hipcc", lambda: "hipcc")
    monkeypatch.setattr(B, "prepare_user_mechs", lambda force=False, verbose=False: (2, []))
    monkeypatch.setattr(B, "_run", lambda cmd, verbose=False: cmds.append(cmd))
    monkeypatch.setattr(B, "ring_register_report", lambda isa_path=None, unit=B.PRODUCT: {"__isa_text__": repr(tuple(unit))})
    monkeypatch.setattr(B, "isa_hazard_report", lambda text: ["a finding"] if text == repr(tuple(last)) else [])
    with pytest.raises(RuntimeError, match="hazards the hardware does not interlock"):
        B.build_lib(force=True)
    assert not [c for c in cmds if "-shared" in c]


def test_cell_split_probe(tmp_path):
    """tests/probe/cell_split_probe.cpp, built with the host compiler and run directly: the split of a host-buffer batch over 1 .. 4 device slots"""
    exe = str(tmp_path / "cell_split_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe", "cell_split_probe.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "40 cases ok" in r.stdout, r.stdout + r.stderr
