#!/usr/bin/env python3
"""Derive a reduced mechanism table from a KMCH v2 table, without KPP (the work is done by mistra_amd/mechderive.py).

  tools/derive_mech.py SOURCE.mech OUT.mech [--drop 3,17,40-44] [--drop-file FILE] [--remove-species]

--drop            reactions to leave out, 0-based, as numbers and ranges
--drop-file       the same, one number or range per line or separated by commas
--remove-species  also remove the variable species that are left without a reaction (they are renumbered out of V)

Writes OUT.mech and, beside it, OUT.json: the source's name and the kept reactions and species as index maps into the source, with which inputs
of the source mechanism (VAR, RCONST) are cut to the derived one.  With nothing dropped the output equals the source byte for byte.
To run the table, name it in MISTRA_USER_MECHS when the library is built."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def parse_list(text):
    out = []
    for part in text.replace("\n", ",").split(","):
        part = part.strip()
        if not part:
            continue
        if "-" in part:
            lo, hi = part.split("-")
            out += range(int(lo), int(hi) + 1)
        else:
            out.append(int(part))
    return out


def main(argv=None):
    from mistra_amd import mechderive, mechtab
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source")
    ap.add_argument("out")
    ap.add_argument("--drop", default="")
    ap.add_argument("--drop-file")
    ap.add_argument("--remove-species", action="store_true")
    a = ap.parse_args(argv)
    drop = parse_list(a.drop)
    if a.drop_file:
        drop += parse_list(open(a.drop_file).read())
    name = os.path.splitext(os.path.basename(a.source))[0]
    t = mechtab.MechTables(name, a.source)
    tab, maps = mechderive.derive(t, drop, a.remove_species)
    mechderive.write(a.out, tab, maps)
    print("%s -> %s: nvar=%d nfix=%d nreact=%d nnz=%d (source: nvar=%d nreact=%d nnz=%d)" %
          (a.source, a.out, tab["nvar"], tab["nfix"], tab["nreact"], tab["nnz"], t.nvar, t.nreact, t.nnz))


if __name__ == "__main__":
    main()
