"""Derive a reduced mechanism table from a KMCH v2 table (`mistra_amd/mech/<name>.mech`) without KPP: drop reactions, optionally remove the
species that are left without one, and recompute the LU pattern.  `tools/derive_mech.py` is the command line of this module.

What a derived table keeps of its source:
  * every surviving term list (`a_fac` of a reaction, `b_fac` of a B product, the Vdot sum of a species, the JVS sum of a Jacobian slot) in the
    source's order — the kernel and the oracle add in that order;
  * the species order; removed species are renumbered out of V, the F and constant indices shift with them;
  * the constants.
The LU pattern is the symbolic fill-in of the surviving structural pattern (the JVS slots that still have a term, plus the diagonal), eliminated
row by row in the table's order as KppDecomp_x does.  For gas, aer and tot with nothing dropped that reproduces LU_CROW / LU_ICOL exactly, so the
identity derivation gives the shipped tables back byte for byte.
"""
import json
import os
import numpy as np

from . import mechtab

_I32_LISTS = ("crow", "icol", "diag", "a_ptr", "a_fac", "b_rct", "b_ptr", "b_fac", "vd_ptr", "vd_idx", "jv_ptr", "jv_idx")
_F64_LISTS = ("vd_coef", "jv_coef", "consts")


def species_reactions(t):
    """-> per variable species the set of reactions it takes part in, as a factor of the rate product or as a term of its Vdot sum."""
    part = [set() for _ in range(t.nvar)]
    for r in range(t.nreact):
        for f in t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]:
            if f < t.nvar:
                part[f].add(r)
    for s in range(t.nvar):
        part[s].update(int(r) for r in t.vd_idx[t.vd_ptr[s]:t.vd_ptr[s + 1]])
    return part


def symbolic_fill(rows):
    """rows: per row the set of structural columns (diagonal included).  Row-wise elimination in the given order, as KppDecomp_x walks the
    pattern: row k receives, for every j < k it holds (those that fill in on the way too), the columns c > j of row j.  -> sorted rows."""
    out = []
    for k, row in enumerate(rows):
        cols = set(row)
        cols.add(k)
        todo = sorted(c for c in cols if c < k)
        done = set()
        while todo:
            j = todo.pop(0)
            if j in done:
                continue
            done.add(j)
            new = [c for c in out[j] if c > j and c not in cols]
            cols.update(new)
            lower = [c for c in new if c < k]
            if lower:
                todo = sorted(set(todo).union(lower))
        out.append(sorted(cols))
    return out


def derive(t, drop=(), remove_species=False):
    """t: mechtab.MechTables.  drop: reaction indices (0-based) to leave out.  remove_species: also remove the variable species that take part in
    no surviving reaction.  -> (tables dict for write_mech, maps dict: kept reactions and kept species as indices into the source)."""
    drop = set(int(r) for r in drop)
    if any(r < 0 or r >= t.nreact for r in drop):
        raise ValueError("a dropped reaction is not in the mechanism")
    kept_r = [r for r in range(t.nreact) if r not in drop]
    rmap = {old: new for new, old in enumerate(kept_r)}
    part = species_reactions(t)
    if remove_species:
        kept_s = [s for s in range(t.nvar) if part[s] - drop]
    else:
        kept_s = list(range(t.nvar))
    smap = {old: new for new, old in enumerate(kept_s)}
    nvar = len(kept_s)
    shift = nvar - t.nvar

    def code(f):
        f = int(f)
        if f >= t.nvar:
            return f + shift      # F and the constants sit behind V
        if f not in smap:
            raise ValueError("a surviving product has a removed species as a factor")
        return smap[f]

    def products(ptr, fac, keep):
        out_ptr, out_fac = [0], []
        for i in keep:
            out_fac += [code(f) for f in fac[ptr[i]:ptr[i + 1]]]
            out_ptr.append(len(out_fac))
        return np.array(out_ptr, np.int32), np.array(out_fac, np.int32)

    a_ptr, a_fac = products(t.a_ptr, t.a_fac, kept_r)
    kept_b = [b for b in range(t.nb) if int(t.b_rct[b]) in rmap]
    bmap = {old: new for new, old in enumerate(kept_b)}
    b_rct = np.array([rmap[int(t.b_rct[b])] for b in kept_b], np.int32)
    b_ptr, b_fac = products(t.b_ptr, t.b_fac, kept_b)

    def sums(ptr, idx, coef, rows, remap):      # rows: source row per output row, None = an empty sum
        out_ptr, out_idx, out_coef = [0], [], []
        for i in rows:
            if i is not None:
                for q in range(ptr[i], ptr[i + 1]):
                    if int(idx[q]) in remap:
                        out_idx.append(remap[int(idx[q])])
                        out_coef.append(coef[q])
            out_ptr.append(len(out_idx))
        return np.array(out_ptr, np.int32), np.array(out_idx, np.int32), np.array(out_coef, np.float64)

    vd_ptr, vd_idx, vd_coef = sums(t.vd_ptr, t.vd_idx, t.vd_coef, kept_s, rmap)

    # ---- the surviving structural pattern and its fill-in
    slot_of = {}
    rows = [set() for _ in range(nvar)]
    for k in kept_s:
        for p in range(t.crow[k], t.crow[k + 1]):
            c = int(t.icol[p])
            if c in smap and any(int(b) in bmap for b in t.jv_idx[t.jv_ptr[p]:t.jv_ptr[p + 1]]):
                rows[smap[k]].add(smap[c])
                slot_of[(smap[k], smap[c])] = p
    filled = symbolic_fill(rows)
    crow = np.zeros(nvar + 1, np.int32)
    icol, diag, src_slot = [], [], []
    for k, cols in enumerate(filled):
        for c in cols:
            if c == k:
                diag.append(len(icol))
            src_slot.append(slot_of.get((k, c)))
            icol.append(c)
        crow[k + 1] = len(icol)
    jv_ptr, jv_idx, jv_coef = sums(t.jv_ptr, t.jv_idx, t.jv_coef, src_slot, bmap)

    tab = dict(nvar=nvar, nfix=t.nfix, nreact=len(kept_r), nnz=len(icol), crow=crow, icol=np.array(icol, np.int32), diag=np.array(diag, np.int32),
               a_ptr=a_ptr, a_fac=a_fac, b_rct=b_rct, b_ptr=b_ptr, b_fac=b_fac, vd_ptr=vd_ptr, vd_idx=vd_idx, vd_coef=vd_coef,
               jv_ptr=jv_ptr, jv_idx=jv_idx, jv_coef=jv_coef, consts=np.array(t.consts, np.float64))
    maps = dict(source=t.name, nvar=nvar, nfix=t.nfix, nreact=len(kept_r), nnz=len(icol), kept_reactions=kept_r, kept_species=kept_s)
    return tab, maps


def table_bytes(tab):
    """The KMCH v2 file of a tables dict (the layout tools/extract_mech.py writes and mechtab.MechTables reads)."""
    hdr = np.array([mechtab.MAGIC, mechtab.VERSION, tab["nvar"], tab["nfix"], tab["nreact"], tab["nnz"], len(tab["a_fac"]), len(tab["b_rct"]),
                    len(tab["b_fac"]), len(tab["vd_idx"]), len(tab["jv_idx"]), len(tab["consts"])], np.int32)
    raw = hdr.tobytes() + b"".join(np.ascontiguousarray(tab[k], np.int32).tobytes() for k in _I32_LISTS)
    raw += b"\0" * ((-len(raw)) % 8)
    return raw + b"".join(np.ascontiguousarray(tab[k], np.float64).tobytes() for k in _F64_LISTS)


def maps_text(maps):
    """The .json beside a derived table: the source and the kept reactions and species as index maps into it."""
    return json.dumps(maps, indent=None, separators=(",", ":"), sort_keys=True) + "\n"


def write(path, tab, maps):
    """Writes <path> (the table) and <path minus .mech>.json."""
    with open(path, "wb") as f:
        f.write(table_bytes(tab))
    with open(os.path.splitext(path)[0] + ".json", "w") as f:
        f.write(maps_text(maps))


def load_maps(name, mech_dir=None):
    with open(os.path.join(mech_dir or mechtab.MECH_DIR, name + ".json")) as f:
        return json.load(f)


# The two demo tables of the user mechanism slots: name -> (source, remove the species left without a reaction), both cut by
# fewest_reactions_rule.  Their index maps (<name>.json) are committed; the tables themselves are binary and are not: they are derived from the
# committed source tables where they are missing or stale (mistra_amd/build.py before it reads them; the tests through tests/user_mech_cases.py,
# which pins a SHA-256 of every one of the four files).
DEMO_TABLES = {"demo_g": ("gas", True), "demo_a": ("aer", False)}
DEMO_SPECIES = 16


def ensure_demo_tables(mech_dir=None):
    """Writes <mech dir>/demo_g.mech and demo_a.mech where the file is missing or is not what the rule derives; a file that is already right is
    left untouched, and so is every committed file: the .json maps are never written here (a map that differs from the rule raises).
    -> the tables' paths"""
    mech_dir = mech_dir or mechtab.MECH_DIR
    paths = []
    for name, (source, remove) in DEMO_TABLES.items():
        t = mechtab.MechTables(source, os.path.join(mech_dir, source + ".mech"))
        _, drop = fewest_reactions_rule(t, DEMO_SPECIES)
        tab, maps = derive(t, drop, remove)
        with open(os.path.join(mech_dir, name + ".json")) as f:
            if f.read() != maps_text(maps):
                raise RuntimeError("%s.json is not the index map of the table the rule derives from %s.mech" % (name, source))
        path, want, have = os.path.join(mech_dir, name + ".mech"), table_bytes(tab), None
        if os.path.exists(path):
            with open(path, "rb") as f:
                have = f.read()
        if have != want:      # (whole file or nothing: another process may be reading the directory)
            tmp = "%s.%d.tmp" % (path, os.getpid())
            with open(tmp, "wb") as f:
                f.write(want)
            os.replace(tmp, path)
        paths.append(path)
    return paths


# Tables at the edges of the user slots' size classes, for the twin libraries mistra_amd/build.py: build_edge_twins links and
# tests/test_user_edges.py, tests/test_gpu_user_edges.py run: name -> (source, species handed to fewest_reactions_rule; None = the source's own
# bytes under this name).  All are cut with the species left without a reaction REMOVED.  Neither the tables nor their maps are committed: both are
# written into EDGE_DIR, beside copies of gas.mech, aer.mech and tot.mech, so that the directory serves as a mechanism directory.
# tests/user_edge_cases.py pins a SHA-256 and the sizes of every table.
EDGE_TABLES = {"edge_g64": ("gas", 37), "edge_a128": ("aer", 129), "edge_a129": ("aer", 128), "edge_t417": ("tot", None)}
EDGE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "build", "edge_mech")


def derive_edge(name, mech_dir=None):
    """-> (tables dict, maps dict) of an edge table, derived from the source table in `mech_dir`"""
    source, nspecies = EDGE_TABLES[name]
    t = mechtab.MechTables(source, os.path.join(mech_dir or mechtab.MECH_DIR, source + ".mech"))
    drop = () if nspecies is None else fewest_reactions_rule(t, nspecies)[1]
    return derive(t, drop, remove_species=True)


def _write_if_changed(path, want):
    have = None
    if os.path.exists(path):
        with open(path, "rb") as f:
            have = f.read()
    if have != want:      # (whole file or nothing: another process may be reading the directory)
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            f.write(want)
        os.replace(tmp, path)


def ensure_edge_tables(out_dir=None, mech_dir=None):
    """Writes the edge tables, their .json maps and copies of gas.mech, aer.mech and tot.mech into `out_dir` (default EDGE_DIR) where a file is
    missing or is not what the rule derives; a file that is already right is left untouched.  -> {name: the table's path}"""
    out_dir, mech_dir = out_dir or EDGE_DIR, mech_dir or mechtab.MECH_DIR
    os.makedirs(out_dir, exist_ok=True)
    for source in sorted({s for s, _ in EDGE_TABLES.values()}):
        with open(os.path.join(mech_dir, source + ".mech"), "rb") as f:
            _write_if_changed(os.path.join(out_dir, source + ".mech"), f.read())
    paths = {}
    for name in EDGE_TABLES:
        tab, maps = derive_edge(name, mech_dir)
        paths[name] = os.path.join(out_dir, name + ".mech")
        _write_if_changed(paths[name], table_bytes(tab))
        _write_if_changed(os.path.join(out_dir, name + ".json"), maps_text(maps).encode())
    return paths


def fewest_reactions_rule(t, nspecies=16):
    """The cut the demo tables are made with: the `nspecies` variable species that take part in the fewest reactions (ties: the lower index;
    species that take part in none are skipped) and every reaction any of them takes part in.  -> (species, reactions to drop), sorted."""
    part = species_reactions(t)
    order = sorted((len(part[s]), s) for s in range(t.nvar) if part[s])
    species = sorted(s for _, s in order[:nspecies])
    drop = sorted(set().union(*(part[s] for s in species)))
    return species, drop
