"""In-tree build of libmistra_chem.so (HIP kernels for gfx950 + the C ABI of include/mistra_chem.h).

`python -m mistra_amd.build` or `build_lib()`.  hipcc cross-compiles for gfx950 without a GPU present.
The library is written to mistra_amd/lib/ (git-ignored, shipped to the GPU box with the working tree).
"""
import collections
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
OBJDIR = os.path.join(PKG, "build")
LIB = os.path.join(LIBDIR, "libmistra_chem.so")
# the same library WITHOUT user slots, linked beside it whenever the library has slots (capi.cpp compiled once more, every other object shared):
# what tests/test_gpu_user_mech.py holds gas, aer and tot of the library with slots to, bit for bit.  Nothing loads it otherwise.
LIB_NOSLOTS = os.path.join(LIBDIR, "libmistra_chem_noslots.so")
# ... and the library without user slots whose tot product kernels and tot Rodas4 unit are compiled with -DMISTRA_GSUM_CHAIN=0 (no chain passes in the
# gather-sum machine): what tests/test_gpu_gsum_chain.py holds the product to, bit for bit.  Nothing loads it otherwise.
LIB_NOCHAIN = os.path.join(LIBDIR, "libmistra_chem_nochain.so")
NOCHAIN_FLAG = "-DMISTRA_GSUM_CHAIN=0"

ARCH = "gfx950"
# -ffp-contract=off: one rounding per multiply and per add, as in the reference built without FMA contraction
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function"]
SOURCES = ["mech_tables.cpp", "schedule.cpp", "capi.cpp", "rates.hip", "pack.hip"]
# ---- THE KERNEL UNITS: every translation unit that holds ros3_integrate_kernel instantiations, as one list of uniform records.  Each is a unit of its
# own because the non-inlined device functions the kernels share are compiled once per unit, under the register budget of all kernels in it: the product
# kernels' unit compiles as it does without the others, and they side by side.
#   Unit("product", None, None)      ros3_kernel.hip: the product, phase-timing, first-step-dump and options (Ros3) kernels of gas, aer and tot
#   Unit(variant, mech, method)      ros_unit_kernel.hip once per kernel VARIANT 3 .. 6 (ros3_kernel.hip), mechanism 0 gas | 1 aer | 2 tot and IPAR(4):
#                                    3 the method kernels (Ros2, Ros4, Rodas3, Rodas4; Ros3 with options is in the product unit), 4 the step-control trace
#                                    (Ros3 only), 5 the series kernels and 6 the flux kernels (all five methods)
#   Unit("user", slot, None)         ros_user_kernel.hip once per user mechanism slot (mechanism ids 3 and 4), against the slot's generated traits header
# MISTRA_USER_MECHS = at most two table paths separated by colons, default the two demo tables (tools/derive_mech.py cuts them from gas and aer), empty =
# a library without user slots.  Per slot user_traits_gen (a host program built from the schedule compiler) writes the traits header into the build
# directory.
Unit = collections.namedtuple("Unit", "variant mech method")
PRODUCT = Unit("product", None, None)
NOCHAIN_UNIT = Unit(3, 2, 5)      # the method kernels, tot, Rodas4
PRODUCT_SOURCE = "ros3_kernel.hip"
UNIT_SOURCE = "ros_unit_kernel.hip"
USER_SOURCE = "ros_user_kernel.hip"
ROS3 = 2
VARIANT_METHODS = {3: (1, 3, 4, 5), 4: (ROS3,), 5: (1, 2, 3, 4, 5), 6: (1, 2, 3, 4, 5)}
VARIANT_UNITS = [Unit(v, mech, method) for v, methods in VARIANT_METHODS.items() for mech in (0, 1, 2) for method in methods]
USER_GEN_SOURCES = ["user_traits_gen.cpp", "schedule.cpp", "mech_tables.cpp"]
USER_DEFAULT = [os.path.join(PKG, "mech", "demo_g.mech"), os.path.join(PKG, "mech", "demo_a.mech")]
MAX_USER_MECHS = 2
MAX_JOBS = 16


def user_mech_tables():
    """The tables of the user slots, from MISTRA_USER_MECHS (unset: the demo tables; empty: none)."""
    env = os.environ.get("MISTRA_USER_MECHS")
    if env is None:      # the demo tables are derived from gas.mech and aer.mech, not committed (binary): written here where missing or stale
        from . import mechderive
        return mechderive.ensure_demo_tables()
    tables = [os.path.abspath(p) for p in env.split(":") if p]
    if len(tables) > MAX_USER_MECHS:
        raise RuntimeError("MISTRA_USER_MECHS names %d tables, there are %d user mechanism slots" % (len(tables), MAX_USER_MECHS))
    if len({os.path.splitext(os.path.basename(p))[0] for p in tables}) != len(tables):
        raise RuntimeError("MISTRA_USER_MECHS: the tables' names are the mechanisms' names, they must differ")
    return tables


def build_traits_gen(force=False, verbose=False):
    """-> path of the host program that writes a slot's traits header (user_traits_gen.cpp with the schedule compiler)"""
    os.makedirs(OBJDIR, exist_ok=True)
    exe = os.path.join(OBJDIR, "user_traits_gen")
    srcs = [os.path.join(CSRC, f) for f in USER_GEN_SOURCES]
    deps = srcs + [os.path.join(CSRC, f) for f in ("schedule.hpp", "mech_tables.hpp", "kernel_args.hpp")]
    if force or _stale(exe, deps):
        cmd = [hipcc(), "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", exe] + srcs
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return exe


def user_traits(table, slot, out, gen=None):
    """Runs the schedule compiler on `table` and writes the traits header of user slot `slot` to `out` -> the traits as a dict (integers, booleans,
    'NT', 'NAME', and 'WAVES_PER_SIMD' as the macro it names).  Raises RuntimeError with the generator's text where it refuses the table."""
    import re
    gen = gen or build_traits_gen()
    r = subprocess.run([gen, table, str(slot), out], stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("user mechanism slot %d: %s" % (slot, r.stderr.strip()))
    text = open(out).read()
    traits = {}
    for k, v in re.findall(r"\b([A-Z_]+) = (\w+)", text):
        traits[k] = {"true": True, "false": False}.get(v, int(v) if v.isdigit() else v)
    for k, v in re.findall(r"kUser\d(NT|LdsTotal|LdsAB|LdsJB|Temps) = (\d+)", text):
        traits[k] = int(v)
    traits["NAME"] = re.search(r'kUser\dName\[\] = "(\w+)"', text).group(1)
    return traits


def prepare_user_mechs(force=False, verbose=False):
    """Writes build/user_traits_<slot>.hpp for every slot and build/user_mechs.cfg (what the slots were built from); both only when their content
    changes, so that the units that include them are rebuilt exactly then.  -> (number of slots, the files)"""
    tables = user_mech_tables()
    files = []
    if tables:
        gen = build_traits_gen(force, verbose)
    for slot, table in enumerate(tables):
        tmp = os.path.join(OBJDIR, "user_traits_%d.hpp.new" % slot)
        final = os.path.join(OBJDIR, "user_traits_%d.hpp" % slot)
        files.append(final)
        if not force and not _stale(final, [table, gen]) and ('"%s"' % os.path.splitext(os.path.basename(table))[0]) in open(final).read():
            continue      # (written from this table by this generator)
        user_traits(table, slot, tmp, gen)
        if not os.path.exists(final) or open(final).read() != open(tmp).read():
            os.replace(tmp, final)
        else:
            os.remove(tmp)
    cfg = os.path.join(OBJDIR, "user_mechs.cfg")
    text = "".join("%d %s\n" % (i, os.path.splitext(os.path.basename(t))[0]) for i, t in enumerate(tables)) or "none\n"
    if not os.path.exists(cfg) or open(cfg).read() != text:
        with open(cfg, "w") as f:
            f.write(text)
    files.append(cfg)
    return len(tables), files


def kernel_units(n_user):
    """The kernel units of a library with n_user user slots: what build_lib compiles and checks, what tools/isa_compare.py lists."""
    return [PRODUCT] + VARIANT_UNITS + [Unit("user", slot, None) for slot in range(n_user)]


def unit_build(unit, incdir=None):
    """-> (source file, object name, flags) of a kernel unit.  Raises for a unit that does not exist: a VARIANT 3 unit of Ros3 (that kernel lives
    in the product unit), a trace unit of another method, a mechanism, method or slot out of range.  incdir: where a user slot's traits header
    lies (default the build directory; an edge twin has a directory of its own)."""
    variant, mech, method = unit
    if unit == PRODUCT:
        return PRODUCT_SOURCE, "ros3_kernel.o", []
    if variant == "user" and mech in range(MAX_USER_MECHS) and method is None:
        return USER_SOURCE, "ros_user_%d.o" % mech, ["-DMISTRA_USER_SLOT=%d" % mech, "-DMISTRA_USER_MECHS=%d" % (mech + 1), "-I" + (incdir or OBJDIR)]
    if variant not in VARIANT_METHODS or mech not in (0, 1, 2) or method not in VARIANT_METHODS[variant]:
        raise ValueError("no kernel unit %r: VARIANT -> methods %r on mechanisms 0 .. 2, the product unit, user slots 0 .. %d" %
                         (tuple(unit), VARIANT_METHODS, MAX_USER_MECHS - 1))
    return UNIT_SOURCE, "ros_unit_%d_%d_%d.o" % unit, ["-DMISTRA_UNIT_VARIANT=%d" % variant, "-DMISTRA_UNIT_MECH=%d" % mech, "-DMISTRA_UNIT_METHOD=%d" % method]


def unit_listing_cmd(unit, out, incdir=None):
    """-> the command that writes the gfx950 assembly of a kernel unit's device code to `out`, compiled as the build compiles it"""
    src, _, flags = unit_build(unit, incdir)
    return [hipcc(), "--offload-arch=" + ARCH] + [f for f in COMMON if f != "-fPIC"] + flags + ["-S", "--offload-device-only", os.path.join(CSRC, src), "-o", out]


def _jobs():
    return max(1, min(MAX_JOBS, os.cpu_count() or 1))


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd, verbose=False):
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)


def build_lib(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(OBJDIR, exist_ok=True)
    cc = hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))]
    headers.append(os.path.join(PKG, "..", "include", "mistra_chem.h"))
    headers.append(os.path.abspath(__file__))
    from concurrent.futures import ThreadPoolExecutor
    objs, cmds = [], []
    kernel_src = os.path.join(CSRC, PRODUCT_SOURCE)
    n_user, user_files = prepare_user_mechs(force, verbose)
    kunits = kernel_units(n_user)
    user_objs = {unit_build(u)[1] for u in kunits if u.variant == "user"}
    units = [(src, os.path.splitext(src)[0] + ".o", ["-DMISTRA_USER_MECHS=%d" % n_user, "-I" + OBJDIR] if src == "capi.cpp" else [],
              user_files if src == "capi.cpp" else []) for src in SOURCES]
    # (every kernel unit but the product's includes ros3_kernel.hip; a user slot's its generated traits header too)
    units += [unit_build(u) + (([] if u == PRODUCT else [kernel_src]) + (user_files if u.variant == "user" else []),) for u in kunits]
    if n_user:
        units.append(("capi.cpp", "capi_noslots.o", ["-DMISTRA_USER_MECHS=0", "-I" + OBJDIR], []))
    for src, name, flags, deps in units:
        path = os.path.join(CSRC, src)
        obj = os.path.join(OBJDIR, name)
        objs.append(obj)
        if force or _stale(obj, [path] + deps + headers):
            cmd = [cc, "--offload-arch=" + ARCH] + COMMON + flags + ["-c", path, "-o", obj]
            if src.endswith(".hip"):
                cmd += ["-Rpass-analysis=kernel-resource-usage"] if verbose else []
            cmds.append(cmd)
    with ThreadPoolExecutor(_jobs()) as pool:
        list(pool.map(lambda cmd: _run(cmd, verbose), cmds))
    noslots_objs = [o for o in objs if os.path.basename(o) not in user_objs and os.path.basename(o) != "capi.o"] if n_user else []
    objs = [o for o in objs if os.path.basename(o) != "capi_noslots.o"]
    if force or _stale(LIB, objs) or (n_user and _stale(LIB_NOSLOTS, noslots_objs)):
        # the look-ahead rings of ros3_kernel.hip sit in registers the compiler does not know are busy: no library is linked
        # from a kernel object in which a ring-using function's own registers reach its ring (raises).  Every code object that
        # holds the ring functions is checked: every kernel unit of the list.
        with ThreadPoolExecutor(_jobs()) as pool:
            reports = list(pool.map(lambda u: ring_register_report(unit=u), kunits))
        for u, isa in zip(kunits, reports):
            hits = isa_hazard_report(isa["__isa_text__"])
            if hits:
                raise RuntimeError("hazards the hardware does not interlock inside hand-written assembly (kernel unit %r):\n  " % (tuple(u),) + "\n  ".join(hits))
        _run([cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"], verbose)
        if n_user:
            _run([cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB_NOSLOTS] + noslots_objs + ["-ldl"])
    return LIB


def build_nochain_twin(force=False, verbose=False):
    """Links LIB_NOCHAIN from the objects build_lib has made (call it first): the library without user slots, with the product unit, tot's Rodas4 unit
    and the C ABI — which hands the kernels' trait to the schedule compiler — compiled once more with NOCHAIN_FLAG (the
    product unit then holds the instructions it had before there were chain passes)."""
    cc = hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))] + [os.path.abspath(__file__)]
    kernel_src = os.path.join(CSRC, PRODUCT_SOURCE)
    twins = {}      # object of build_lib -> (source, flags) of its twin
    for u in (PRODUCT, NOCHAIN_UNIT):
        src, name, flags = unit_build(u)
        twins[name] = (src, flags)
    twins["capi.o"] = ("capi.cpp", ["-DMISTRA_USER_MECHS=0", "-I" + OBJDIR])
    objs, cmds = [], []
    for name in [os.path.splitext(s)[0] + ".o" for s in SOURCES] + [unit_build(u)[1] for u in kernel_units(0)]:
        if name not in twins:
            objs.append(os.path.join(OBJDIR, name))
            continue
        src, flags = twins[name]
        obj = os.path.join(OBJDIR, "nochain_" + name)      # (not ros_unit_*.o: the variant and diagnostic builds link that pattern)
        objs.append(obj)
        if force or _stale(obj, [os.path.join(CSRC, src), kernel_src] + headers):
            cmds.append([cc, "--offload-arch=" + ARCH] + COMMON + flags + [NOCHAIN_FLAG, "-c", os.path.join(CSRC, src), "-o", obj])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(_jobs()) as pool:
        list(pool.map(lambda cmd: _run(cmd, verbose), cmds))
    if force or _stale(LIB_NOCHAIN, objs):
        _run([cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB_NOCHAIN] + objs + ["-ldl"], verbose)
    return LIB_NOCHAIN


# ---- the edge twins: the library with tables at the edges of the user slots' size classes in its two slots (mistra_amd/mechderive.py:
# EDGE_TABLES), what tests/test_gpu_user_edges.py runs in child processes.  Nothing loads them otherwise.  edge_a128 (one wave per cell WITH a
# scaling pass) sits apart from edge_g64 and edge_a129, so that those two do not depend on its unit passing the ring-register check.
EDGE_TWINS = collections.OrderedDict([("edge0", ("edge_g64", "edge_a129")), ("edge1", ("edge_a128", "edge_t417"))])


def edge_twin_lib(twin):
    return os.path.join(LIBDIR, "libmistra_chem_%s.so" % twin)


def edge_twin_dir(twin):
    """where a twin's traits headers, its two user units and its capi.o lie: the product's build/user_traits_*.hpp and user_mechs.cfg stay as they are"""
    return os.path.join(OBJDIR, twin)


def build_edge_twins(force=False, verbose=False):
    """Links the edge twins from the objects build_lib has made (call it first): every object of the product but the two user units and capi.o, which
    are compiled against the twin's own traits headers in edge_twin_dir.  The ring-register and hazard checks run on a twin's user units before it is
    linked, as build_lib runs them on the product's.  -> the libraries' paths"""
    from concurrent.futures import ThreadPoolExecutor
    from . import mechderive
    tables = mechderive.ensure_edge_tables()
    cc = hipcc()
    gen = build_traits_gen(force, verbose)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))]
    headers += [os.path.join(PKG, "..", "include", "mistra_chem.h"), os.path.abspath(__file__)]
    kernel_src = os.path.join(CSRC, PRODUCT_SOURCE)
    shared = [os.path.splitext(s)[0] + ".o" for s in SOURCES if s != "capi.cpp"] + [unit_build(u)[1] for u in kernel_units(0)]
    libs = []
    for twin, names in EDGE_TWINS.items():
        tdir = edge_twin_dir(twin)
        os.makedirs(tdir, exist_ok=True)
        traits = []
        for slot, name in enumerate(names):
            final, tmp = os.path.join(tdir, "user_traits_%d.hpp" % slot), os.path.join(tdir, "user_traits_%d.hpp.new" % slot)
            traits.append(final)
            if not force and not _stale(final, [tables[name], gen]) and ('"%s"' % name) in open(final).read():
                continue
            user_traits(tables[name], slot, tmp, gen)
            if not os.path.exists(final) or open(final).read() != open(tmp).read():
                os.replace(tmp, final)
            else:
                os.remove(tmp)
        uunits = [Unit("user", slot, None) for slot in range(len(names))]
        own = [("capi.cpp", "capi.o", ["-DMISTRA_USER_MECHS=%d" % len(names), "-I" + tdir], traits)]
        own += [unit_build(u, tdir) + ([kernel_src] + traits,) for u in uunits]
        objs, cmds = [os.path.join(OBJDIR, name) for name in shared], []
        for src, name, flags, deps in own:
            obj = os.path.join(tdir, name)
            objs.append(obj)
            if force or _stale(obj, [os.path.join(CSRC, src)] + deps + headers):
                cmds.append([cc, "--offload-arch=" + ARCH] + COMMON + flags + ["-c", os.path.join(CSRC, src), "-o", obj])
        with ThreadPoolExecutor(_jobs()) as pool:
            list(pool.map(lambda cmd: _run(cmd, verbose), cmds))
        lib = edge_twin_lib(twin)
        if force or _stale(lib, objs):
            with ThreadPoolExecutor(_jobs()) as pool:
                reports = list(pool.map(lambda u: ring_register_report(unit=u, incdir=tdir), uunits))
            for u, isa in zip(uunits, reports):
                hits = isa_hazard_report(isa["__isa_text__"])
                if hits:
                    raise RuntimeError("hazards the hardware does not interlock inside hand-written assembly (%s, kernel unit %r):\n  " % (twin, tuple(u)) + "\n  ".join(hits))
            _run([cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs + ["-ldl"], verbose)
        libs.append(lib)
    return libs


# the non-inlined device functions of ros3_kernel.hip in which table loads are in flight in the look-ahead ring (their last template
# argument is the ring's placement).  In gsum_run_pair a FILLED ring outlives compiler code: the statements between its two programs.
RING_FUNCTIONS = ("gsum_run", "gsum_run_bar", "gsum_run_pair", "gsum_pass_run", "tail_solve", "scale_run")
RING_HIGH_SLOTS = (192, 196, 208, 212, 224, 228, 240, 244)      # ros3_kernel.hip: MISTRA_RING_HI<K>


def ring_register_report(isa_path=None, unit=PRODUCT, incdir=None):
    """Checks the one assumption the table look-ahead ring of ros3_kernel.hip rests on (see the comment there): in the
    non-inlined device functions, every register the COMPILER allocates — named outside inline asm, or chosen by it for an asm
    statement's result — stays below the ring's blocks (v192.. or, in the low placement, v64..), so a
    table load landing in the ring can never hit a compiler value.  Compiles the kernel source to gfx950 assembly and
    scans it.  Returns {function: highest VGPR named outside inline asm}; raises if a ring-using function reaches its ring, and if
    a function that is not one of RING_FUNCTIONS (nor an integrating kernel, which only calls them) loads into the ring at all.
    unit: one of kernel_units() (a user slot's traits header must be in the build directory: prepare_user_mechs — or in `incdir`, an edge twin's
    directory); default the product kernels' unit."""
    import re
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        if isa_path is None:
            isa_path = os.path.join(tmp, "unit.s")
            subprocess.run(unit_listing_cmd(unit, isa_path, incdir), check=True, stderr=subprocess.DEVNULL)
        lines = open(isa_path).read().split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN6mistra.*:", l)]
    starts.append((len(lines), "end"))
    report = {}
    ring_users = set()
    for (i, name), (j, _) in zip(starts, starts[1:]):
        in_asm, hi = False, 0
        for l in lines[i:j]:
            if "ASMSTART" in l:
                in_asm = True
            elif "ASMEND" in l:
                in_asm = False
            elif in_asm and re.search(r"global_load_dwordx4 v\[(64|192):\d+\], v\[\d+:\d+\], off", l):
                ring_users.add(name)         # the function issues ring loads (vm_ring_load) itself; (vm_run's own ring is
                                             # loaded and consumed inside ONE asm statement that lists it as clobbered)
            elif in_asm and re.search(r"global_load_dwordx4 v\[(%s):\d+\]," % "|".join(map(str, RING_HIGH_SLOTS)), l):
                ring_users.add(name)         # any load into the high placement, whatever its address form (the generated streams,
                                             # the tail chain's scalar-base loads): nothing else lives up there
            elif "Folded Spill" in l or "Folded Reload" in l:
                pass    # prologue / epilogue saves of callee-saved ring blocks: before the first ring load, after the drain
            elif not in_asm and not l.strip().startswith((";", ".")):
                for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", l):
                    hi = max(hi, int(m.group(1) or m.group(3)))
            elif in_asm and not l.strip().startswith((";", ".")):
                # inside asm: the destination the compiler chose for an asm result (an LDS gather, a multiply-add...) — every value
                # of the compiler's is written either outside asm or here; the ring loads' own destinations and the ring registers
                # read as sources (gather addresses, table words) are the ring itself
                t = l.split(";")[0].strip().split(None, 1)
                if len(t) == 2 and t[0].startswith("v_") or len(t) == 2 and t[0].startswith("ds_read"):
                    m = re.match(r"\s*(?:v(\d+)\b|v\[(\d+):(\d+)\])", t[1])
                    if m:
                        hi = max(hi, int(m.group(1) or m.group(3)))
        report[name] = hi
        low = re.search(r"\d(%s)I.*Lb([01])E+[A-Z]" % "|".join(RING_FUNCTIONS), name)       # last template argument: ring placement LOW
        if low:
            limit = 64 if low.group(2) == "1" else 192
            if hi >= limit:
                raise RuntimeError("%s: the compiler allocates v%d, inside the look-ahead ring's register blocks (v%d..)" % (name, hi, limit))
        elif name in ring_users and "ros3_integrate_kernel" not in name:
            raise RuntimeError("%s issues look-ahead ring loads but is not covered by the register check" % name)
    report["__isa_text__"] = "\n".join(lines)
    return report


# ---- hazards inside hand-written assembly.  The compiler's hazard recogniser and its s_waitcnt insertion do not look inside asm statements,
#      and ros3_kernel.hip carries ~4 000 lines of hand-written / generated instructions (vm_exec_asm.inc, gsum_exec_asm.inc, the ring
#      helpers, the DPP chains).  Three classes are checked on the ISA the compiler emits, each the cause of a wrong result or a GPU
#      memory fault met while those were written:
#   (i)   an SGPR written by v_readfirstlane / v_readlane and used as the scalar base of a vector-memory instruction less than 5 wait
#         states later (round 3: a table base moved to scalar registers in front of a global_load -> memory access fault);
#   (ii)  a DPP instruction whose DPP-read source (src0) was written by a VALU instruction less than 2 wait states earlier (the hardware
#         does not interlock the read: tools/ubench/dpp.hip returns wrong sums with none);
#   (iii) an `s_waitcnt vmcnt(N)` inside an asm block with N not below the number of distinct registers-in-flight slots of its ring (such
#         a wait can never guarantee that the oldest slot has landed): the slots the block's own loads fill where it issues loads (an
#         executor that streams its ring inside one statement: vm_exec_asm.inc, gsum_exec_asm.inc), else the slots all asm loads of the
#         function fill (a ring loaded and waited for by separate statements: the ring helpers, the tail chain).  Per block, not per
#         function: an integrating kernel inlines rings of several depths, whose union would pass a wait too deep for the smaller one.
# An instruction is one wait state, `s_nop N` is N + 1.  The scan is linear per function (labels are ignored: conservative for the
# straight-line blocks these sequences are).
def isa_hazard_report(isa_text, sgpr_vmem_wait=5, dpp_wait=2, seen=None):
    """-> list of findings (empty = clean).  seen: optional dict that receives how many instructions of each class were examined."""
    import re
    hits = []
    seen = seen if seen is not None else {}
    for k in ("vmem_scalar_base", "dpp", "vmcnt", "functions"):
        seen.setdefault(k, 0)
    func, insts = None, []

    def regs(tok, kind):
        """register numbers named by an operand token of class `kind` ('s' or 'v'): s3, s[2:3], -v[4:5], |v7| ..."""
        tok = tok.strip().lstrip("-").strip("|")
        m = re.match(r"^%s(\d+)$" % kind, tok)
        if m:
            return {int(m.group(1))}
        m = re.match(r"^%s\[(\d+):(\d+)\]$" % kind, tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        return set()

    def flush():
        if func is None:
            return
        seen["functions"] += 1
        loads = [i for i in insts if i["asm"] and i["op"].startswith(("global_load", "buffer_load")) and i["ops"]]
        depth = len({i["ops"][0] for i in loads})
        block_depth = {}
        for i in loads:
            block_depth.setdefault(i["block"], set()).add(i["ops"][0])
        for n, it in enumerate(insts):
            if not it["asm"]:
                continue
            op, ops = it["op"], it["ops"]
            if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
                base = set()
                for o in ops:
                    if re.match(r"^s\[\d+:\d+\]$", o.strip()):
                        base |= regs(o, "s")
                if base:
                    seen["vmem_scalar_base"] += 1
                    waited, k = 0, n - 1
                    while k >= 0 and waited < sgpr_vmem_wait:
                        p = insts[k]
                        if p["op"] in ("v_readfirstlane_b32", "v_readlane_b32") and p["ops"] and regs(p["ops"][0], "s") & base:
                            hits.append("%s: line %d `%s` reads a scalar base written by `%s` %d wait state(s) earlier (needs %d)" %
                                        (func, it["line"], it["text"], p["text"], waited, sgpr_vmem_wait))
                            break
                        waited += p["wait"]
                        k -= 1
            if "_dpp" in op or re.search(r"\b(row_newbcast|row_shr|row_shl|row_ror|row_bcast|quad_perm|row_mirror|row_half_mirror|row_share|row_xmask):?", it["text"]):
                src0 = regs(ops[1], "v") if len(ops) > 1 else set()
                seen["dpp"] += 1
                waited, k = 0, n - 1
                while src0 and k >= 0 and waited < dpp_wait:
                    p = insts[k]
                    if p["op"].startswith("v_") and p["ops"] and regs(p["ops"][0], "v") & src0:
                        hits.append("%s: line %d `%s` DPP-reads a register written by `%s` %d wait state(s) earlier (needs %d)" %
                                    (func, it["line"], it["text"], p["text"], waited, dpp_wait))
                        break
                    waited += p["wait"]
                    k -= 1
            if op == "s_waitcnt" and depth:
                m = re.search(r"vmcnt\((\d+)\)", it["text"])
                seen["vmcnt"] += 1 if m else 0
                own = len(block_depth.get(it["block"], ()))
                if m and int(m.group(1)) >= (own or depth):
                    hits.append("%s: line %d `%s` waits for at most %s loads in flight, %s fill only %d slots" %
                                (func, it["line"], it["text"], m.group(1), "its asm block's loads" if own else "the function's asm loads",
                                 own or depth))

    in_asm, block = False, 0
    for ln, raw in enumerate(isa_text.split("\n"), 1):
        if re.match(r"^[A-Za-z_.$][\w.$]*:", raw) and not raw.startswith(".L"):
            flush()
            func, insts, in_asm = raw.split(":")[0], [], False
            continue
        if "ASMSTART" in raw:
            in_asm, block = True, block + 1
            continue
        if "ASMEND" in raw:
            in_asm = False
            continue
        t = raw.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        op = parts[0]
        ops = [o.strip() for o in re.split(r",(?![^\[]*\])", parts[1].split(" offset")[0])] if len(parts) > 1 else []
        # modifiers that follow the last operand without a comma (row_newbcast:3 row_mask:0x1 ...) stay glued to it: cut them off
        ops = [o.split()[0] if o.split() else o for o in ops]
        wait = 1
        if op == "s_nop" and ops:
            wait = int(ops[0], 0) + 1
        insts.append({"op": op, "ops": ops, "asm": in_asm, "block": block if in_asm else 0, "line": ln, "text": t, "wait": wait})
    flush()
    return hits


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
    print(build_nochain_twin(force="--force" in sys.argv, verbose=True))
    print(build_edge_twins(force="--force" in sys.argv, verbose=True))
