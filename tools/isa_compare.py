#!/usr/bin/env python3
"""Function-by-function comparison of two gfx950 assembly listings of the integrator's translation unit (hipcc -S --offload-device-only of
mistra_amd/csrc/ros3_kernel.hip at two commits), and the resources of the method kernels' code objects.

    python tools/isa_compare.py PARENT.s NEW.s      per function: instructions in both, whether the bodies are identical
    python tools/isa_compare.py --listings DIR      the listing of every kernel unit (mistra_amd/build.py: kernel_units) into DIR, one .s each: run at
                                                    two commits and compare the files pairwise
    python tools/isa_compare.py --methods           per method unit (VARIANT_UNITS, variant 3): the kernel's registers, scratch and LDS
                                                    from the code object's metadata, compiled here as the build compiles them
    python tools/isa_compare.py --series            per series unit (variant 5): the same figures of the series kernel beside its VARIANT 3
                                                    sibling's — the product unit's options kernel for Ros3, the method unit's for the other four
    python tools/isa_compare.py --flux              per flux unit (variant 6): the same table for the flux kernel
    python tools/isa_compare.py --dense             per series unit: the same table for the dense-output kernel (VARIANT 7) the unit also holds
    python tools/isa_compare.py --ops               per trace unit: the same table for the operator kernel (VARIANT 8) the unit also holds

A kernel's mangled name carries its template arguments: the METHOD parameter added to ros3_integrate_kernel (default Ros3 = 2) is cut out of the
new listing's names before the comparison; nothing else is normalised."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mistra_amd import build as B  # noqa: E402


def functions(path):
    """{symbol: [instruction lines]} of a listing: labels at column 0 up to .Lfunc_end, comments and directives dropped"""
    text = open(path).read()
    text = re.sub(r"(ros3_integrate_kernelINS_\d+[A-Za-z]+TraitsELi\d+ELi[0-3])ELi2E", r"\1E", text)
    out, name = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(_Z[\w.$]+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        t = line.split(";")[0].strip()
        if name and t and not t.startswith("."):
            out[name].append(t)
    return out


def compare(a, b):
    fa, fb = functions(a), functions(b)
    names = sorted(set(fa) | set(fb))
    same = 0
    print("%-12s %-12s %-10s function" % ("parent", "new", "identical"))
    for n in names:
        x, y = fa.get(n), fb.get(n)
        eq = x is not None and y is not None and hashlib.sha256("\n".join(x).encode()).digest() == hashlib.sha256("\n".join(y).encode()).digest()
        same += eq
        print("%-12s %-12s %-10s %s" % ("-" if x is None else len(x), "-" if y is None else len(y), "yes" if eq else "NO", n))
    print("%d functions, %d identical instruction for instruction, %d differ or exist on one side only" % (len(names), same, len(names) - same))
    return same == len(names)


NAMES = {1: "Ros2", 2: "Ros3", 3: "Ros4", 4: "Rodas3", 5: "Rodas4"}
MECHS = ("gas", "aer", "tot")
COLS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")


def _kernels(path):
    """[(kernel name, {metadata key: value})] of a listing's code object metadata"""
    text = open(path).read()
    out = []
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count|\namdhsa\.target)", text, re.S):
        k = m.group(0)
        out.append((re.search(r"\.name:\s+(\S+)", k).group(1), {key: int(v) for key, v in re.findall(r"\.(\w+):\s+(\d+)\n", k)}))
    return out


def unit_name(unit):
    """file name of a kernel unit's listing: product | v<variant>_<mech>_<method> | user_<slot>"""
    return unit.variant if unit == B.PRODUCT else "user_%d" % unit.mech if unit.variant == "user" else "v%d_%s_%s" % (unit.variant, MECHS[unit.mech], NAMES[unit.method])


def listing(unit, path):
    """the gfx950 assembly of a kernel unit (mistra_amd/build.py: kernel_units), compiled as the build compiles it -> path"""
    subprocess.run(B.unit_listing_cmd(unit, path), check=True, stderr=subprocess.DEVNULL)
    return path


def listings(outdir):
    """one .s per kernel unit of the library as it is configured (MISTRA_USER_MECHS), to be compared pairwise with another commit's"""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(outdir, exist_ok=True)
    units = B.kernel_units(B.prepare_user_mechs()[0])
    with ThreadPoolExecutor(B._jobs()) as pool:
        for path in pool.map(lambda u: listing(u, os.path.join(outdir, unit_name(u) + ".s")), units):
            print(path)


def _integrator(unit, tmp, variant=None):
    """the metadata of the integrating kernel of a variant unit: the unit's own VARIANT, or the dense-output kernel (variant=7) a series unit also holds"""
    tag = "ELi%dELi%dEEEv" % (variant or unit.variant, unit.method)
    ks = [k for n, k in _kernels(listing(unit, os.path.join(tmp, "u.s"))) if "ros3_integrate_kernel" in n and tag in n]
    assert len(ks) == 1, (unit, variant, len(ks))
    return ks[0]


def methods():
    print("%-5s %-7s %6s %6s %8s %12s %10s  (LDS: dynamic, set at launch: LdsLayout<MT, NT>::TOTAL doubles, as the product kernels)" %
          ("mech", "method", "VGPRs", "SGPRs", "scratch", "spilled VGPR", "static LDS"))
    with tempfile.TemporaryDirectory() as tmp:
        for u in (u for u in B.VARIANT_UNITS if u.variant == 3):
            k = _integrator(u, tmp)
            print("%-5s %-7s %6d %6d %8d %12d %10d" % ((MECHS[u.mech], NAMES[u.method]) + tuple(k[c] for c in COLS)))


def beside_variant_3(variant, what, kernel=None):
    """per unit of `variant`: the figures of its kernel (kernel: of the VARIANT `kernel` instantiation it also holds) beside its VARIANT 3 sibling's"""
    print("%-4s %-7s | %-40s | %s" % ("mech", "method", "VARIANT 3 (the options kernel)", "VARIANT %d (the %s kernel)" % (kernel or variant, what)))
    print("%-4s %-7s | %5s %5s %8s %7s %10s | %5s %5s %8s %7s %10s   (LDS: dynamic, LdsLayout<MT, NT>::TOTAL doubles, the same for both)" %
          (("", "") + ("VGPRs", "SGPRs", "scratch", "spilled", "static LDS") * 2))
    with tempfile.TemporaryDirectory() as tmp:
        product = _kernels(listing(B.PRODUCT, os.path.join(tmp, "p.s")))
        for u in (u for u in B.VARIANT_UNITS if u.variant == variant):
            if u.method == B.ROS3:
                sib, = [k for n, k in product if re.search(r"ros3_integrate_kernelINS_\d+%sTraitsELi\d+ELi3ELi2E" % MECHS[u.mech].capitalize(), n)]
            else:
                sib = _integrator(u._replace(variant=3), tmp)
            new = _integrator(u, tmp, kernel)
            print("%-4s %-7s | %5d %5d %8d %7d %10d | %5d %5d %8d %7d %10d" % ((MECHS[u.mech], NAMES[u.method]) + tuple(sib[c] for c in COLS) + tuple(new[c] for c in COLS)))


if __name__ == "__main__":
    if "--methods" in sys.argv:
        methods()
    elif "--series" in sys.argv:
        beside_variant_3(5, "series")
    elif "--flux" in sys.argv:
        beside_variant_3(6, "flux")
    elif "--dense" in sys.argv:
        beside_variant_3(5, "dense-output", kernel=7)
    elif "--ops" in sys.argv:
        beside_variant_3(4, "operator", kernel=8)
    elif "--listings" in sys.argv:
        listings(sys.argv[sys.argv.index("--listings") + 1])
    else:
        sys.exit(0 if compare(sys.argv[1], sys.argv[2]) else 1)
