#!/usr/bin/env python3
"""Function-by-function comparison of two gfx950 assembly listings of the integrator's translation unit (hipcc -S --offload-device-only of
mistra_amd/csrc/ros3_kernel.hip at two commits), and the resources of the method kernels' code objects.

    python tools/isa_compare.py PARENT.s NEW.s      per function: instructions in both, whether the bodies are identical
    python tools/isa_compare.py --methods           per method unit (mistra_amd/build.py: METHOD_UNITS): the kernel's registers, scratch and LDS
                                                    from the code object's metadata, compiled here as the build compiles them
    python tools/isa_compare.py --series            per series unit (SERIES_UNITS): the same figures of the series kernel (VARIANT 5) beside its VARIANT 3
                                                    sibling's — the product unit's options kernel for Ros3, the method unit's for the other four
    python tools/isa_compare.py --flux              per flux unit (FLUX_UNITS): the same table for the flux kernel (VARIANT 6)

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


def methods():
    from mistra_amd import build as B
    names = {1: "Ros2", 3: "Ros4", 4: "Rodas3", 5: "Rodas4"}
    print("%-5s %-7s %6s %6s %8s %12s %10s  (LDS: dynamic, set at launch: LdsLayout<MT, NT>::TOTAL doubles, as the product kernels)" %
          ("mech", "method", "VGPRs", "SGPRs", "scratch", "spilled VGPR", "static LDS"))
    with tempfile.TemporaryDirectory() as tmp:
        for mech, method in B.METHOD_UNITS:
            s = os.path.join(tmp, "u.s")
            cmd = [B.hipcc(), "--offload-arch=" + B.ARCH] + [f for f in B.COMMON if f != "-fPIC"] + B.method_flags(mech, method) + \
                  ["-S", "--offload-device-only", os.path.join(B.CSRC, B.METHOD_SOURCE), "-o", s]
            subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
            text = open(s).read()
            k = re.search(r"- \.agpr_count:.*?\.name:\s+(\S*ros3_integrate_kernel\S*).*?(?=\n  - \.agpr_count|\namdhsa\.target)", text, re.S).group(0)
            get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
            print("%-5s %-7s %6d %6d %8d %12d %10d" % (("gas", "aer", "tot")[mech], names[method], get("vgpr_count"), get("sgpr_count"),
                                                        get("private_segment_fixed_size"), get("vgpr_spill_count"), get("group_segment_fixed_size")))


def _kernels(path):
    """[(kernel name, {metadata key: value})] of a listing's code object metadata"""
    text = open(path).read()
    out = []
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count|\namdhsa\.target)", text, re.S):
        k = m.group(0)
        out.append((re.search(r"\.name:\s+(\S+)", k).group(1), {key: int(v) for key, v in re.findall(r"\.(\w+):\s+(\d+)\n", k)}))
    return out


def series(variant=5, what="series"):
    from mistra_amd import build as B
    units, source, flags_of = (B.SERIES_UNITS, B.SERIES_SOURCE, B.series_flags) if variant == 5 else (B.FLUX_UNITS, B.FLUX_SOURCE, B.flux_flags)
    names = {1: "Ros2", 2: "Ros3", 3: "Ros4", 4: "Rodas3", 5: "Rodas4"}
    mechs = ("gas", "aer", "tot")
    cols = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
    print("%-4s %-7s | %-40s | %s" % ("mech", "method", "VARIANT 3 (the options kernel)", "VARIANT %d (the %s kernel)" % (variant, what)))
    print("%-4s %-7s | %5s %5s %8s %7s %10s | %5s %5s %8s %7s %10s   (LDS: dynamic, LdsLayout<MT, NT>::TOTAL doubles, the same for both)" %
          (("", "") + ("VGPRs", "SGPRs", "scratch", "spilled", "static LDS") * 2))
    with tempfile.TemporaryDirectory() as tmp:
        def listing(src, flags):
            s = os.path.join(tmp, "u.s")
            cmd = [B.hipcc(), "--offload-arch=" + B.ARCH] + [f for f in B.COMMON if f != "-fPIC"] + flags + ["-S", "--offload-device-only", os.path.join(B.CSRC, src), "-o", s]
            subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
            return _kernels(s)
        product = listing("ros3_kernel.hip", [])
        for mech, method in units:
            if method == 2:
                sib = [k for n, k in product if re.search(r"ros3_integrate_kernelINS_\d+%sTraitsELi\d+ELi3ELi2E" % mechs[mech].capitalize(), n)]
            else:
                sib = [k for n, k in listing(B.METHOD_SOURCE, B.method_flags(mech, method)) if "ros3_integrate_kernel" in n]
            new = [k for n, k in listing(source, flags_of(mech, method)) if "ros3_integrate_kernel" in n]
            assert len(sib) == 1 and len(new) == 1, (mech, method, len(sib), len(new))
            print("%-4s %-7s | %5d %5d %8d %7d %10d | %5d %5d %8d %7d %10d" % ((mechs[mech], names[method]) + tuple(sib[0][c] for c in cols) + tuple(new[0][c] for c in cols)))


if __name__ == "__main__":
    if "--methods" in sys.argv:
        methods()
    elif "--series" in sys.argv:
        series()
    elif "--flux" in sys.argv:
        series(6, "flux")
    else:
        sys.exit(0 if compare(sys.argv[1], sys.argv[2]) else 1)
