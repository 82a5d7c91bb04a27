"""Per kernel instantiation, two builds of the same sources side by side (old / new, `!` where they differ): registers, LDS and scratch
from the compiler's kernel-info comments, and the counts of double-precision arithmetic, LDS and barrier instructions in the device
assembly.  No GPU needed.  Made for refactors that must leave the machine code as it was (profiles/frame_ssim_resources.txt).

    for n in frame_metric frame_msssim; do       # in csrc/ of each checkout, with the Makefile's flags for the source
        hipcc -O3 -fPIC -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S $n.hip -o <dir>/$n.s
    done
    python tools/kernel_resources.py <old dir> <new dir> frame_metric frame_msssim
"""
import re
import sys
from collections import OrderedDict

CLASSES = (("f64 fma/fmac", ("v_fma_f64", "v_fmac_f64")), ("f64 mul", ("v_mul_f64",)), ("f64 add", ("v_add_f64",)),
           ("f64 div*", ("v_div_", "v_rcp_f64")), ("ds_*", ("ds_",)), ("s_barrier", ("s_barrier",)))
INFO = (("VGPR", "NumVgprs"), ("AGPR", "NumAgprs"), ("SGPR", "TotalNumSgprs"), ("LDS B", "LDSByteSize"), ("scratch B", "ScratchSize"))


def short(mangled):
    """k_name<1,0,...> from the mangled name of a kernel whose template arguments are bools."""
    k = re.search(r"\d+(k_[a-z0-9_]+?)(?=I|E|P|v)", mangled).group(1)
    bools = re.findall(r"Lb([01])E", mangled.split(k, 1)[1].split("EEv", 1)[0]) if k + "ILb" in mangled else []
    return k + ("<" + ",".join(bools) + ">" if bools else "")


def kernels(path):
    text = open(path).read()
    out = OrderedDict()
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:\n\t\.size\t\1,.*?; Kernel info:(.*?)\n\t\.", text, re.S | re.M):
        if ".amdhsa_kernel " + m.group(1) + "\n" not in text:
            continue   # (a device function, not a kernel)
        ins = [ln.split()[0] for ln in m.group(0).split("; Kernel info:")[0].splitlines()
               if ln.startswith("\t") and not ln.startswith(("\t.", "\t;")) and ln.split()]
        row = OrderedDict((name, int(re.search(r"; " + pat + r": (\d+)", m.group(2)).group(1))) for name, pat in INFO)
        for name, prefixes in CLASSES:
            row[name] = sum(i.startswith(prefixes) for i in ins)
        row["insts"] = len(ins)
        out[short(m.group(1))] = row
    return out


old_dir, new_dir, names = sys.argv[1], sys.argv[2], sys.argv[3:]
for name in names:
    old, new = kernels(f"{old_dir}/{name}.s"), kernels(f"{new_dir}/{name}.s")
    assert sorted(old) == sorted(new), (sorted(old), sorted(new))
    cols = list(next(iter(old.values())))
    print(f"{name}.hip: old / new")
    print(f"  {'kernel':20s}" + "".join(f"{c:>14s}" for c in cols))
    for k in old:
        print(f"  {k:20s}" + "".join(f"{str(old[k][c]) + '/' + str(new[k][c]) + ('' if old[k][c] == new[k][c] else '!'):>14s}" for c in cols))
    print()
