#!/usr/bin/env python3
"""Are the kernels of two device-only assembly listings the same machine code?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include --cuda-device-only -S csrc/FILE.hip -o FILE.s      (both trees)
    python tools/compare_device_asm.py PARENT_DIR CHANGE_DIR            compares every *.s the two directories share

A host-side change must leave every kernel as it was.  Compared per kernel symbol, so that a changed order of template
instantiation does not count: the body (label .. .Lfunc_end) and the .amdhsa_kernel block, with the per-function numbers of the
local labels (.LBB<n>_, .Lfunc_end<n>, ...) replaced and the comments dropped.  Exit status 1 on any difference."""
import glob
import os
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.S | re.M)
        code = re.sub(r"(\.L[A-Za-z_]+)\d+", r"\1N", re.sub(r"\s*;.*", "", body.group(0))) if body else None
        out[name] = (code, m.group(2))
    return out


def main(parent, change):
    bad = 0
    for p in sorted(glob.glob(os.path.join(parent, "*.s"))):
        c = os.path.join(change, os.path.basename(p))
        if not os.path.exists(c):
            continue
        kp, kc = kernels(p), kernels(c)
        differ = sorted(set(kp) ^ set(kc)) + sorted(k for k in set(kp) & set(kc) if kp[k] != kc[k] or kp[k][0] is None)
        same_text = [l for l in open(p) if "__hip_cuid_" not in l] == [l for l in open(c) if "__hip_cuid_" not in l]
        print("%-28s %3d kernels: %s%s" % (os.path.basename(p), len(kp), "DIFFERENT: %s" % differ if differ else "identical",
                                           "" if differ else (" (whole listing)" if same_text else " (per kernel; order changed)")))
        bad += len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
