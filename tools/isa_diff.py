#!/usr/bin/env python3
"""Which kernels' machine code differs between two hipcc -S outputs (--cuda-device-only -S, or --save-temps):
python tools/isa_diff.py before.s after.s [old_symbol=new_symbol ...]
Labels, comments and the translation unit's id are normalised away; symbol pairs map kernels that were renamed (e.g. made templates).
Either file may be several outputs concatenated (one source split into several): a symbol that comes more than once --
a library kernel instantiated in two translation units -- must have the same body every time ("repeated" otherwise)."""
import re
import sys


def bodies(path):
    out, cur, buf = {}, None, []
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, buf = m.group(1), []
            continue
        if cur and (re.match(r"^\.Lfunc_end", line) or line.startswith("\t.section")):
            if out.setdefault(cur, buf) != buf:
                print("repeated", cur, "in", path, "with another body")
            cur = None
            continue
        if cur:
            t = line.split(";")[0].strip()
            if t:
                t = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", t)       # (the translation unit's id: it trails the last data object)
                buf.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
ren = dict(x.split("=", 1) for x in sys.argv[3:])
same = 0
for k, v in sorted(a.items()):
    k2 = ren.get(k, k)
    if k2 not in b:
        print("gone    ", k)
    elif v == b[k2]:
        same += 1
    else:
        print("differs ", k, len(v), "->", len(b[k2]), "instructions")
for k in sorted(set(b) - set(ren.get(x, x) for x in a)):
    print("new     ", k)
print("identical:", same)
