#!/usr/bin/env python3
"""Compare two device assembly files (tools/kernel_isa.sh) kernel by kernel: tools/isa_diff.py OLD.s NEW.s
Bodies are compared without comments, empty lines and the numbers of function-local labels (these only encode the order in
which functions were emitted).  Only the instructions between a symbol's label and its .Lfunc_end are compared: the .amdhsa
kernel descriptors (registers, scratch, LDS) are not — tools/kernel_resources.py prints those.  Prints the symbols only one file has and the symbols whose bodies differ; exit status 1 if
NEW has a symbol OLD lacks or any common body differs."""
import re, sys


def bodies(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if name is None:
            if m: name = m.group(1); out[name] = []
            continue
        if line.startswith(".Lfunc_end"): name = None; continue
        s = line.split(";")[0].strip()
        if s: out[name].append(re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1", s))
    return out


old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
for k in gone: print("only in", sys.argv[1], k)
for k in added: print("only in", sys.argv[2], k)
for k in differ: print("differs", k)
print(f"{len(old)} -> {len(new)} symbols, {len(gone)} dropped, {len(added)} added, {len(differ)} differing bodies")
sys.exit(1 if added or differ else 0)
