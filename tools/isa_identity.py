#!/usr/bin/env python
"""Development (no GPU): is the gfx950 device code of a translation unit the same text as at another revision?  The check a refactor
of kernel sources is held to (profiles/*_isa_identity.txt).
    python tools/isa_identity.py UNIT... [REV] [-DFLAG ...]     UNIT: pf_main, pf_col_f32, ... ; REV: default HEAD
Each unit is compiled from the working tree and from REV - each with its own tree's recipe - by the library's compile line plus
-save-temps, a fixed -DPF_SOURCE_SHA256 and the flags given (arguments that start with '-': -DPF_DEVTOOLS, -DPFK_ISA_MARKS).  The
gfx950 listing is split into per-symbol bodies (-- Begin function / -- End function), ';' comments are dropped, .LBB* / .Ltmp* /
.Lfunc_end* / .Lpost_getpc* labels are renumbered per body in order of first appearance, and every .amdhsa_kernel descriptor block
becomes an entry of its own.  Printed per unit: entries / same keys / differing, and the demangled names that differ.  It compares
text and looks for nothing in particular.  Exit status 1 when any unit differs.
NOT compared: what lies outside the function bodies and descriptors - data sections (.rodata constants, __constant__ tables), LDS
symbol sizes and the amdhsa.kernels metadata.  A change to device-side tables needs a look of its own."""
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import kernel_resources as kr

FIXED = ["-UPF_SOURCE_SHA256", '-DPF_SOURCE_SHA256="x"']
LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_end|Lpost_getpc)[0-9_]+")


def canonical(body: str) -> str:
    lines = []
    for line in body.split("\n"):
        if '"' not in line:  # (a ';' inside a string literal is no comment)
            line = line.split(";", 1)[0]
        line = line.rstrip()
        if line:
            lines.append(line)
    seen = {}
    return LABEL.sub(lambda m: seen.setdefault(m.group(0), f".{m.group(1)}#{len(seen)}"), "\n".join(lines))


def entries(text: str) -> dict:
    """{symbol: canonical body without its descriptor, "desc " + kernel: canonical descriptor block}"""
    out = {}
    for m in re.finditer(r"^[^\n]*-- Begin function (\S+)\n(.*?)-- End function", text, re.S | re.M):
        body = m.group(0)
        for d in re.finditer(r"[ \t]*\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel\n", body, re.S):
            out["desc " + d.group(1)] = canonical(d.group(0))
        out[m.group(1)] = canonical(re.sub(r"[ \t]*\.amdhsa_kernel \S+\n.*?\.end_amdhsa_kernel\n", "", body, flags=re.S))
    return out


def unit_entries(recipe, name: str, extra) -> dict:
    with tempfile.TemporaryDirectory() as work:
        return entries(kr.gfx950_listing(kr.unit_of(recipe, name, work), work, FIXED + list(extra)))


def main() -> int:
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    known = {os.path.basename(u[-1])[:-2] for u in kr.ge.build_units("")}
    rev = args.pop() if args and args[-1] not in known else "HEAD"
    if not args:
        raise SystemExit(__doc__)
    all_same = True
    with tempfile.TemporaryDirectory() as tree, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        kr.checkout(rev, tree)
        old_recipe = kr.load_recipe(tree)
        jobs = [(name, pool.submit(unit_entries, kr.ge, name, extra), pool.submit(unit_entries, old_recipe, name, extra)) for name in args]
        for name, new_f, old_f in jobs:
            new, old = new_f.result(), old_f.result()
            differing = sorted(k for k in set(new) & set(old) if new[k] != old[k])
            same_keys = set(new) == set(old)
            kernels = sum(1 for k in new if k.startswith("desc "))
            flags = " ".join(kr.unit_of(kr.ge, name, "")[1] + extra)
            print(f"{name} ({os.path.basename(kr.unit_of(kr.ge, name, '')[0])} {flags}) vs {rev}: entries {len(new)} "
                  f"({kernels} kernels + descriptors, {len(new) - 2 * kernels} device functions) same keys {same_keys} differing {len(differing)}")
            odd = differing + sorted(set(new) ^ set(old))
            names = kr.demangle([k.replace("desc ", "") for k in odd]) if odd else {}
            for k in odd:
                what = "differs" if k in differing else ("only now" if k in new else f"only at {rev}")
                print(f"    {what}: {'descriptor of ' if k.startswith('desc ') else ''}{names[k.replace('desc ', '')][:200]}")
            all_same = all_same and same_keys and not differing
    print("ALL IDENTICAL" if all_same else "DIFFERENT")
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
