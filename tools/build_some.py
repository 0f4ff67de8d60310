#!/usr/bin/env python
"""Development: recompile SOME translation units of libpfamd.so (by unit name: ``main col_f32 col_f64 clu_f32 clu_f64 f32d1_v4_m0
... f64_m1``, with or without the objects' ``pf_`` prefix) with the flags ``__graft_entry__.build_units`` gives them, and link them
with the production objects of the rest (``build/obj``, from ``__graft_entry__.build()``).
    python tools/build_some.py UNIT...                                     in place: build/obj -> libpfamd.so - minutes less than
        ``build(force=True)`` when an edit touches one header.  The digest compiled in is the tree's, so
        ``binary_matches_sources()`` holds only if every unit the edit reaches was named.
    python tools/build_some.py --variant NAME [--flags="FLAGS"] UNIT...    an A/B library next to the shipped one: the named units
        with the extra flags into build/NAME/, linked into pyfilter_amd/libpfamd_NAME.so - load it with
        ``PF_AMD_LIB=.../libpfamd_NAME.so`` (tools/kbench.py, tools/ab.sh, the test suite).  ``--flags=-fslp-vectorize`` undoes the float
        units' ``NO_SLP`` (write the ``=``: the flags begin with a dash)."""
import argparse
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def rebuild(names, extra=(), variant=None):
    """Compiles the named units (``extra``: further hipcc flags) and links them with the production objects of the others: in place,
    or - ``variant`` given - into ``build/<variant>/`` and ``pyfilter_amd/libpfamd_<variant>.so``.  Returns the library's path."""
    want = {n if n.startswith("pf_") else "pf_" + n for n in names}
    objdir = os.path.join(ROOT, "build", variant or "obj")
    os.makedirs(objdir, exist_ok=True)
    mine = [u for u in ge.build_units(objdir) if os.path.basename(u[2])[:-2] in want]
    assert len(mine) == len(want), "unknown unit name"
    procs = [subprocess.Popen(**ge.unit_command(u, extra)) for u in mine]
    if any([p.wait() for p in procs]):
        raise SystemExit("compile failed")
    rebuilt = {os.path.basename(obj): obj for _, _, obj in mine}
    objs = [rebuilt.get(os.path.basename(obj), obj) for _, _, obj in ge.build_units(os.path.join(ROOT, "build", "obj"))]
    lib = ge.LIB if variant is None else os.path.join(ROOT, "pyfilter_amd", f"libpfamd_{variant}.so")
    subprocess.check_call(**ge.link_command(objs, lib))
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", help="link pyfilter_amd/libpfamd_<variant>.so instead of relinking libpfamd.so in place")
    ap.add_argument("--flags", default="", help="extra hipcc flags for the named units: --flags=\"-DX -DY\"")
    ap.add_argument("units", nargs="+")
    a = ap.parse_args()
    lib = rebuild(a.units, shlex.split(a.flags), a.variant)
    if a.variant is None:
        print("relinked; matches sources:", ge.binary_matches_sources())
    print(lib)


if __name__ == "__main__":
    main()
