#!/usr/bin/env python
"""The figures behind ``tests/test_linmat_parity_gpu.py``: the ``PF_HID_LINEAR_MAT`` kernels (``csrc/pf_linear.hpp``) against the exact
oracle of ``tests/linmat_oracle.py`` over the case list of ``tests/linmat_cases.py``.

Per case and entry point: the float64 ``err / bound`` (largest over particles and components, particles ``x`` and log-weights ``w``) and
the float32 errors of the kernel and of the reference's own float32 arithmetic (``oracle/cpu_ref.py`` on the CPU).  For the
conditioning ladder the kernel's float64 error against ``cond_2(P)``; and - here only, asserted by no test - (4, 2) and (8, 3) at
``s_o / s`` = 1e-4 and 1e-5, beyond the cap of ``cond_2(P) = 1e8`` under which the bound is a test.

    python tools/linmat_parity.py [--out FILE] [--all]      # recorded in profiles/linear_parity.txt  (--all: every edge case too)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, F64 = torch.float32, torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--all", action="store_true", help="list every edge case, not only the worst per shape")
    a = ap.parse_args()
    import _env
    _env.setup()
    from tests import linmat_cases as LC

    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    worst64, worst32 = (0.0, ""), (0.0, "")

    def fmt(m, k):
        return f"{m[k]:9.3g}" if k in m else f"{'-':>9s}"

    def row(c, entry, dtypes=(F64, F32)):
        nonlocal worst64, worst32
        m64 = LC.measure(c, entry, F64)
        text = f"{repr(c):34s} {entry:14s} {fmt(m64, 'x')} {fmt(m64, 'w')}"
        big = max(m64.get("x", 0.0), m64.get("w", 0.0))
        if big > worst64[0]:
            worst64 = (big, f"{c!r} {entry}")
        if F32 in dtypes:
            m32 = LC.measure(c, entry, F32)
            for k in ("x", "w"):
                if k in m32:
                    ratio = m32[k + "_err"] / m32[k + "_ref"] if m32[k + "_ref"] > 0 else float("inf") if m32[k + "_err"] > 0 else 0.0
                    text += f"  {k}: {m32[k + '_err']:9.3g} / {m32[k + '_ref']:9.3g} = {ratio:6.3g} ({m32[k]:.3g} of bound)"
                    if ratio > worst32[0]:
                        worst32 = (ratio, f"{c!r} {entry} {k}")
        return text, m64

    head = f"{'case':34s} {'entry':14s} {'f64 x':>9s} {'f64 w':>9s}  float32: kernel error / reference error"
    lines += ["", "every D x O, N = 65, B = 3, one y row per filter, s_o / s = 2 - float64 err / bound; float32 errors", head]
    for c in LC.every_shape():
        lines += [row(c, e)[0] for e in LC.ENTRY_POINTS]
    lines += ["", "edge shapes: particle counts, filters, observation rows" + ("" if a.all else " - the worst entry point of each case"), head]
    for c in LC.edge_cases():
        rows = [row(c, e) for e in LC.ENTRY_POINTS]
        lines += [t for t, _ in rows] if a.all else [max(rows, key=lambda r: max(r[1].get("x", 0.0), r[1].get("w", 0.0)))[0]]
    lines += ["", "states far from zero", head]
    for c in LC.level_cases():
        lines += [row(c, e)[0] for e in LC.ENTRY_POINTS]
    lines += ["", "second trip of the grid stride (N = 2048 x 256 + 77)", head]
    for (d, o), dtype in LC.SECOND_TRIP:
        for e in ("lgo", "pre_lgo"):
            lines.append(row(LC.second_trip_case(d, o), e, (F64, F32) if dtype == F32 else (F64,))[0])
    lines += ["", "conditioning ladder, float64, optimal proposal: the kernel's error against cond_2(P)",
              f"{'case':34s} {'cond_2(P)':>10s} {'x error':>10s} {'w error':>10s} {'x err/bound':>12s} {'w err/bound':>12s}"]
    for c in LC.ladder_cases():
        _, m = row(c, "lgo", (F64,))
        lines.append(f"{repr(c):34s} {c.cond_P():10.3g} {m['x_err']:10.3g} {m['w_err']:10.3g} {m['x']:12.3g} {m['w']:12.3g}")
        for e in LC.ENTRY_POINTS[1:]:
            row(c, e, (F64,))
    lines += ["", "beyond the cap (asserted by no test): the kernel's float64 error, optimal proposal",
              f"{'case':34s} {'cond_2(P)':>10s} {'x error':>10s} {'w error':>10s} {'x err/bound':>12s} {'w err/bound':>12s}"]
    w64 = worst64
    for d, o in ((4, 2), (8, 3)):
        for ratio in (1e-4, 1e-5):
            c = LC.case(d, o, 65, 3, 3, ratio=ratio)
            _, m = row(c, "lgo", (F64,))
            lines.append(f"{repr(c):34s} {c.cond_P():10.3g} {m['x_err']:10.3g} {m['w_err']:10.3g} {m['x']:12.3g} {m['w']:12.3g}")
    worst64 = w64  # (the uncapped cases do not count)
    lines += ["", f"largest float64 err / bound over the tested cases: {worst64[0]:.3g} ({worst64[1]})",
              f"largest float32 kernel error / reference error: {worst32[0]:.3g} ({worst32[1]})"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
