#!/usr/bin/env python
"""The figures behind the tolerances of ``tests/test_score_parity_gpu.py``, per model kind (S = 17, N = 65, B = 3, shared
observations): the reference's own float32 error - torch float32 autograd of the expression on the CPU against the float64
oracle at the same inputs - and the kernel's error in both dtypes, each as the largest ``|difference| / A_k`` over the row slots
(``A_k = 1/N sum |term|``; slots a kind never reads have ``A_k = 0`` and are exact).  The float64 test bound is 1e-10 in these
units, the float32 bound four times the reference's figure plus 64 eps32 = 7.6e-6.

    python tools/path_score_parity.py [--out FILE]           # recorded in profiles/path_score_parity.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    from tests import test_score_parity_gpu as t

    def rel(err, scale):
        return float((err / scale.clamp_min(1e-300)).max())

    lines = [f"device: {torch.cuda.get_device_name(0)}; S = 17, N = 65, B = 3; largest |difference| / A_k over value and row slots",
             f"{'kind':24s} {'condition':>9s} {'reference f32':>14s} {'kernel f32':>12s} {'kernel f64':>12s}"]
    for name in sorted(t.BY_NAME):
        inp, y, ref, ref32 = t.case(name, 17, 65, 3, 1)
        cols = [max(rel((ref32["value"].double() - ref["value"]).abs(), ref["A_value"]),
                    rel((ref32["grad"].double() - ref["grad"]).abs(), ref["A_grad"]))]
        for dtype in (torch.float32, torch.float64):
            value, grad = t.run_kernel(t.BY_NAME[name], inp, y, dtype)
            cols.append(max(rel((value - ref["value"]).abs(), ref["A_value"]), rel((grad - ref["grad"]).abs(), ref["A_grad"])))
        lines.append(f"{name:24s} {ref['condition']:9.1f} {cols[0]:14.3g} {cols[1]:12.3g} {cols[2]:12.3g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
