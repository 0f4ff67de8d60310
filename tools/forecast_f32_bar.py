"""What ``oracle/models.py`` evaluated in float32 differs from its float64 self on the inputs of ``tests/test_forecast_gpu.py``'s
float32 check (``tests/forecast_oracle.grid``): the figure that test's bar is four times of.  Scaled error ``max |d| / (1 + |ref|)``,
worst call per model, for the four moment arrays and for the two paths; with ``cuda`` the same for the kernel.

Then the same for the clouds at a level of ``tests/test_moments_parity_gpu.py`` (``tests/forecast_oracle.level_grid``), per model
and level: the two means and the two paths scaled as above, the two variances RELATIVE TO THE VARIANCE.

    python tools/forecast_f32_bar.py [cpu|cuda]           # recorded in profiles/forecast.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import forecast_oracle as fo  # noqa: E402


def main(device):
    rows = {}
    for inp in fo.grid(fo.GPU_MODELS, torch.float32):
        ref = inp.reference(torch.float32)
        routes = {"oracle32": inp.oracle_f32()}
        if device == "cuda":
            routes["kernel"] = fo.run_kernel(inp, torch.float32)
        for route, got in routes.items():
            k = (inp.model, route)
            rows[k] = tuple(max(a, b) for a, b in zip(rows.get(k, (0.0, 0.0)), fo.errors(got, ref)))
    for (model, route), (mom, path) in sorted(rows.items()):
        print(f"{model:11s} {route:8s} moments {mom:.2e}   paths {path:.2e}")
    rows = {}
    for inp in fo.level_grid():
        ref = inp.reference(torch.float32)
        routes = {"oracle32": inp.oracle_f32()}
        if device == "cuda":
            routes["kernel"] = fo.run_kernel(inp, torch.float32)
        for route, got in routes.items():
            k = (inp.model, inp.level, route)
            rows[k] = tuple(max(a, b) for a, b in zip(rows.get(k, (0.0, 0.0, 0.0)), fo.level_errors(got, ref)))
    for (model, level, route), (mean, var, path) in sorted(rows.items()):
        print(f"{model:11s} level {level:.0e} {route:8s} means {mean:.2e}   variances (relative) {var:.2e}   paths {path:.2e}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "cpu")
