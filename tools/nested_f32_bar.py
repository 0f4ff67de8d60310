"""What the package's TORCH route of the nested proposal differs, in float32, from the float64 oracle (``tests/nested_oracle.py``) on
the inputs of ``tests/test_nested_gpu.py``'s float32 checks - the figure that test's bar is four times of - and, with a GPU, the same
for the kernel.  ``max |dw| / (1 + |w|)`` and the share of differing picks, worst call per model.

    python tools/nested_f32_bar.py [cpu|cuda]           # recorded in profiles/nested_proposal.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import nested_cases as nc  # noqa: E402


def main(device):
    rows = {}
    for call in nc.f32_inputs():
        routes = {"torch": nc.torch_route(call, device)}
        if device == "cuda":
            routes["kernel"] = nc.run_kernel(call)
        for route, (_, w, pick) in routes.items():
            k = (call.case["model"], route)
            e, p = rows.get(k, (0.0, 0.0))
            rows[k] = (max(e, nc.weight_error(w, call.ref_w)), max(p, nc.pick_mismatch(pick, call.ref_pick)))
    for (model, route), (e, p) in sorted(rows.items()):
        print(f"{device:5s} {model:11s} {route:6s} weight error {e:.2e}   picks differing {p:.1e}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "cpu")
