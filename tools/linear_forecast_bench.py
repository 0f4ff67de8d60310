#!/usr/bin/env python
"""Times forecasting from a ``LinearModel`` filter state (``PF_HID_LINEAR_MAT``, ``csrc/pf_forecast_linear.hpp``) on either route, on
the same filter state, GPU and process, float32, ``H = 32``:

* ``filt.forecast(state, 32, route="kernel")`` (``pf_forecast_linear``) against ``route="torch"`` (a loop of torch operations over
  the horizon), the two alternating call by call, each timed call ending in a device synchronise (host clock), the median of the
  timed calls after a warm-up;
* the kernel pair alone (``ops.forecast_linear_soa`` on its own layout) from device events;

at 64 filters x 1 024 particles and 8 x 65 536, for the constant-velocity model (``D = 4, O = 2``) and a dense ``D = O = 8`` model,
with and without ``covariance``, with and without ``paths``.

    python tools/linear_forecast_bench.py [--reps 20] [--out FILE]           # recorded in profiles/forecast_linear.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import linear_smooth_bench as LS  # noqa: E402  (the models and their parameters)

F32 = torch.float32
H = 32
SHAPES = ((64, 1024), (8, 65536))


def filter_state(builder, theta, b, n, y):
    from pyfilter_amd.filters.particle import SISR

    filt = SISR(builder, n, seed=1)
    filt.set_batch_shape(torch.Size([b]))
    filt.initialize_model(theta)
    return filt, filt.batch_filter(y, bar=False).latest_state


def alternating(fns, reps, warm=3):
    """ms per call of each function, called in turn; every timed region ends in a synchronise"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
            del r
    return [(statistics.median(v), min(v)) for v in out]


def lines_for(name, builder, theta_of, d, o, reps):
    from pyfilter_amd import ops
    from pyfilter_amd.filters.particle.forecast import normalized_weights

    lines = []
    for b, n in SHAPES:
        y = LS.cv_data(20) if o == 2 else torch.randn((20, o), generator=torch.Generator().manual_seed(5)).cuda()
        filt, state = filter_state(builder, theta_of(b), b, n, y)
        ctx = filt._ensure_context()
        soa = ops.to_soa(state.timeseries_state.value, True, True)
        W = ops.to_cols(normalized_weights(state.weights))
        lines.append(f"forecast: {name}, D = {d}, O = {o}, {b} filters x {n} particles, H = {H}, float32; ms per call, median (min) of {reps}")
        lines.append(f'  {"":28s} {"route=kernel":>20s} {"route=torch":>20s} {"torch / kernel":>15s} {"kernel pair alone":>20s}')
        for cov in (False, True):
            for paths in (False, True):
                kern, tor = alternating([lambda: filt.forecast(state, H, paths=paths, seed=7, route="kernel", covariance=cov),
                                         lambda: filt.forecast(state, H, paths=paths, seed=7, route="torch", covariance=cov)], reps)
                alone = LS.events(lambda: ops.forecast_linear_soa(ctx.kind, ctx.params, H, soa, W, None, None, 7, paths, cov), reps)
                label = f"covariance={cov!s:5s} paths={paths!s:5s}"
                lines.append(f"  {label:28s} {kern[0]:11.3f} ({kern[1]:6.3f}) {tor[0]:11.3f} ({tor[1]:6.3f}) {tor[0] / kern[0]:14.1f}x "
                             f"{alone[0]:11.3f} ({alone[1]:6.3f})")
        del filt, state, soa, W
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.reps >= 20, "the medians are of at least 20 timed calls"
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def emit(new):
        nonlocal lines
        lines += new
        print("\n".join(new), flush=True)
        if a.out:  # (rewritten after every section: what was measured survives a later section that fails)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit([])
    emit(lines_for("constant velocity", LS.cv_builder(), LS.cv_theta, 4, 2, a.reps))
    emit(lines_for("dense model", LS.dense_builder(8, 8), lambda b: LS.dense_theta(b, 8, 8), 8, 8, a.reps))


if __name__ == "__main__":
    main()
