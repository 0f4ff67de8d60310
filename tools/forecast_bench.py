#!/usr/bin/env python
"""Times ``ParticleFilter.forecast`` on the kernel route (``pf_forecast``: moments only, and with paths) against the torch loop it
stands beside (``ParticleFilterCorrection.predict_path`` -> ``StateSpaceModel.sample_states``, which always materialises paths and
gives no moments), for the README's sine diffusion in float32 at 2^20 x 1 and 400 x 1000 (particles x filters), H in {8, 32}.
Device events around every call, a warm-up, the routes alternated within one process; median and minimum of the repeats.
Also: the bytes a moments-only call has to move - (D + 1) * 4 per particle, the cloud and its weights read once - against its time.

    python tools/forecast_bench.py [--reps 20] [--out FILE]           # recorded in profiles/forecast.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(n, b):
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import APF
    from pyfilter_amd.timeseries import models

    t = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")  # noqa: E731
    ssm = ts.LinearStateSpaceModel(models.SineDiffusion(t(0.0), t(1.0), dt=0.1), (t(1.0), t(0.1))).to("cuda")  # (the increments too)
    filt = APF(ssm, n, seed=1)
    filt.set_batch_shape(torch.Size([b]))
    state = filt.initialize()
    y = torch.zeros(3, device="cuda")
    return filt, filt.batch_filter(y, bar=False, init_state=state).latest_state


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    del out
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; sine diffusion (D = 1, O = 1), float32; ms per call, median (min) of {a.reps}"]
    for n, b in ((1 << 20, 1), (400, 1000)):
        filt, state = build(n, b)
        for h in (8, 32):
            routes = {
                "kernel, moments only": lambda: filt.forecast(state, h),
                "kernel, with paths": lambda: filt.forecast(state, h, paths=True),
                "torch loop (predict_path)": lambda: state.predict_path(filt.ssm, h).get_paths(),
            }
            for fn in routes.values():  # warm-up
                for _ in range(3):
                    timed(fn)
            times = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, fn in routes.items():  # alternated
                    times[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, v in times.items():
                lines.append(f"N = {n:8d} B = {b:5d} H = {h:3d}  {k:27s} {med[k]:9.3f} ({min(v):9.3f})")
            moved = n * b * 2 * 4  # (D + 1) * 4 bytes per particle, D = 1
            lines.append(f"    moments only: {moved / 1e6:.2f} MB read once -> {moved / (med['kernel, moments only'] * 1e-3) / 1e9:.1f} GB/s of its call time; "
                         f"torch loop / kernel with paths = {med['torch loop (predict_path)'] / med['kernel, with paths']:.2f}, "
                         f"/ moments only = {med['torch loop (predict_path)'] / med['kernel, moments only']:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
