#!/usr/bin/env python
"""Time of one ``NestedProposal.sample_and_weight`` call at 2^20 x 1 and 400 x 1000 particles x filters, M in {4, 16, 64}, both types,
on the stochastic-volatility and Lorenz-63 kinds (Philox draws), beside Bootstrap's ``pf_sample_and_weight`` at the same shape.

    python tools/nested_bench.py [sv] [lorenz]
        CALL time: device events around K back-to-back calls (K sized for a window of >= 20 ms), median of 7 windows after 3
        warm-up calls - the larger of the host's time to issue a call and the device's to run it (a short kernel reads as the
        host's ~11 us per call) - and the same for the torch route of the scalar model.
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/nested_bench.py --trace [sv] [lorenz]
    python tools/nested_bench.py --read DIR/.../t_kernel_trace.csv [sv] [lorenz]
        KERNEL time: the dispatches' own durations from a kernel trace, in a run of its own.

Recorded in profiles/nested_proposal.txt.  The torch route of a vector state is not timed: one such call, 2^26 candidates of Lorenz-63,
ended in a device memory fault inside torch's operations (cause not established; profiles/nested_proposal.txt).
"""
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfilter_amd import _lib as L  # noqa: E402
from pyfilter_amd import ops  # noqa: E402
from pyfilter_amd import timeseries as ts  # noqa: E402
from pyfilter_amd.filters.particle import SISR, proposals  # noqa: E402
from pyfilter_amd.filters.particle.state import ParticleFilterPrediction  # noqa: E402
from pyfilter_amd.timeseries import TimeseriesState, models  # noqa: E402


def build(kind, b, dtype):
    t = lambda v: torch.tensor(v, dtype=dtype, device="cuda")  # noqa: E731
    if kind == "sv":
        i = torch.arange(b, dtype=dtype, device="cuda") / max(b, 1)
        hidden = models.Verhulst(0.05 + 0.01 * i, 1.0 + 0.1 * i, 0.10 + 0.02 * i, dt=0.2, initial=(t(1.0), t(0.1)))
        return models.StochasticVolatilityModel(hidden, 0.05 * i).to("cuda"), t(0.3)
    hidden = models.Lorenz63(t(10.0), t(28.0), t(8.0 / 3.0), t(1.0), dt=0.01)
    a = t([[0.8, 0.0, 0.0], [0.0, 0.0, 0.8]])
    return ts.LinearStateSpaceModel(hidden, (a, t([0.0]), t([math.sqrt(0.1)])), torch.Size([2])).to("cuda"), t([-4.7, 19.6])


def timed(fn, budget_ms=20.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()  # noqa: E702
    k = max(3, min(2000, int(budget_ms / max(a.elapsed_time(b), 1e-3)) + 1))
    windows = []
    for _ in range(7):
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / k * 1e3)
    return statistics.median(windows), min(windows), max(windows)


TRACE_CALLS = 20  # calls per configuration in --trace mode (the last 15 are read)


def configs(kinds):
    for kind in kinds:
        for dtype in (torch.float32, torch.float64):
            for n, b in ((1 << 20, 1), (400, 1000)):
                yield kind, dtype, n, b


def setup(kind, dtype, n, b):
    ssm, y = build(kind, b, dtype)
    filt = SISR(ssm, n, proposal=proposals.NestedProposal(4), seed=1)
    filt.set_batch_shape(torch.Size([b]))
    state = filt.initialize()
    ctx = filt._ensure_context()
    soa = ops.to_soa(state.timeseries_state.value, True, ctx.has_event).contiguous()
    return ssm, y, state, ctx, soa


def main(kinds):
    print(f"{'kind':7s}{'type':5s}{'N x B':>16s}{'M':>4s}  {'nested call us (min..max)':>30s}{'bootstrap call us':>19s}{'torch call us':>15s}")
    for kind, dtype, n, b in configs(kinds):
        ssm, y, state, ctx, soa = setup(kind, dtype, n, b)
        x = state.timeseries_state
        boot = timed(lambda: ops.sample_and_weight_soa(ctx.kind, ctx.params, L.PROP_BOOTSTRAP, soa, y, None, 1, 0))
        for m in (4, 16, 64):
            ker = timed(lambda: ops.nested_sample_and_weight_soa(ctx.kind, ctx.params, m, soa, y, None, None, 1, 0))
            tor = None
            if kind == "sv":  # (the scalar model only: module docstring)
                prop = proposals.NestedProposal(m).set_model(ssm)  # (no kernel context on this proposal: the torch route)
                pred = ParticleFilterPrediction.equally_weighted(TimeseriesState(0, x.value, x.event_shape), state.weights)
                tor = timed(lambda: prop.sample_and_weight(y, pred))
            print(f"{kind:7s}{'f32' if dtype == torch.float32 else 'f64':5s}{f'{n} x {b}':>16s}{m:4d}  "
                  f"{ker[0]:14.1f} ({ker[1]:.1f}..{ker[2]:.1f}){boot[0]:19.1f}" + (f"{tor[0]:15.1f}" if tor else f"{'-':>15s}"), flush=True)
            torch.cuda.empty_cache()


def trace_calls(kinds):
    """--trace: TRACE_CALLS synchronised calls of Bootstrap's kernel, then of the nested kernel per M, per configuration - to be run
    under ``rocprofv3 --kernel-trace``; ``read_trace`` reads the kernels' own durations back in this order."""
    for kind, dtype, n, b in configs(kinds):
        _, y, _, ctx, soa = setup(kind, dtype, n, b)
        for _ in range(TRACE_CALLS):
            ops.sample_and_weight_soa(ctx.kind, ctx.params, L.PROP_BOOTSTRAP, soa, y, None, 1, 0)
            torch.cuda.synchronize()
        for m in (4, 16, 64):
            for _ in range(TRACE_CALLS):
                ops.nested_sample_and_weight_soa(ctx.kind, ctx.params, m, soa, y, None, None, 1, 0)
                torch.cuda.synchronize()


def read_trace(path, kinds):
    """Kernel durations (End - Start timestamp, ns) of a ``*_kernel_trace.csv`` written under ``trace_calls``: median of the last 15 of
    each configuration's TRACE_CALLS dispatches."""
    import csv

    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"boot": [], "nested": []}
    for r in rows:
        name = r["Kernel_Name"]
        key = "nested" if "k_nested_sample_and_weight" in name else ("boot" if "k_sample_and_weight" in name else None)
        if key:
            dur[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    cfgs = list(configs(kinds))
    assert len(dur["boot"]) == TRACE_CALLS * len(cfgs) and len(dur["nested"]) == 3 * TRACE_CALLS * len(cfgs), (len(dur["boot"]), len(dur["nested"]))
    print(f"{'kind':7s}{'type':5s}{'N x B':>16s}{'M':>4s}{'nested kernel us':>18s}{'ns/candidate':>14s}{'bootstrap kernel us':>21s}{'ns/particle':>13s}")
    for c, (kind, dtype, n, b) in enumerate(cfgs):
        bo = statistics.median(dur["boot"][c * TRACE_CALLS + 5:(c + 1) * TRACE_CALLS])
        for k, m in enumerate((4, 16, 64)):
            lo = (3 * c + k) * TRACE_CALLS
            ne = statistics.median(dur["nested"][lo + 5:lo + TRACE_CALLS])
            print(f"{kind:7s}{'f32' if dtype == torch.float32 else 'f64':5s}{f'{n} x {b}':>16s}{m:4d}{ne:18.1f}{ne * 1e3 / (n * b * m):14.4f}"
                  f"{bo:21.1f}{bo * 1e3 / (n * b):13.4f}")


if __name__ == "__main__":
    names = [k for k in sys.argv[1:] if k in ("sv", "lorenz")] or ["sv", "lorenz"]
    if "--trace" in sys.argv:
        trace_calls(names)
    elif "--read" in sys.argv:
        read_trace(sys.argv[sys.argv.index("--read") + 1], names)
    else:
        main(names)
