#!/usr/bin/env python
"""Where a NESS run spends its time (development tool), at two shapes: 1 000 theta x 400 state particles (the reference's published
operating point, examples/lorenz.ipynb in BASELINE.md) and 128 theta x 8 192.  The model is the Ornstein-Uhlenbeck state-space
model with the priors of tools/smc2_timeline.py - NOT the notebook's Lorenz-63, which was not set up with per-theta parameters
here: the figures are comparable with this repository's SMC^2 timelines, and only context next to the notebook's.

    python tools/ness_timeline.py                      # the three measurements below at both shapes
    python tools/ness_timeline.py --count ROUTE K      # K updates + 2 K moves, then 2 K moves alone (for rocprofv3, see below)

1. Time per observation WITHOUT an update - ``NESS.step`` (threshold 0: the update never fires) next to ``SMC2.step`` (threshold
   0) in the same process, interleaved repeats: both make the same ``pf_filter_observe`` call.  (The A/B against the parent
   commit's ``SMC2.step`` is ``tools/smc2_step_profile.py`` run from a checkout of the parent in the same session.)
2. Time of one update on both theta routes: every step ends with the poll of the host slot, so ``perf_counter`` per step is
   meaningful; an update's cost is the median step WITH an update minus the median step without one.
3. Whole-run observations per second of the default ``NESS`` (threshold 0.9, ``NonShrinkingKernel``).

Launch counts come from a ``rocprofv3 --kernel-trace --stats`` run of ``--count`` per route: (launches of the run with K
updates - launches of the run without) / K.  Every repeat is printed; "spread" is the range of the repeats' medians."""
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _env  # noqa: E402

_env.setup()


def setup(t_len, dtype=torch.float32):
    from torch.distributions import Exponential, LogNormal, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    device = torch.device("cuda")
    g = torch.Generator().manual_seed(123)
    x, ys = 0.0, []
    for _ in range(t_len):
        x = x * math.exp(-0.025) + 0.05 * math.sqrt((1 - math.exp(-0.05)) / 0.05) * torch.randn((), generator=g).item()
        ys.append(x + 0.05 * torch.randn((), generator=g).item())
    y = torch.tensor(ys, dtype=dtype, device=device)
    priors = {"kappa": Exponential(10.0), "gamma": Normal(0.0, 1.0), "sigma": LogNormal(-2.0, 1.0)}
    obs_a, obs_s = torch.tensor(1.0, dtype=dtype, device=device), torch.tensor(0.05, dtype=dtype, device=device)

    def build(theta):
        return ts.LinearStateSpaceModel(models.OrnsteinUhlenbeck(theta["kappa"], theta["gamma"], theta["sigma"], dt=1.0), (obs_a, obs_s))

    return y, priors, build


def make(cls, build, priors, n_theta, n_state, seed, **kwargs):
    from pyfilter_amd.filters.particle import APF, proposals

    filt = APF(build, n_state, proposal=proposals.LinearGaussianObservations(), seed=2024 + seed)
    return cls(filt, n_theta, priors, device="cuda", dtype=torch.float32, seed=seed, **kwargs)


def step_times(alg, y, updates_of):
    """Per-step wall times of one run, split into steps with and without an update."""
    state = alg.initialize()
    torch.cuda.synchronize()
    plain, updated = [], []
    t_all = time.perf_counter()
    for yt in y:
        n0 = updates_of(alg)
        t0 = time.perf_counter()
        state = alg.step(yt, state)
        dt = time.perf_counter() - t0
        (updated if updates_of(alg) != n0 else plain).append(dt)
    torch.cuda.synchronize()
    return plain, updated, time.perf_counter() - t_all


def med_us(v):
    return 1e6 * statistics.median(v) if v else float("nan")


def timeline(n_theta, n_state, t_len=400, repeats=5, warm=40):
    from pyfilter_amd.hints import HINTS
    from pyfilter_amd.inference import NESS, SMC2

    y, priors, build = setup(t_len)
    print(f"== {n_theta} theta x {n_state} state particles, T = {t_len}, float32, OU model ==", flush=True)
    # 1. no update: NESS.step next to SMC2.step (threshold 0: neither ever moves the parameters), interleaved
    meds = {"NESS": [], "SMC2": []}
    for rep in range(repeats + 1):
        for name, cls in (("NESS", NESS), ("SMC2", SMC2)):
            alg = make(cls, build, priors, n_theta, n_state, rep, threshold=0.0)
            plain, updated, _ = step_times(alg, y, (lambda a: a._kernel.updates) if name == "NESS" else (lambda a: len(a._kernel.acceptance_history)))
            assert not updated
            if rep:  # (repeat 0 warms up: library load, plans, allocator)
                meds[name].append(med_us(plain[warm:]))
    for name, v in meds.items():
        print(f"1. {name}.step without an update: median per observation {statistics.median(v):7.1f} us; repeats " + ", ".join(f"{m:.1f}" for m in v) +
              f"; spread {min(v):.1f} .. {max(v):.1f} us", flush=True)
    # 2. one update on both routes
    for route in ("kernels", "torch"):
        HINTS.theta_kernels = route == "kernels"
        costs = []
        for rep in range(repeats + 1):
            alg = make(NESS, build, priors, n_theta, n_state, rep)
            plain, updated, total = step_times(alg, y, lambda a: a._kernel.updates)
            assert alg._kernel.last_route == route, alg._kernel.last_route
            if rep:
                costs.append((med_us(updated[5:]) - med_us(plain), med_us(updated[5:]), med_us(plain), len(updated), t_len / total))
        HINTS.theta_kernels = True
        c = [k[0] for k in costs]
        print(f"2. one update, {route:7s} route: median cost {statistics.median(c):7.1f} us (step with an update {statistics.median(k[1] for k in costs):.1f} us - "
              f"step without {statistics.median(k[2] for k in costs):.1f} us); repeats " + ", ".join(f"{v:.1f}" for v in c) +
              f"; spread {min(c):.1f} .. {max(c):.1f} us; updates per run {[k[3] for k in costs]}", flush=True)
        r = [k[4] for k in costs]
        print(f"3. whole run, {route:7s} route: median {statistics.median(r):8.0f} observations/s; repeats " + ", ".join(f"{v:.0f}" for v in r), flush=True)


def count(route, k, n_theta=1000, n_state=400):
    """K updates among 2 K moves (``FixedWidthNESS(block_len=2)``), or none (``--count ROUTE-none``): the launches of the two differ
    by K updates."""
    from pyfilter_amd.hints import HINTS
    from pyfilter_amd.inference import FixedWidthNESS

    y, priors, build = setup(2 * k)
    none = route.endswith("-none")
    HINTS.theta_kernels = route.startswith("kernels")
    alg = make(FixedWidthNESS, build, priors, n_theta, n_state, 0, block_len=(10 ** 9 if none else 2))
    state = alg.initialize()
    for yt in y:
        state = alg.step(yt, state)
    torch.cuda.synchronize()
    print(f"{route}: {alg._kernel.updates} updates, {2 * k} moves, route {alg._kernel.last_route}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--count":
        count(sys.argv[2], int(sys.argv[3]))
    else:
        for shape in ((1000, 400), (128, 8192)):
            timeline(*shape)
