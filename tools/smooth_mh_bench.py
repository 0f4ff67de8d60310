#!/usr/bin/env python
"""Times ``smooth(states, "ffbs-mh")`` (``pf_smooth_mh``, ``csrc/pf_smooth_mh.hpp``) at K = ``mcmc_steps`` in {2, 8, 32} against
``"ffbs"`` and ``"fl"`` of the same build, on the same GPU, recorded states and process, float32:

* the sine diffusion at 64 filters x 1 024 particles x T = 100 and at 8 x 65 536 x T = 50;
* the 4-D constant-velocity tracker (``LinearModel``, ``route="kernel"``) at 64 x 1 024 x T = 100;
* one PMMH move at 64 chains x 1 024 particles x T = 100 with ``RandomWalk`` and with ``GradientBasedProposal`` under each method:
  the Ornstein-Uhlenbeck model of ``tools/path_score_bench.py`` and the tracker of ``tools/linear_smooth_bench.py``.

Device events around each call (or a host clock around a PMMH move that ends in a device synchronise), warm-ups, the median (and
minimum) of the repeats; one process.  A call that takes more than a second is repeated three times, one of more than ten seconds once, not ``--reps`` times.

    python tools/smooth_mh_bench.py [--reps 10] [--moves 5] [--out FILE]           # recorded in profiles/smooth_mh.txt
"""
import argparse
import importlib.util
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = torch.float32
ROUNDS = (2, 8, 32)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def t32(v):
    return torch.tensor(v, dtype=F32, device="cuda")


def events(fn, reps, warm=2):
    """Median and minimum ms of ``fn()`` by device events, and the repeats taken."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    if first > 10.0:
        reps = 1
    elif first > 1.0:
        reps = min(reps, 3)
    else:
        for _ in range(warm - 1):
            fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        r = fn()
        stop.record()
        stop.synchronize()
        del r
        out.append(start.elapsed_time(stop))
    return statistics.median(out), min(out), reps


def sine_recorded(b, n, t_obs):
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.timeseries import models

    ssm = ts.LinearStateSpaceModel(models.SineDiffusion(t32(0.0), t32(1.0), dt=0.1), (t32(1.0), t32(0.1))).to("cuda")
    filt = APF(ssm, n, proposal=proposals.LinearGaussianObservations(), record_states=True, seed=1)
    filt.set_batch_shape(torch.Size([b]))
    y = (0.5 * torch.randn(t_obs, generator=torch.Generator().manual_seed(4)).cumsum(0)).cuda()
    return filt, list(filt.batch_filter(y, bar=False).states)


def smooth_lines(name, filt, states, shape, reps, route="auto"):
    b, n, t_obs = shape
    lines = [f"smooth(states, method): {name}, {b} filters x {n} particles x T = {t_obs}, float32, route={route}; ms per call, median (min) of n"]
    got = {}
    calls = [("fl", lambda: filt.smooth(states, "fl")), ("ffbs", lambda: filt.smooth(states, "ffbs", route=route))]
    calls += [(f"ffbs-mh K={k}", lambda k=k: filt.smooth(states, "ffbs-mh", mcmc_steps=k, route=route)) for k in ROUNDS]
    for label, fn in calls:
        med, lo, taken = events(fn, reps)
        got[label] = med
        lines.append(f"  {label:16s} {med:12.3f} ({lo:.3f})   n = {taken}")
    lines.append("  ffbs / ffbs-mh: " + ", ".join(f"K={k}: {got['ffbs'] / got[f'ffbs-mh K={k}']:.1f} x" for k in ROUNDS)
                 + "; ffbs-mh / fl: " + ", ".join(f"K={k}: {got[f'ffbs-mh K={k}'] / got['fl']:.1f} x" for k in ROUNDS))
    return lines


def pmmh_lines(name, build, priors, y, configs, moves):
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.inference import PMMH, run_pmmh

    lines = [f"PMMH, {name}, 64 chains x 1 024 particles x T = {y.shape[0]}, float32: ms per move, median (min) of {moves} moves, each "
             "ending in a device synchronise (host clock)"]
    got = {}
    for label, proposal, record in configs:
        alg = PMMH(SISR(build, 1024, record_states=record, seed=1), moves, priors, num_chains=64, proposal=proposal, seed=2)
        state = alg.initialize(y)
        kernel = proposal.build(alg.theta, state, alg.filter, y)
        ptheta, pfilter = alg.theta.like(), alg.filter.copy()
        pfilter.initialize_model(ptheta)

        def move():
            return run_pmmh(alg.theta, state, proposal, kernel, pfilter, ptheta, y, alg.filter.batch_shape, mutate_kernel=True, generator=alg._gen)

        for _ in range(2):
            move()
        torch.cuda.synchronize()
        out = []
        for _ in range(moves):
            t0 = time.perf_counter()
            move()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        got[label] = statistics.median(out)
        lines.append(f"  {label:52s} {got[label]:10.2f} ({min(out):.2f})")
        del alg, state, kernel, pfilter
        torch.cuda.empty_cache()
    return lines


def ou_pmmh(moves):
    from torch.distributions import LogNormal, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.inference import GradientBasedProposal, RandomWalk
    from pyfilter_amd.timeseries import models

    gen = torch.Generator().manual_seed(5)
    x, ys = torch.tensor(1.0), []
    e, sd = math.exp(-0.5), 0.4 * math.sqrt((1.0 - math.exp(-1.0)) / 1.0)
    for _ in range(100):
        x = 1.0 + (x - 1.0) * e + sd * torch.randn((), generator=gen)
        ys.append(x + 0.3 * torch.randn((), generator=gen))
    y = torch.stack(ys).cuda()
    priors = {"kappa": LogNormal(math.log(0.5), 0.2), "gamma": Normal(1.0, 0.3), "sigma": LogNormal(math.log(0.4), 0.2)}

    def build(theta):
        return ts.LinearStateSpaceModel(models.OrnsteinUhlenbeck(theta["kappa"], theta["gamma"], theta["sigma"]), (t32(1.0), t32(0.3)))

    configs = [("RandomWalk", RandomWalk(0.05), False), ("RandomWalk, states recorded", RandomWalk(0.05), True),
               ('GradientBasedProposal("fl")', GradientBasedProposal(0.05, "fl"), True),
               ('GradientBasedProposal("ffbs")', GradientBasedProposal(0.05, "ffbs"), True)]
    configs += [(f'GradientBasedProposal("ffbs-mh", mcmc_steps={k})', GradientBasedProposal(0.05, "ffbs-mh", mcmc_steps=k), True) for k in ROUNDS]
    return pmmh_lines("Ornstein-Uhlenbeck", build, priors, y, configs, moves)


def tracker_pmmh(lin, moves):
    from torch.distributions import LogNormal

    from pyfilter_amd.inference import GradientBasedProposal

    priors = {"phi": LogNormal(math.log(0.9), 0.05), "q": LogNormal(math.log(0.3), 0.2), "r": LogNormal(math.log(0.5), 0.2)}
    configs = [('GradientBasedProposal("fl")', GradientBasedProposal(0.05, "fl"), True),
               ('GradientBasedProposal("ffbs", route="kernel")', GradientBasedProposal(0.05, "ffbs", route="kernel"), True)]
    configs += [(f'GradientBasedProposal("ffbs-mh", mcmc_steps={k})', GradientBasedProposal(0.05, "ffbs-mh", mcmc_steps=k), True) for k in ROUNDS]
    return pmmh_lines("constant-velocity tracker D = 4", lin.cv_builder(), priors, lin.cv_data(100), configs, moves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moves", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lin = _tool("linear_smooth_bench")
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
    filt, states = sine_recorded(64, 1024, 100)
    emit(smooth_lines("sine diffusion", filt, states, (64, 1024, 100), a.reps))
    filt, states = lin.recorded(lin.cv_builder(), lin.cv_theta(64), 64, 1024, lin.cv_data(100))
    emit(smooth_lines("constant-velocity tracker D = 4", filt, states, (64, 1024, 100), a.reps, route="kernel"))
    del filt, states
    emit(ou_pmmh(a.moves))
    emit(tracker_pmmh(lin, a.moves))
    filt, states = sine_recorded(8, 65536, 50)
    emit(smooth_lines("sine diffusion", filt, states, (8, 65536, 50), a.reps))


if __name__ == "__main__":
    main()
