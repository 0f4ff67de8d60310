#!/usr/bin/env python
"""Times the path score (``pf_path_score``, ``csrc/pf_score.hpp``) against torch autograd of the same expression
(``ParticleFilter.path_score(route="torch")``) on the same GPU and inputs, float32:

    sine diffusion   S = 251, N = 1 024,  B = 256, D = 1
    Lorenz-63        S = 101, N = 65 536, B = 1,   D = 3

Trajectories are simulated from the model on the device.  Per shape: the kernel alone (its two launches on the kernel's own
layout; device events, median of the repeats after a warm-up), ``path_score`` with the gradient by parameter name on either
route (layout copy, model builder and vector-Jacobian product included), the device's copy rate on a buffer of the paths' size
(bytes read + written over time), and ``S D B N sizeof(T) / kernel time`` as a fraction of the 8 TB/s HBM peak.
Then the time of one PMMH move at 64 chains x 1 024 particles x T = 100 with ``RandomWalk`` and with ``GradientBasedProposal``
under either smoother (a host clock around moves that end in a device synchronise).

    python tools/path_score_bench.py [--reps 20] [--out FILE]           # recorded in profiles/path_score.txt
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def t32(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def sine(theta):
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    return ts.LinearStateSpaceModel(models.SineDiffusion(theta["gamma"], theta["sigma"], dt=0.1), (t32(1.0), t32(0.1))).to("cuda")


def lorenz(theta):
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    hidden = models.Lorenz63(theta["s"], theta["r"], theta["b"], theta["sigma"], dt=0.01)
    return ts.LinearStateSpaceModel(hidden, (t32([1.0, 0.0, 0.0]), t32(0.5))).to("cuda")


def simulate(model, s, n, b):
    """``(paths (S, N, [B], [D]), y (S - 1, [O]))`` from the model itself (float32, on the device)."""
    torch.manual_seed(1)
    hidden = model.hidden
    x = hidden.initial_sample(torch.Size([n] + ([b] if b > 1 else [])))
    xs = [x.value]
    for _ in range(s - 1):
        x = hidden.propagate(x)
        xs.append(x.value)
    paths = torch.stack(xs, 0)
    first = paths[1:, 0, 0] if b > 1 else paths[1:, 0]
    y = model.build_density(ts_state(first, hidden)).sample()
    return paths, y


def ts_state(values, hidden):
    from pyfilter_amd.timeseries import TimeseriesState

    return TimeseriesState(0, values, hidden.event_shape)


def events(fn, reps, warm=3):
    for _ in range(warm):
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
    return statistics.median(out), min(out)


def shape_lines(name, builder, theta, s, n, b, reps):
    from pyfilter_amd import ops
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.filters.particle.forecast import tape_soa
    from pyfilter_amd.timeseries.models import pack_params

    filt = SISR(builder, n)
    if b > 1:
        filt.set_batch_shape(torch.Size([b]))
    filt.initialize_model(theta)
    model = filt.ssm
    paths, y = simulate(model, s, n, b)
    kind = model.kernel_kind
    soa = tape_soa(paths, paths, b > 1, model.hidden.n_dim > 0)
    rows = pack_params(model, b, torch.float32, paths.device)
    nbytes = soa.numel() * soa.element_size()
    other = torch.empty_like(soa)
    routes = [("kernel alone (pf_path_score, its own layout)", lambda: ops.path_score(kind, rows, soa, y)),
              ("path_score(theta), kernel route", lambda: filt.path_score(paths, y, theta=theta)),
              ("path_score(theta), torch route", lambda: filt.path_score(paths, y, theta=theta, route="torch")),
              ("device copy of the paths", lambda: other.copy_(soa))]
    got = {label: events(fn, reps) for label, fn in routes}
    lines = [f"{name}: S = {s}, N = {n}, B = {b}, D = {kind.dim}, float32; paths {nbytes / 1e6:.1f} MB; ms per call, median (min) of {reps}"]
    for label, (med, lo) in got.items():
        lines.append(f"  {label:48s} {med:9.4f} ({lo:.4f})")
    k = got[routes[0][0]][0] * 1e-3
    c = got[routes[3][0]][0] * 1e-3
    lines.append(f"  kernel: {nbytes / k / 1e12:.3f} TB/s of paths read = {100 * nbytes / k / PEAK:.1f} % of the 8 TB/s peak; "
                 f"device copy: {2 * nbytes / c / 1e12:.3f} TB/s read + written")
    lines.append(f"  torch route / kernel route: {got[routes[2][0]][0] / got[routes[1][0]][0]:.1f} x; torch route / kernel alone: "
                 f"{got[routes[2][0]][0] / got[routes[0][0]][0]:.1f} x")
    a, g = filt.path_score(paths, y, theta=theta), filt.path_score(paths, y, theta=theta, route="torch")
    worst = max(float(((a[1][k_] - g[1][k_]).abs() / g[1][k_].abs().clamp_min(1e-30)).max()) for k_ in theta)
    lines.append(f"  largest relative difference of the two routes' gradients by name: {worst:.2e} (the torch route computes in float32)")
    return lines


def pmmh_lines(moves):
    from torch.distributions import LogNormal, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.inference import PMMH, GradientBasedProposal, RandomWalk, run_pmmh
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

    lines = [f"PMMH, Ornstein-Uhlenbeck, 64 chains x 1 024 particles x T = 100, float32: ms per move (host clock, {moves} moves, synchronised)"]
    for label, proposal, record in (("RandomWalk", RandomWalk(0.05), False), ("RandomWalk, states recorded", RandomWalk(0.05), True),
                                    ('GradientBasedProposal("ffbs")', GradientBasedProposal(0.05, "ffbs"), True),
                                    ('GradientBasedProposal("fl")', GradientBasedProposal(0.05, "fl"), True)):
        alg = PMMH(SISR(build, 1024, record_states=record, seed=1), moves, priors, num_chains=64, proposal=proposal, seed=2)
        state = alg.initialize(y)
        kernel = proposal.build(alg.theta, state, alg.filter, y)
        ptheta, pfilter = alg.theta.like(), alg.filter.copy()
        pfilter.initialize_model(ptheta)

        def move():
            return run_pmmh(alg.theta, state, proposal, kernel, pfilter, ptheta, y, alg.filter.batch_shape, mutate_kernel=True, generator=alg._gen)

        for _ in range(3):
            move()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(moves):
            move()
        torch.cuda.synchronize()
        lines.append(f"  {label:34s} {(time.perf_counter() - t0) / moves * 1e3:9.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    lines += shape_lines("sine diffusion", sine, {"gamma": t32(0.5), "sigma": t32(0.4)}, 251, 1024, 256, a.reps)
    lines += shape_lines("Lorenz-63", lorenz, {"s": t32(10.0), "r": t32(28.0), "b": t32(8.0 / 3.0), "sigma": t32(1.0)}, 101, 65536, 1, a.reps)
    lines += pmmh_lines(a.moves)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
