#!/usr/bin/env python
"""Times what follows the filter for a ``LinearModel`` (``PF_HID_LINEAR_MAT``, ``csrc/pf_linear_smooth.hpp``) on either route, on the
same GPU, inputs and process, float32:

* ``smooth(states, "ffbs", route="kernel")`` (``pf_smooth_ffbs_linear``) against ``route="torch"`` (the reference's ``(N, N, B, D)``
  logits with torch ops): the 4-D constant-velocity model, 8 filters x 1 024 particles x T = 50 - and the kernel route alone at
  64 x 1 024 x T = 100;
* ``path_score(theta=..., route="kernel")`` (``pf_path_score_linear``) against ``route="torch"`` at 64 x 1 024 x T = 100 for
  D = 4, O = 2 and for a dense D = O = 8 model, and the kernel alone on its own layout;
* one PMMH move with ``GradientBasedProposal(method="ffbs")``, ``route="kernel"`` against ``"auto"``, 64 chains x 1 024 x T = 100.

Device events (or, for the PMMH moves, a host clock around moves that end in a device synchronise), a warm-up, the median of the
repeats.

    python tools/linear_smooth_bench.py [--reps 10] [--out FILE]           # recorded in profiles/linear_smooth.txt
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

F32 = torch.float32


def t32(v):
    return torch.tensor(v, dtype=F32, device="cuda")


def cv_builder():
    """Constant velocity in the plane, positions observed: velocities decay by ``phi``, process noise ``q``, observation noise ``r``."""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    shift = t32([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    decay = t32([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    noise, h = t32([0.5, 0.5, 1.0, 1.0]), t32([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])
    m0, s0 = t32([0.0, 0.0, 1.0, -0.5]), t32([0.5, 0.5, 0.5, 0.5])

    def build(theta):
        phi, q, r = (theta[k].reshape(-1) for k in ("phi", "q", "r"))
        a, s = shift + phi.reshape(-1, 1, 1) * decay, q.reshape(-1, 1) * noise
        inc = Independent(Normal(t32(0.0), t32(1.0)).expand(torch.Size([4])), 1)
        hidden = models.LinearModel((a, torch.zeros_like(s), s), inc, lambda *_: Independent(Normal(m0, s0), 1))
        return ts.LinearStateSpaceModel(hidden, (h, t32([0.0, 0.0]), r.reshape(-1, 1) * t32([1.0, 1.0])), torch.Size([2]))

    return build


def dense_builder(d, o):
    """A dense ``D x D`` transition and ``O x D`` observation matrix, one set per filter: ``theta = {A, s, so}``."""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    gen = torch.Generator().manual_seed(4)
    ao = torch.randn((o, d), generator=gen).to("cuda", F32)
    m0, s0 = torch.ones(d, device="cuda", dtype=F32), 0.5 * torch.ones(d, device="cuda", dtype=F32)

    def build(theta):
        inc = Independent(Normal(t32(0.0), t32(1.0)).expand(torch.Size([d])), 1)
        hidden = models.LinearModel((theta["A"], torch.zeros_like(theta["s"]), theta["s"]), inc, lambda *_: Independent(Normal(m0, s0), 1))
        return ts.LinearStateSpaceModel(hidden, (ao, torch.zeros(o, device="cuda", dtype=F32), theta["so"]), torch.Size([o]))

    return build


def cv_theta(b):
    gen = torch.Generator().manual_seed(3)
    spread = lambda: 1.0 + 0.05 * (2.0 * torch.rand(b, generator=gen) - 1.0)  # noqa: E731
    return {"phi": (0.9 * spread()).to("cuda", F32), "q": (0.3 * spread()).to("cuda", F32), "r": (0.5 * spread()).to("cuda", F32)}


def dense_theta(b, d, o):
    gen = torch.Generator().manual_seed(3)
    a = 0.9 * torch.eye(d) + 0.1 * torch.randn((b, d, d), generator=gen) / math.sqrt(d)
    return {"A": a.to("cuda", F32), "s": (0.3 + 0.3 * torch.rand((b, d), generator=gen)).to("cuda", F32),
            "so": (0.5 + 0.5 * torch.rand((b, o), generator=gen)).to("cuda", F32)}


def cv_data(t_obs):
    gen = torch.Generator().manual_seed(2024)
    x, ys = torch.tensor([0.0, 0.0, 1.0, -0.5]), []
    for _ in range(t_obs):
        x = torch.stack((x[0] + x[2], x[1] + x[3], 0.9 * x[2], 0.9 * x[3])) + 0.3 * torch.tensor([0.5, 0.5, 1.0, 1.0]) * torch.randn(4, generator=gen)
        ys.append(x[:2] + 0.5 * torch.randn(2, generator=gen))
    return torch.stack(ys).cuda()


def events(fn, reps, warm=2):
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


def recorded(builder, theta, b, n, y):
    from pyfilter_amd.filters.particle import SISR

    filt = SISR(builder, n, record_states=True, seed=1)
    filt.set_batch_shape(torch.Size([b]))
    filt.initialize_model(theta)
    return filt, list(filt.batch_filter(y, bar=False).states)


def smooth_lines(reps):
    lines = []
    build = cv_builder()
    for b, t_obs, both in ((8, 50, True), (64, 100, False)):
        filt, states = recorded(build, cv_theta(b), b, 1024, cv_data(t_obs))
        logits = 1024 * 1024 * b * 4 * 4
        lines.append(f'smooth(states, "ffbs"): constant velocity D = 4, {b} filters x 1 024 particles x T = {t_obs}, float32; ms per call, '
                     f"median (min) of {reps}")
        k = events(lambda: filt.smooth(states, "ffbs", route="kernel"), reps)
        lines.append(f'  {"route=kernel (pf_smooth_ffbs_linear, Philox)":48s} {k[0]:10.3f} ({k[1]:.3f})')
        if both:
            t = events(lambda: filt.smooth(states, "ffbs", route="torch"), reps)
            lines.append(f'  {"route=torch ((N, N, B, D) logits)":48s} {t[0]:10.3f} ({t[1]:.3f})')
            lines.append(f"  torch route / kernel route: {t[0] / k[0]:.1f} x; the torch route's residual tensor: {logits / 2 ** 20:.0f} MiB per backward step")
        else:
            lines.append(f"  route=torch was not run at this size: its residual tensor alone is {logits / 2 ** 30:.0f} GiB per backward step, with "
                         "the temporaries of log_prob and Categorical on top; it is part of the PMMH move below, nowhere else")
    return lines


def simulate(model, s, n, b):
    torch.manual_seed(1)
    hidden = model.hidden
    x = hidden.initial_sample(torch.Size([n, b]))
    xs = [x.value]
    for _ in range(s - 1):
        x = hidden.propagate(x)
        xs.append(x.value)
    paths = torch.stack(xs, 0)
    a, ob, os_ = model.parameters  # (the observations of path 0 of filter 0 under that filter's noise)
    xo = paths[1:, 0, 0]
    y = ob + (a @ xo.unsqueeze(-1)).squeeze(-1) + os_.reshape(-1, os_.shape[-1])[0] * torch.randn_like(xo[:, : a.shape[0]])
    return paths, y


def score_lines(name, builder, theta, d, reps, s=101, n=1024, b=64):
    from pyfilter_amd import ops
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.filters.particle.forecast import tape_soa
    from pyfilter_amd.timeseries.models import pack_params

    filt = SISR(builder, n)
    filt.set_batch_shape(torch.Size([b]))
    filt.initialize_model(theta)
    model = filt.ssm
    paths, y = simulate(model, s, n, b)
    kind = model.kernel_kind
    soa = tape_soa(paths, paths, True, True)
    rows = pack_params(model, b, F32, paths.device)
    nbytes = soa.numel() * soa.element_size()
    routes = [("kernel alone (pf_path_score_linear, its own layout)", lambda: ops.path_score_linear(kind, rows, soa, y)),
              ('path_score(theta), route="kernel"', lambda: filt.path_score(paths, y, theta=theta, route="kernel")),
              ('path_score(theta), route="torch"', lambda: filt.path_score(paths, y, theta=theta, route="torch"))]
    got = {label: events(fn, reps) for label, fn in routes}
    lines = [f"path_score: {name}, D = {kind.dim}, O = {kind.obs_dim}, S = {s}, N = {n}, B = {b}, float32; paths {nbytes / 1e6:.1f} MB; ms per call, "
             f"median (min) of {reps}"]
    for label, (med, lo) in got.items():
        lines.append(f"  {label:52s} {med:10.3f} ({lo:.3f})")
    lines.append(f"  torch route / kernel route: {got[routes[2][0]][0] / got[routes[1][0]][0]:.1f} x; torch route / kernel alone: "
                 f"{got[routes[2][0]][0] / got[routes[0][0]][0]:.1f} x")
    a, g = filt.path_score(paths, y, theta=theta, route="kernel"), filt.path_score(paths, y, theta=theta, route="torch")
    worst = max(float((a[1][k_] - g[1][k_]).abs().max() / g[1][k_].abs().max().clamp_min(1e-30)) for k_ in theta)
    lines.append(f"  largest difference of the two routes' gradients by name, relative to the largest entry: {worst:.2e} "
                 "(the torch route computes in float32)")
    return lines


def pmmh_lines(moves):
    from torch.distributions import LogNormal

    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.inference import PMMH, GradientBasedProposal, run_pmmh

    y = cv_data(100)
    priors = {"phi": LogNormal(math.log(0.9), 0.05), "q": LogNormal(math.log(0.3), 0.2), "r": LogNormal(math.log(0.5), 0.2)}
    lines = [f'PMMH, constant velocity D = 4, 64 chains x 1 024 particles x T = 100, float32, GradientBasedProposal(method="ffbs"): ms per move '
             f"(host clock, {moves} moves, synchronised)"]
    for route in ("kernel", "auto"):
        proposal = GradientBasedProposal(0.05, "ffbs", route=route)
        alg = PMMH(SISR(cv_builder(), 1024, record_states=True, seed=1), moves, priors, num_chains=64, proposal=proposal, seed=2)
        state = alg.initialize(y)
        kernel = proposal.build(alg.theta, state, alg.filter, y)
        ptheta, pfilter = alg.theta.like(), alg.filter.copy()
        pfilter.initialize_model(ptheta)

        def move():
            return run_pmmh(alg.theta, state, proposal, kernel, pfilter, ptheta, y, alg.filter.batch_shape, mutate_kernel=True, generator=alg._gen)

        move()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(moves):
            move()
        torch.cuda.synchronize()
        lines.append(f'  {"route=" + route:16s} {(time.perf_counter() - t0) / moves * 1e3:10.2f}')
        del alg, state, kernel, pfilter
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moves", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
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
    emit(smooth_lines(a.reps))
    emit(score_lines("constant velocity", cv_builder(), cv_theta(64), 4, a.reps))
    emit(score_lines("dense model", dense_builder(8, 8), dense_theta(64, 8, 8), 8, a.reps))
    emit(pmmh_lines(a.moves))


if __name__ == "__main__":
    main()
