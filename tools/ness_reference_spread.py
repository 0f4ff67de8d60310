"""
Development (no GPU): how far the posterior means of the **unmodified reference's** NESS lie from those of its SMC^2 on the
same data, over repeated runs - the number ``tests/test_ness_gpu.py::test_ness_agrees_with_smc2_on_simulated_ou_data`` takes
its bound from.  Writes ``profiles/ness_reference_spread.txt``.

    python tools/ness_reference_spread.py [--theta 200] [--particles 200] [--steps 400] [--seeds 6] [--smc2-theta B --smc2-particles N]

The model, priors and data generator are those of ``tools/make_golden_ness.py`` (Ornstein-Uhlenbeck observed with noise).  One
SMC^2 run (threshold 0.5, the reference's defaults otherwise) gives the posterior mean and standard deviation of every
parameter (constrained space); every NESS run (defaults: threshold 0.9, ``NonShrinkingKernel``) gives its posterior mean; the
figure per run and parameter is ``|mean_NESS - mean_SMC2| / sd_SMC2``.
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("PF_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=200)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--smc2-theta", type=int, default=None, help="SMC2's own size (default: NESS's): its re-filters are what costs")
    ap.add_argument("--smc2-particles", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ness_reference_spread.txt"))
    args = ap.parse_args()

    import math

    import torch

    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shim"))
    sys.path.insert(1, REFERENCE)
    import pyfilter  # noqa: F401  (the reference)
    from pyfilter import inference as inf
    from pyfilter.filters.particle import APF, proposals
    from pyfilter.utils import normalize
    from pyro.distributions import Exponential, LogNormal, Normal
    from stochproc import timeseries as ts

    def ou(kappa, gamma, sigma, dt=1.0):
        def ms(x, k, g, s):
            e = torch.exp(-k * dt)
            return g + (x.value - g) * e, s * torch.sqrt((1.0 - torch.exp(-2.0 * k * dt)) / (2.0 * k))

        inc = torch.distributions.Normal(torch.tensor(0.0), torch.tensor(1.0))
        return ts.AffineProcess(ms, (kappa, gamma, sigma), inc, lambda k, g, s: torch.distributions.Normal(g, s / torch.sqrt(2.0 * k)))

    def build_model(cntxt):
        kappa = cntxt.named_parameter("kappa", Exponential(rate=10.0))
        gamma = cntxt.named_parameter("gamma", Normal(loc=0.0, scale=1.0))
        sigma = cntxt.named_parameter("sigma", LogNormal(loc=-2.0, scale=1.0))
        return ts.LinearStateSpaceModel(ou(kappa, gamma, sigma), (torch.tensor(1.0), torch.tensor(0.05)), torch.Size([]))

    def simulate(t_len, seed):
        g = torch.Generator().manual_seed(seed)
        x, ys = 0.0, []
        for _ in range(t_len):
            x = x * math.exp(-0.025) + 0.05 * math.sqrt((1 - math.exp(-0.05)) / 0.05) * torch.randn((), generator=g).item()
            ys.append(x + 0.05 * torch.randn((), generator=g).item())
        return torch.tensor(ys)

    y = simulate(args.steps, 4242)

    def run(make, seed, particles):
        torch.manual_seed(seed)
        with inf.make_context() as context:
            filt = APF(build_model, particles, proposal=proposals.LinearGaussianObservations())
            alg = make(filt)
            state = alg.initialize()
            for t in range(y.shape[0]):
                state = alg.step(y[t], state)
            w = normalize(state.w)
            theta = context.stack_parameters(constrained=True)
            mean = (w.unsqueeze(-1) * theta).sum(0)
            sd = (w.unsqueeze(-1) * (theta - mean) ** 2).sum(0).sqrt()
            return mean, sd, list(context.parameters.keys())

    lines = [f"reference NESS against reference SMC2: OU data, T = {args.steps}, {args.theta} theta-particles x {args.particles} state particles (APF, "
             f"LinearGaussianObservations), float32, CPU", ""]
    t0 = time.time()
    b2, n2 = args.smc2_theta or args.theta, args.smc2_particles or args.particles
    m2, s2, names = run(lambda f: inf.sequential.SMC2(f, b2, threshold=0.5), 1, n2)
    lines.append(f"SMC2 ({b2} x {n2}, seed 1, {time.time() - t0:.0f} s): " + ", ".join(f"{n} mean {float(m):.5f} sd {float(s):.5f}" for n, m, s in zip(names, m2, s2)))
    worst, figures = 0.0, []
    for seed in range(1, args.seeds + 1):
        t0 = time.time()
        m, s, _ = run(lambda f: inf.sequential.NESS(f, args.theta), 100 + seed, args.particles)
        z = (m - m2).abs() / s2
        worst = max(worst, float(z.max()))
        figures += [float(v) for v in z]
        lines.append(f"NESS seed {100 + seed} ({time.time() - t0:.0f} s): " + ", ".join(f"{n} mean {float(a):.5f} (own sd {float(b):.5f}) |dz| {float(c):.2f}"
                                                                                      for n, a, b, c in zip(names, m, s, z)))
    import statistics

    mean, sd = statistics.mean(figures), statistics.stdev(figures)
    lines += ["", f"largest |mean_NESS - mean_SMC2| / sd_SMC2 over {args.seeds} seeds and {len(names)} parameters: {worst:.2f}",
              f"mean {mean:.2f}, standard deviation {sd:.2f} of the {len(figures)} figures; mean + 3 sd = {mean + 3 * sd:.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
