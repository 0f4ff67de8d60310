"""NESS on the GPU (``pyfilter_amd.inference.ness`` on the HIP filters and ``csrc/pf_jitter.hpp``): the reference's event logs
replayed on both theta routes, the jittering kernels against the torch route on seeded random inputs, the fast online path
against the plain ``filter()`` path, reproducibility per seed and one statistical end-to-end run against ``SMC2``."""
import math

import pytest
import torch

from tests.ness_replay import NESS_CASES, replay_ness
from tests.replay import close, taped

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["theta_kernels", "theta_torch"])
def theta_route(request):
    """Both theta routes: the update's arithmetic in ``pf_theta_resample / pf_jitter_fit / pf_jitter_apply`` (taken for the scalar
    Exponential / Normal / LogNormal priors of these cases) and in torch operations."""
    from pyfilter_amd.hints import HINTS

    HINTS.theta_kernels = request.param == "theta_kernels"
    yield request.param
    HINTS.theta_kernels = True


def _ou_builder(dtype):
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    def build(theta):  # tests/inference/models.py:22-33 (the OU process with its stationary initial distribution)
        t = lambda v: torch.tensor(v, dtype=dtype, device="cuda")  # noqa: E731
        return ts.LinearStateSpaceModel(models.OrnsteinUhlenbeck(theta["kappa"], theta["gamma"], theta["sigma"], dt=1.0), (t(1.0), t(0.05)))

    return build


def _hip_filter(cursor, n):
    from pyfilter_amd.filters.particle import APF, proposals

    cls = taped(APF)
    cls.cursor = cursor
    return cls(_ou_builder(torch.float64), n, proposal=proposals.LinearGaussianObservations())


@pytest.mark.parametrize("name", sorted(NESS_CASES))
def test_ness_on_the_hip_filters_replays_the_reference_event_log(name, theta_route):
    updates, routes = replay_ness(name, _hip_filter, "cuda", rtol=1e-7)
    assert updates >= 3
    assert routes == ({"kernels"} if theta_route == "theta_kernels" else {"torch"})


# ---- the jittering kernels against the torch route -------------------------------------------------------------------------------
FAMILIES = ["nonshrinking", "shrinking", "liuwest", "constant", "constant_vector"]
SIZES = [7, 48, 250, 1000, 4096, 8192]  # (the last one: _lib.JITTER_MAXB, the most pf_jitter_fit sorts in LDS)
GAP = 1e-9
_skipped, _ran = [], []


def _priors(p):
    from torch.distributions import Beta, Exponential, Gamma, HalfNormal, LogNormal, Normal, Uniform

    pool = [Normal(0.0, 1.0), LogNormal(-2.0, 1.0), Exponential(10.0), Gamma(2.0, 3.0), HalfNormal(1.0), Beta(2.0, 3.0), Uniform(-1.0, 2.0),
            Normal(0.5, 2.0)]
    return {f"p{k}": pool[k] for k in range(p)}


def _kernel(family, p):
    from pyfilter_amd.inference import ConstantKernel, LiuWestShrinkage, NonShrinkingKernel, ShrinkingKernel

    if family == "constant":
        return ConstantKernel(0.125)
    if family == "constant_vector":
        return ConstantKernel(torch.arange(1, p + 1, dtype=torch.float64) / 16)  # (exact in float32 too)
    return {"nonshrinking": NonShrinkingKernel, "shrinking": ShrinkingKernel, "liuwest": LiuWestShrinkage}[family]()


def _inputs(b, p, special, seed):
    """float64 CPU inputs: values ``randn(B, P)``, log-weights ``2 randn(B)`` (weights ``softmax(2 randn(B))``), ancestors by
    systematic resampling, the draws."""
    from pyfilter_amd.inference.utils import theta_normalize, theta_systematic

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, p, generator=g, dtype=torch.float64)
    lw = 2.0 * torch.randn(b, generator=g, dtype=torch.float64)
    if special == "nonfinite":  # weights with -inf / NaN entries (a filter that lost every particle)
        bad = torch.rand(b, generator=g) < 0.15
        bad[0] = True
        lw[bad] = -math.inf
        lw[torch.randint(0, b, (1,), generator=g)] = math.nan
        if b > 3:
            lw[b // 2] = 0.5  # (at least one particle carries weight)
    elif special == "constant_column":  # every theta-particle agrees in column 0: zero variance -> the min_std clamp
        x[:, 0] = 0.75
    elif special == "duplicates":  # the state right after a resampling without jitter
        x = x[theta_systematic(theta_normalize(2.0 * torch.randn(b, generator=g, dtype=torch.float64)), torch.tensor(0.4, dtype=torch.float64))]
    idx = theta_systematic(theta_normalize(lw), torch.tensor(0.37, dtype=torch.float64))
    eps = torch.randn(b, p, generator=g, dtype=torch.float64)
    sel = (torch.rand(b, generator=g) < b ** -0.5).double()
    return x, lw, idx, eps, sel


def _quartile_gap(x, w):
    """How well-conditioned the two quartile picks of ``robust_var`` are (float64 torch result): the smallest margin by which the
    picked position's ``|cdf - q|`` beats that of a position holding ANOTHER value (a position with the same value gives the same
    quartile; one whose weight does not move the cdf repeats its predecessor and can only be picked when it comes first)."""
    srt, order = x.sort(dim=0, stable=True)
    cdf = w[order].cumsum(0)
    gap = math.inf
    for q in (0.25, 0.75):
        d = (cdf - q).abs()
        best = d.argmin(0)
        for c in range(x.shape[1]):
            moved = torch.ones(x.shape[0], dtype=torch.bool)
            moved[1:] = cdf[1:, c] != cdf[:-1, c]
            other = (srt[:, c] != srt[best[c], c]) & moved
            if other.any():
                gap = min(gap, float((d[other, c] - d[best[c], c]).min()))
    return gap


def _torch_route(kernel, pri, x, lw, idx, eps, sel, discrete, dtype):
    """The update's arithmetic as the torch route does it, on float64 CPU tensors: jittered (unconstrained, constrained)."""
    from pyfilter_amd.inference import ThetaParticles
    from pyfilter_amd.inference.utils import theta_normalize

    w = theta_normalize(lw)
    jittered = kernel.jitter(x, w, idx, eps)
    if discrete:
        to_jitter = sel.unsqueeze(-1)
        jittered = (1 - to_jitter) * x[idx] + to_jitter * jittered
    theta = ThetaParticles(pri, x.shape[0], "cpu", torch.float64).initialize_parameters(torch.Generator().manual_seed(0))
    theta.unstack_parameters(jittered, constrained=False)
    return jittered, theta.stack_parameters(True), kernel.last_fit, w


def _kernel_route(kernel, pri, x, lw, idx, eps, sel, discrete, dtype):
    from pyfilter_amd import ops
    from pyfilter_amd.inference import ThetaParticles
    from pyfilter_amd.inference.ness import _eps_of

    b, p = x.shape
    theta = ThetaParticles(pri, b, "cuda", dtype).initialize_parameters(torch.Generator().manual_seed(0))
    native = theta.native_priors()
    assert native is not None
    kind, par, scale = kernel.native(dtype)
    dev = lambda t: t.to(device="cuda", dtype=dtype)  # noqa: E731
    e = _eps_of(dtype)
    fit, mean, scale_out = ops.jitter_fit(dev(x), dev(lw), kind, par, scale, kernel.min_std(dtype), (e, 1 - e))
    out = [torch.empty(b, device="cuda", dtype=dtype) for _ in range(p)]
    u = ops.jitter_apply(native, dev(x), idx.cuda(), fit, kind, par, out, discrete, dev(eps), dev(sel) if discrete else None, 0, 0, (e, 1 - e))
    return u, torch.stack(out, dim=1), fit


@pytest.mark.parametrize("special", ["plain", "nonfinite", "constant_column", "duplicates"])
@pytest.mark.parametrize("discrete", [False, True], ids=["all", "discrete"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("p", [1, 3, 8])
@pytest.mark.parametrize("b", SIZES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_jitter_kernels_match_the_torch_route(dtype, b, p, family, discrete, special):
    """``pf_jitter_fit`` + ``pf_jitter_apply`` against ``JitterKernel.jitter`` and the priors' bijections in float64 torch.

    float64: the replay bar of the theta-level quantities (rtol 1e-8, atol 1e-10).  float32: the kernels compute in double from
    the float32 inputs and round once, so the result is the float64 torch result of the same (float32) inputs rounded to
    float32, to 1 ulp: rtol 2^-22, atol 0.  A case whose quartile pick is ill-conditioned (``_quartile_gap`` below 1e-9: the
    summation order decides, which is not a property of the algorithm) is skipped; ``test_few_cases_were_ill_conditioned``
    bounds how many."""
    specials = ["plain", "nonfinite", "constant_column", "duplicates"]
    seed = b * 7919 + p * 104729 + FAMILIES.index(family) * 31 + int(discrete) * 7 + specials.index(special)
    x, lw, idx, eps, sel = _inputs(b, p, special, seed)
    if dtype == torch.float32:  # the float32 inputs both sides start from
        x, lw, eps = x.float().double(), lw.float().double(), eps.float().double()
    pri = _priors(p)
    kernel, ref_kernel = _kernel(family, p), _kernel(family, p)
    want_u, want_x, (_, scale, std), w = _torch_route_dtype(ref_kernel, pri, x, lw, idx, eps, sel, discrete, dtype)
    _ran.append(1)
    if not family.startswith("constant") and _quartile_gap(x, w) < GAP:
        _skipped.append((dtype, b, p, family, discrete, special))
        pytest.skip("ill-conditioned quartile pick")
    got_u, got_x, fit = _kernel_route(kernel, pri, x, lw, idx, eps, sel, discrete, dtype)
    what = f"B={b} P={p} {family} discrete={discrete} {special}"
    close(fit[1], scale.expand(p), f"{what}: scale")
    close(fit[2], std.expand(p), f"{what}: std")
    if special == "constant_column" and not family.startswith("constant"):
        assert float(fit[2][0]) == kernel.min_std(dtype), "a column without variance jitters with the smallest allowed std"
    if dtype == torch.float64:
        close(got_u, want_u, f"{what}: jittered (unconstrained)")
        close(got_x, want_x, f"{what}: jittered (constrained)")
    else:
        tol = dict(rtol=2.0 ** -22, atol=0.0)
        torch.testing.assert_close(got_u.cpu(), want_u.float(), msg=lambda m: f"{what}: jittered (unconstrained): {m}", **tol)
        torch.testing.assert_close(got_x.cpu(), want_x.float(), msg=lambda m: f"{what}: jittered (constrained): {m}", **tol)


def _torch_route_dtype(kernel, pri, x, lw, idx, eps, sel, discrete, dtype):
    """``_torch_route`` in float64 with the constants of a run in ``dtype`` (EPS: the std threshold and the bandwidth clamp)."""
    if dtype == torch.float64:
        return _torch_route(kernel, pri, x, lw, idx, eps, sel, discrete, dtype)
    from pyfilter_amd.inference import ness

    real = ness._eps_of
    ness._eps_of = lambda _dtype: real(torch.float32)
    try:
        return _torch_route(kernel, pri, x, lw, idx, eps, sel, discrete, dtype)
    finally:
        ness._eps_of = real


def test_few_cases_were_ill_conditioned():
    """Runs after the comparison above (file order): at most 1 % of its cases may have been skipped."""
    if not _ran:
        pytest.skip("the comparison did not run in this session")
    assert len(_skipped) <= 0.01 * len(_ran), (len(_skipped), len(_ran), _skipped[:10])


def test_more_theta_particles_than_the_kernels_sort_take_the_torch_route():
    from pyfilter_amd import _lib, ops

    b = _lib.JITTER_MAXB + 1
    with pytest.raises(AssertionError):
        ops.jitter_fit(torch.zeros(b, 1, device="cuda"), torch.zeros(b, device="cuda"), _lib.JITTER_NONSHRINKING)
    rc = _lib.load().pf_jitter_fit(1, 1, b, 1, 0, 0.0, None, 0.0, 0.0, 1.0, _lib.PF_F32, 1, None, None, None)
    assert rc != 0  # PF_EINVAL before anything is launched


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _ou_data(t_len, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x, ys = 0.0, []
    for _ in range(t_len):
        x = x * math.exp(-0.025) + 0.05 * math.sqrt((1 - math.exp(-0.05)) / 0.05) * float(torch.randn((), generator=g))
        ys.append(x + 0.05 * float(torch.randn((), generator=g)))
    return torch.tensor(ys, dtype=dtype, device="cuda")


def _ness(n_theta, n_state, dtype, seed, **kwargs):
    from torch.distributions import Exponential, LogNormal, Normal

    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.inference import NESS

    pri = {"kappa": Exponential(10.0), "gamma": Normal(0.0, 1.0), "sigma": LogNormal(-2.0, 1.0)}
    filt = APF(_ou_builder(dtype), n_state, proposal=proposals.LinearGaussianObservations(), seed=11 + seed)
    return NESS(filt, n_theta, pri, device="cuda", dtype=dtype, seed=seed, **kwargs), pri


@pytest.mark.parametrize("discrete", [False, True], ids=["all", "discrete"])
def test_the_fast_online_path_is_the_plain_filter_path_draw_for_draw(discrete, monkeypatch):
    """``NESS.step`` through the fast driver (one ``pf_filter_observe`` per observation; after an update it re-attaches to the
    gathered state and reads the rewritten parameters) against the same loop over ``filter()`` (the driver switched off), the
    particle-level draws injected into both and the theta-level draws keyed by (seed, update): the same updates at the same
    observations, the same ancestors, theta, weights and filter state - float64, at the replay tolerances."""
    from pyfilter_amd.filters.particle import base as pbase

    dtype, b, n, t_len = torch.float64, 64, 256, 90
    y = _ou_data(t_len, 9, dtype)
    g = torch.Generator().manual_seed(77)
    z0 = torch.randn(n, b, generator=g, dtype=dtype).cuda()
    z = torch.randn(t_len + 1, n, b, generator=g, dtype=dtype).cuda()
    u = torch.rand(t_len + 1, b, generator=g, dtype=dtype).cuda()
    outs = {}
    for how in ("fast", "plain"):
        if how == "plain":
            monkeypatch.setattr(pbase._OnlineRun, "applies", staticmethod(lambda filt, result: False))
        alg, _ = _ness(b, n, dtype, 5, discrete=discrete)
        alg.filter.set_tape(z=z, u=u, z0=z0)
        alg._kernel.trace = []
        state = alg.initialize()
        used, when = 0, []
        for k in range(t_len):
            before = alg._kernel.updates
            state = alg.step(y[k], state)
            used += state._online is not None
            if alg._kernel.updates != before:
                when.append(k)
        assert (used > t_len // 2) == (how == "fast"), (how, used)
        assert {tr["route"] for tr in alg._kernel.trace} == {"kernels"}
        fs = state.filter_state
        outs[how] = dict(when=when, idx=[tr["indices"].cpu() for tr in alg._kernel.trace], w=state.w.cpu(), ess=torch.stack(state.ess).cpu(),
                         theta=alg.theta.stack_parameters(True).cpu(), ll=fs.loglikelihood.cpu(), means=fs.filter_means.cpu(),
                         x=fs.latest_state.timeseries_state.value.cpu(), lw=fs.latest_state.weights.cpu())
    a, c = outs["fast"], outs["plain"]
    assert len(a["when"]) >= 5 and a["when"] == c["when"], (a["when"], c["when"])
    assert all(torch.equal(i, j) for i, j in zip(a["idx"], c["idx"])), "theta ancestors"
    assert a["means"].shape == c["means"].shape == (t_len + 1, b, 1)
    # (NaN in both: a theta-particle jittered to where its filter breaks down - its weight counts as -inf from then on)
    for key in ("theta", "w", "ess"):
        torch.testing.assert_close(a[key], c[key], rtol=1e-8, atol=1e-10, equal_nan=True, msg=lambda m, key=key: f"{key}: {m}")
    for key in ("ll", "means", "x", "lw"):
        torch.testing.assert_close(a[key], c[key], rtol=1e-7, atol=1e-9, equal_nan=True, msg=lambda m, key=key: f"{key}: {m}")


def test_a_run_is_a_function_of_its_seed():
    dtype, t_len = torch.float32, 60
    y = _ou_data(t_len, 3, dtype)
    outs = []
    for seed in (4, 4, 5):
        alg, _ = _ness(96, 200, dtype, seed)
        state = alg.fit(y)
        assert alg._kernel.updates >= 5 and alg._kernel.last_route == "kernels"
        outs.append((alg.theta.stack_parameters(True).cpu(), state.w.cpu(), state.filter_state.loglikelihood.cpu()))
    for p, q in zip(outs[0], outs[1]):  # two runs with one seed are identical, bit for bit (NaN - a broken-down filter - in both)
        torch.testing.assert_close(p, q, rtol=0.0, atol=0.0, equal_nan=True)
    assert torch.isfinite(outs[0][0]).all()
    assert not torch.equal(outs[0][0], outs[2][0]) and not torch.equal(outs[0][1], outs[2][1]), "two seeds differ"


# profiles/ness_reference_spread.txt: the reference's NESS (1 000 x 400, T = 1 000, float32, CPU, 5 seeds) against the reference's SMC2 on
# the data of this test - |mean_NESS - mean_SMC2| / sd_SMC2 per seed and parameter: largest 1.54, mean 0.76, standard deviation 0.36
# of the 15 figures.  The bound is their mean + 3 standard deviations (the largest of 15 draws is a bound a sixteenth equally good
# run would miss with probability 1 / 16).
REFERENCE_SPREAD = 1.84


def test_ness_agrees_with_smc2_on_simulated_ou_data():
    """NESS (1 000 theta x 400 state particles, float32, T = 1 000) against ``SMC2`` on the same simulated OU data: the posterior
    mean of every parameter within ``REFERENCE_SPREAD`` posterior standard deviations (of the SMC^2 posterior) of SMC^2's.

    The bound is what repeated runs of the REFERENCE's own NESS show against the reference's SMC^2 on the same data
    (``tools/ness_reference_spread.py`` -> ``profiles/ness_reference_spread.txt``; CPU, float32, NESS at 1 000 x 400, T = 1 000, 5
    seeds; SMC^2 at 150 x 150): ``|mean_NESS - mean_SMC2| / sd_SMC2`` per seed for (kappa, gamma, sigma) = (1.54, 1.04, 1.10),
    (0.41, 1.06, 0.47), (0.79, 1.17, 0.41), (0.49, 0.79, 0.77), (0.26, 0.63, 0.43) - largest 1.54, mean 0.76, standard deviation
    0.36; ``REFERENCE_SPREAD`` is their mean + 3 standard deviations, 1.84.  (At 150 x 150, T = 300 the reference's NESS leaves
    the posterior altogether - kappa above 1e12 in 2 of 5 seeds -, so no bound can be read off a smaller size.)"""
    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.inference import SMC2
    from pyfilter_amd.inference.utils import theta_normalize

    dtype, t_len = torch.float32, 1000
    y = _ou_data(t_len, 4242, dtype)
    alg, pri = _ness(1000, 400, dtype, 1)
    state = alg.fit(y)
    assert alg._kernel.updates >= 50 and alg._kernel.last_route == "kernels"
    mean_ness = alg.posterior_mean(state).double().cpu()
    smc2 = SMC2(APF(_ou_builder(dtype), 400, proposal=proposals.LinearGaussianObservations(), seed=21), 1000, pri, threshold=0.5, device="cuda",
                dtype=dtype, seed=2)
    s2 = smc2.fit(y)
    w = theta_normalize(s2.w).double().cpu()
    th = smc2.theta.stack_parameters(True).double().cpu()
    mean2 = w @ th
    sd2 = (w @ (th - mean2) ** 2).sqrt()
    z = (mean_ness - mean2).abs() / sd2
    print(f"NESS {mean_ness.tolist()} SMC2 {mean2.tolist()} sd {sd2.tolist()} |dz| {z.tolist()} updates {alg._kernel.updates}")
    assert torch.isfinite(z).all() and float(z.max()) <= REFERENCE_SPREAD, (z.tolist(), REFERENCE_SPREAD)
