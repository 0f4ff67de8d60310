"""The host oracle of the theta-level arithmetic (``tests/theta_oracle.py``) without a GPU:

* it reproduces what the REFERENCE recorded - every ``tests/golden/inference_smc2_* / _pmmh_* / _ness_*`` event log: ancestors,
  proposal mean and factor, theta*, reverse kernel, log acceptance probability, accepted mask, the NESS fit and jittered values -
  from the recorded inputs, at the replay tolerances of ``tests/replay.py``;
* its seven densities in unconstrained space agree with two independent statements, ``scipy.stats`` + the analytic log-Jacobian and
  ``mpmath`` at 50 digits, on u = -30 .. 30 and the parameter values of the GPU tests - the error against mpmath is the measured
  floor under the density bars of ``tests/test_theta_parity_gpu.py`` and must leave them a factor of 8;
* the product's torch route on CPU float64 computes the same (a disagreement between product and oracle shows without a GPU);
* the word tuples of the jitter kernels' Philox calls are injective and apart from every filter stream's;
* the INPUT CONDITIONS of the GPU comparisons hold on exactly their case list: few resampling positions within delta of a cdf
  entry, few ill-conditioned quartile picks.

Figures go to the file named by ``THETA_PARITY_REPORT`` when it is set (``profiles/theta_parity.txt`` is assembled from it)."""
import math
import os
import re

import numpy as np
import pytest

from tests import philox_ref as PR
from tests import theta_cases as TC
from tests import theta_oracle as O
from tests.ness_replay import CONSTANT_SCALE, NESS_CASES
from tests.source_registries import streams_in_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL, ATOL = 1e-8, 1e-10  # tests/replay.py::close
THETA_RTOL, THETA_ATOL = 1e-11, 1e-12  # the project's theta bar (tests/test_theta_kernels_gpu.py::_tol)
OU = ((O.EXPONENTIAL, 10.0, 0.0), (O.NORMAL, 0.0, 1.0), (O.LOGNORMAL, -2.0, 1.0))  # kappa, gamma, sigma: tests/ness_replay.py::priors
OU_KINDS, OU_A, OU_B = zip(*OU)


def report(line):
    path = os.environ.get("THETA_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line.rstrip() + "\n")


def close(got, want, what, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=rtol, atol=atol,
                               equal_nan=True, err_msg=what)


def events(name):
    out = {}
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as f:
        for key in f.files:
            m = re.fullmatch(r"e(\d+)::(\w+)::(\w+)", key)
            out.setdefault(int(m.group(1)), (m.group(2), {}))[1][m.group(3)] = f[key]
    return [out[k] for k in sorted(out)]


def unconstrain(theta):
    return np.stack([np.log(theta[:, 0]), theta[:, 1], np.log(theta[:, 2])], axis=1)


def ou_prior(u):
    return O.log_prior(OU_KINDS, OU_A, OU_B, u)[0]


def logs(prefix):
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith(prefix) and f.endswith(".npz"))


# ---- the reference's recordings ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", logs("inference_smc2_"))
def test_oracle_reproduces_the_recorded_smc2_rejuvenations(name):
    """mh.py:52-56 + run_pmmh: every quantity of every rejuvenation from the recorded inputs.  The state between events (theta and
    the main filters' log-likelihoods) is carried along from the log itself: ``move`` adds its increments, ``rejuvenate`` gathers
    by the ancestors, ``pmmh_accept`` / ``rejuvenated`` record what they left."""
    evs = events(name)
    assert list(evs[0][1]["names"]) == ["kappa", "gamma", "sigma"]
    theta = evs[0][1]["theta"].copy()
    ll = np.zeros(theta.shape[0])
    seen = dict(rejuvenate=0, pmmh=0)
    fwd = u_star = ll_star = None
    for kind, ev in evs[1:]:
        if kind == "move":
            ll = ll + ev["ll"]
        elif kind == "run":
            ll_star = ev["ll"]
        elif kind == "rejuvenate":
            with np.errstate(divide="ignore"):
                lw = np.log(ev["W"])
            idx, _, _ = O.systematic(lw, float(ev["u"]))
            assert np.array_equal(idx, ev["indices"]), f"{name}: theta ancestors"
            mean, chol, _ = O.fit(unconstrain(theta), lw, 1.1)  # symmetric_mh.py: construct_mvn(values, weights, scale=1.1)
            close(mean, ev["kernel_mean"], f"{name}: proposal mean")
            close(chol, ev["kernel_scale_tril"], f"{name}: proposal factor")
            theta, ll = theta[idx], ll[idx]
            seen["rejuvenate"] += 1
        elif kind == "pmmh_draw":
            fwd = (ev["kernel_loc"], ev["kernel_scale"])
            u_star, _ = O.propose(*fwd, ev["eps"])
            close(u_star, ev["rvs"], f"{name}: theta*")
            u_star = ev["rvs"]
        elif kind == "pmmh_accept":
            loc, fac, _ = O.fit(u_star, None, 1.1)  # (the reverse kernel: fit to theta* under the proposal state's zero log-weights)
            close(loc, ev["new_kernel_loc"], f"{name}: reverse kernel mean")
            close(fac, ev["new_kernel_scale"], f"{name}: reverse kernel factor")
            u_cur = unconstrain(theta)
            la, _ = O.log_accept(u_cur, u_star, fwd, (ev["new_kernel_loc"], ev["new_kernel_scale"]), ou_prior(u_cur), ou_prior(u_star),
                                 ll, ll_star)
            close(la, ev["log_acc"], f"{name}: log acceptance probability", rtol=1e-7, atol=1e-7)
            assert np.array_equal(O.accepted(ev["u"], la), ev["accepted"]), f"{name}: accepted mask"
            theta, ll = ev["theta"].copy(), ev["ll"].copy()
            seen["pmmh"] += 1
        elif kind == "rejuvenated":
            theta, ll = ev["theta"].copy(), ev["ll"].copy()
    assert seen["rejuvenate"] >= 2 and seen["pmmh"] >= 2, seen


@pytest.mark.parametrize("name", logs("inference_pmmh_"))
def test_oracle_reproduces_the_recorded_pmmh_moves(name):
    """run_pmmh with the random-walk proposal (random_walk.py:31-36: independent normals about every particle, exchanged on
    acceptance): theta*, the reverse kernel, log_acc and the accepted mask."""
    evs = events(name)
    theta, ll, ll_star, moves = evs[0][1]["theta"].copy(), None, None, 0
    normal = lambda x, loc, scale: O.prior(O.NORMAL, loc, scale, x)[1].sum(axis=1)  # noqa: E731
    for kind, ev in evs[1:]:
        if kind == "run":
            ll_star = ev["ll"]
            ll = ll_star if ll is None else ll
        elif kind == "pmmh_draw":
            loc, scale = ev["kernel_loc"], ev["kernel_scale"]
            close(loc + scale * ev["eps"], ev["rvs"], f"{name}: theta*")
            u_star = ev["rvs"]
        elif kind == "pmmh_accept":
            close(u_star, ev["new_kernel_loc"], f"{name}: reverse kernel mean")
            u_cur = unconstrain(theta)
            la = (normal(u_cur, ev["new_kernel_loc"], ev["new_kernel_scale"]) - normal(u_star, loc, scale)) + (
                ou_prior(u_star) - ou_prior(u_cur)) + (ll_star - ll)
            close(la, ev["log_acc"], f"{name}: log acceptance probability", rtol=1e-7, atol=1e-7)
            acc = O.accepted(ev["u"], la)
            assert np.array_equal(acc, ev["accepted"]), f"{name}: accepted mask"
            close(np.where(acc[:, None], u_star, loc), ev["kernel_loc_after"], f"{name}: the exchanged kernel")
            theta, ll = ev["theta"].copy(), ev["ll"].copy()
            moves += 1
    assert moves >= 5


@pytest.mark.parametrize("name", sorted(NESS_CASES))
def test_oracle_reproduces_the_recorded_ness_updates(name):
    """online.py:29-46 around jittering.py: ancestors, the fit (scale, clamped std), the locations, the jittered values in both
    spaces, for every recorded update."""
    case = NESS_CASES[name]
    kind = TC.JITTER_KIND[case["kernel"]]
    par = {O.LIUWEST: TC.LIUWEST_A, O.CONSTANT: CONSTANT_SCALE}.get(kind, 0.0)
    n = 0
    for what, ev in events(name):
        if what != "jitter":
            continue
        with np.errstate(divide="ignore"):
            lw = np.log(ev["W"])
        idx, _, _ = O.systematic(lw, float(ev["u"]))
        assert np.array_equal(idx, ev["indices"]), f"{name} update {n}: theta ancestors"
        fitted = O.jitter_fit(kind, ev["stacked"], lw, par)
        p = ev["stacked"].shape[1]
        close(fitted[1], np.broadcast_to(ev["scale"], (p,)), f"{name} update {n}: scale")
        close(fitted[2], np.broadcast_to(ev["std"], (p,)), f"{name} update {n}: std")
        sel = ev["bernoulli"] if case["discrete"] else None
        assert ("bernoulli" in ev) == case["discrete"]
        loc, _ = O.jitter_apply(kind, ev["stacked"], idx, fitted, np.zeros_like(ev["eps"]), None, par)
        close(loc, ev["mean"], f"{name} update {n}: locations")
        u, _ = O.jitter_apply(kind, ev["stacked"], idx, fitted, ev["eps"], sel, par)
        close(u, ev["jittered"], f"{name} update {n}: jittered (unconstrained)")
        close(O.log_prior(OU_KINDS, OU_A, OU_B, u)[1], ev["theta"], f"{name} update {n}: jittered (constrained)")
        n += 1
    assert n >= 3


# ---- the densities against two independent statements ---------------------------------------------------------------------------
GRID = np.linspace(-30.0, 30.0, 241)
FAMILIES = tuple(dict.fromkeys(TC.PRIORS + TC.NESS_PRIORS))


def _scipy_logpdf(kind, a, b, x):
    from scipy import stats

    dist = {O.NORMAL: lambda: stats.norm(a, b), O.LOGNORMAL: lambda: stats.lognorm(s=b, scale=math.exp(a)),
            O.EXPONENTIAL: lambda: stats.expon(scale=1.0 / a), O.GAMMA: lambda: stats.gamma(a, scale=1.0 / b),
            O.HALFNORMAL: lambda: stats.halfnorm(scale=a), O.BETA: lambda: stats.beta(a, b), O.UNIFORM: lambda: stats.uniform(a, b - a)}[kind]()
    return dist.logpdf(x)


def _log_jacobian(kind, a, b, u):
    if kind == O.NORMAL:
        return np.zeros_like(u)
    if kind in (O.BETA, O.UNIFORM):  # d sigmoid / du = s (1 - s)
        return -np.logaddexp(0.0, -u) - np.logaddexp(0.0, u) + (math.log(b - a) if kind == O.UNIFORM else 0.0)
    return u


def _mp_density(kind, a, b, u, dtype="float64"):
    """The density of u at 50 digits: the textbook density of the family at x(u) times |dx / du|, with the reference's clamp of the
    sigmoid.  Returns (x, log density) as mpmath numbers."""
    import mpmath as mp

    mp.mp.dps = 50
    u, a, b = mp.mpf(float(u)), mp.mpf(a), mp.mpf(b)
    fi = np.finfo(O.np_dtype(dtype))
    if kind == O.NORMAL:
        return u, mp.log(mp.npdf(u, a, b))
    if kind in (O.BETA, O.UNIFORM):
        s = 1 / (1 + mp.exp(-u))
        s = min(max(s, mp.mpf(float(fi.tiny))), 1 - mp.mpf(float(fi.eps)))
        lj = -mp.log(1 + mp.exp(-u)) - mp.log(1 + mp.exp(u))
        if kind == O.BETA:
            return s, (a - 1) * mp.log(s) + (b - 1) * mp.log(1 - s) - mp.log(mp.beta(a, b)) + lj
        return a + (b - a) * s, -mp.log(b - a) + lj + mp.log(b - a)
    x = mp.exp(u)
    if kind == O.LOGNORMAL:
        return x, -((u - a) ** 2) / (2 * b * b) - mp.log(b) - mp.log(2 * mp.pi) / 2 - u + u
    if kind == O.EXPONENTIAL:
        return x, mp.log(a) - a * x + u
    if kind == O.GAMMA:
        return x, a * mp.log(b) + (a - 1) * u - b * x - mp.loggamma(a) + u
    return x, mp.log(2) - x * x / (2 * a * a) - mp.log(a) - mp.log(2 * mp.pi) / 2 + u  # half normal


def density_bar(kind, a, b, u, lp, dtype="float64"):
    """The float64 bar of a log density at ``u`` - the theta bar (rtol 1e-11, atol 1e-12) plus, for Beta, eight times its
    conditioning floor: ``(b - 1) log(1 - x)`` is evaluated from x = sigmoid(u) ROUNDED to float64, one ulp of 1.0 in x is a
    relative 2^-52 / (1 - x) in 1 - x (1e-3 at u = 30), on either side of the comparison - the kernel, the oracle and torch all
    share it, their exp() need not agree in the last bit.  ``test_densities_agree_with_mpmath`` shows the measured error under an
    eighth of this bar."""
    return THETA_ATOL + THETA_RTOL * np.abs(lp) + 8.0 * O.prior_floor(kind, a, b, u, dtype)


@pytest.mark.parametrize("kind,a,b", FAMILIES)
def test_densities_agree_with_scipy(kind, a, b):
    x, lp = O.prior(kind, a, b, GRID)
    with np.errstate(divide="ignore"):
        want = _scipy_logpdf(kind, a, b, x) + _log_jacobian(kind, a, b, GRID)
    assert np.isfinite(lp).all()
    assert (np.abs(lp - want) <= density_bar(kind, a, b, GRID, want)).all(), (kind, float(np.abs(lp - want).max()))


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("kind,a,b", FAMILIES)
def test_densities_agree_with_mpmath(kind, a, b, dtype):
    """The measured floor: the oracle's error against the 50-digit evaluation on the grid and on the tail values of the GPU test, as a
    share of the bar - at most an eighth.  (float32 tensors: the same formulas with the float32 clamp of the sigmoid.)"""
    us = np.concatenate([GRID, [u for u in TC.TAIL_U if abs(u) <= 90.0]])
    x, lp = O.prior(kind, a, b, us, dtype)
    worst = worst_x = 0.0
    for k, u in enumerate(us):
        mx, ml = _mp_density(kind, a, b, u, dtype)
        if not np.isfinite(lp[k]):  # exp(90) squared over 2 a^2 and the like: -inf on both sides
            assert float(ml) < -1e300 or not np.isfinite(float(ml)), (kind, u, lp[k], ml)
            continue
        err = abs(float(lp[k] - ml))
        worst = max(worst, err / float(density_bar(kind, a, b, u, float(ml), dtype)))
        scale = max(abs(a), abs(b)) if kind == O.UNIFORM else max(abs(float(mx)), 1e-300)  # (an interval's x: errors of its end points)
        worst_x = max(worst_x, abs(float(x[k] - mx)) / scale)
    report(f"floor density kind={kind} a={a} b={b} {dtype}: oracle vs mpmath, worst error / bar = {worst:.3g} (<= 0.125), "
           f"x relative {worst_x:.3g}")
    assert worst <= 0.125, (kind, a, b, worst)
    assert worst_x <= 1e-15, worst_x


def test_float32_clamp_keeps_beta_and_uniform_inside_their_support():
    """The reference's float32 ``SigmoidTransform`` clamps at ``finfo(float32).tiny`` and ``1 - finfo(float32).eps``: x rounded to
    float32 stays inside (0, 1) / [low, high) - torch's ``Uniform`` counts ``low`` itself as inside, and ``low + (high - low) tiny``
    IS ``low`` in float32 arithmetic - at every tail value, with a finite density; the float64 clamp does NOT (the float32 rounding of
    ``1 - 2^-52`` is 1.0, of ``2^-1022`` is 0) - which is why the clamp is per dtype."""
    us = np.array(TC.TAIL_U)
    for kind, a, b in ((O.BETA, 2.0, 5.0), (O.UNIFORM, -0.4, 1.3), (O.BETA, 2.0, 3.0), (O.UNIFORM, -1.0, 2.0)):
        lo, hi = (0.0, 1.0) if kind == O.BETA else (a, b)
        x32 = O.prior(kind, a, b, us, "float32")[0].astype(np.float32)
        assert ((x32 > np.float32(lo)) if kind == O.BETA else (x32 >= np.float32(lo))).all() and (x32 < np.float32(hi)).all(), (kind, x32)
        bad = O.prior(kind, a, b, us, "float64")[0].astype(np.float32)
        assert (bad == np.float32(hi)).any() and (kind == O.UNIFORM or (bad == 0).any()), (kind, bad)
        assert np.isfinite(O.prior(kind, a, b, us, "float32")[1]).all()


# ---- the product's torch route (CPU, float64) ----------------------------------------------------------------------------------
def _torch_priors(triples):
    import torch
    from torch.distributions import Beta, Exponential, Gamma, HalfNormal, LogNormal, Normal, Uniform

    make = {O.NORMAL: lambda a, b: Normal(a, b), O.LOGNORMAL: lambda a, b: LogNormal(a, b), O.EXPONENTIAL: lambda a, b: Exponential(a),
            O.GAMMA: lambda a, b: Gamma(a, b), O.HALFNORMAL: lambda a, b: HalfNormal(a), O.BETA: lambda a, b: Beta(a, b),
            O.UNIFORM: lambda a, b: Uniform(a, b)}
    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731  (a Python float would become a float32 parameter)
    return {f"p{k}": make[kind](t(a), t(b)) for k, (kind, a, b) in enumerate(triples)}


@pytest.mark.parametrize("triples", [TC.PRIORS, TC.NESS_PRIORS], ids=["PRIORS", "NESS_PRIORS"])
def test_product_priors_agree_with_the_oracle(triples):
    import torch

    from pyfilter_amd.inference import ThetaParticles

    us = np.concatenate([GRID, [u for u in TC.TAIL_U if abs(u) <= 90.0]])
    theta = ThetaParticles(_torch_priors(triples), len(us), "cpu", torch.float64).initialize_parameters(torch.Generator().manual_seed(1))
    ut = torch.from_numpy(us)
    for (kind, a, b), prior in zip(triples, theta.priors.values()):
        x, lp = O.prior(kind, a, b, us)
        got_x, got_lp = prior.get_constrained(ut).numpy(), prior.unconstrained.log_prob(ut).numpy()
        close(got_x, x, f"kind {kind}: constrained value", rtol=THETA_RTOL, atol=0.0)
        both = np.isfinite(lp) | np.isfinite(got_lp)
        bar = density_bar(kind, a, b, us, lp)
        if kind in (O.BETA, O.UNIFORM):
            # torch's softplus returns its argument beyond its threshold of 20 (an error of log1p(exp(-20)) = 2.06e-9 at most) in the
            # sigmoid's log-Jacobian; the oracle, like scipy, mpmath and the kernels, evaluates it exactly
            bar = bar + np.where(np.abs(us) > 20.0, math.log1p(math.exp(-20.0)), 0.0)
        assert (np.abs(got_lp - lp)[both] <= bar[both]).all(), (kind, np.abs(got_lp - lp)[both].max())
        assert np.array_equal(got_lp[~both], lp[~both], equal_nan=True), kind


@pytest.mark.parametrize("pattern", TC.WEIGHTS)
@pytest.mark.parametrize("b,p", [(1, 1), (2, 3), (65, 8), (257, 5), (1000, 3)])
def test_product_fit_and_resampling_agree_with_the_oracle(b, p, pattern):
    import torch

    from pyfilter_amd.inference.utils import construct_mvn, theta_normalize, theta_systematic

    lw = TC.logw(pattern, b, "float64")
    w = theta_normalize(torch.from_numpy(lw))
    close(w.numpy(), O.normalize(lw), "normalised weights", rtol=1e-13, atol=0.0)
    for kind in ("correlated", "zero_column"):
        x = TC.values(kind, b, p, "float64")
        mean, chol, info = O.fit(x, lw, 1.1)
        if info["fallback"] and not (kind == "zero_column" or b == 1 or pattern in ("first", "last")):
            continue  # (a cloud of fewer weighted points than parameters: positive definite or not by rounding, in the reference too)
        want = construct_mvn(torch.from_numpy(x), w, 1.1)
        close(want.loc.numpy(), mean, "mean", rtol=THETA_RTOL, atol=THETA_ATOL)
        close(want.scale_tril.numpy(), chol, "factor", rtol=1e-9, atol=1e-11)
    for u in TC.RESAMPLE_U:
        got = theta_systematic(w, torch.tensor(u, dtype=torch.float64)).numpy()
        idx, cdf, pos = O.systematic(lw, u)
        assert PR.valid_ancestor(got, pos, cdf, TC.delta64(b)).all() and (np.diff(got) >= 0).all()
        if pattern != "nothing":
            assert (got != idx).sum() <= TC.near_cap(b)


# ---- the jitter kernels' addresses ----------------------------------------------------------------------------------------------
def test_jitter_stream_word_is_the_one_of_the_sources():
    assert streams_in_sources()["JITTER"] == PR.STREAMS["JITTER"] == O.JITTER_STREAM == int.from_bytes(b"JITT", "big")


def test_jitter_addresses_are_injective_and_apart_from_the_filter_streams():
    """The word tuple (particle, parameter, counter low, stream ^ counter high) over i < 8192, q <= 8 (q = P: the Bernoulli call) and
    the update counters 0, 1, 2, 2^32 + 5: no two draws share a call.  While the counter is below 2^32 the fourth word is the jitter
    stream word itself, which no filter stream uses (theirs are small integers, one with 0x200 ORed in), so no jitter call is a filter
    call under the same seed; beyond 2^32 the xor with the counter's high word could in principle produce another stream's word
    (after 0x4A495454 ^ s updates of 2^32 each - not a count any run reaches)."""
    i, q = np.meshgrid(np.arange(8192, dtype=np.uint64), np.arange(9, dtype=np.uint64), indexing="ij")
    rows = []
    for counter in (0, 1, 2, 2 ** 32 + 5):
        words = O.jitter_address(i.ravel(), q.ravel(), counter, 8)
        rows.append(np.stack([np.broadcast_to(np.asarray(w, dtype=np.uint64), i.size) for w in words], axis=1))
    rows = np.concatenate(rows)
    assert (rows < 2 ** 32).all()
    assert len(np.unique(rows, axis=0)) == len(rows) == 4 * 9 * 8192
    others = {name: word for name, word in PR.STREAMS.items() if name != "JITTER"}  # (test_philox_cpu.py: all the sources define)
    theirs = set(others.values()) | {others["MULTINOMIAL"] | PR.EXP_FLAG}
    assert len(others) == len(PR.STREAMS) - 1 == 10 and max(theirs) < 2 ** 16 and O.JITTER_STREAM not in theirs
    low = rows[rows[:, 3] == O.JITTER_STREAM]
    assert len(low) == 3 * 9 * 8192  # (every counter below 2^32 carries the bare stream word)
    # the draws themselves: unit-variance normals, uniforms below `prob` at the rate `prob`, two updates apart
    eps, sel, unif = O.jitter_draws(3, 0, 4096, 8, 1 / 64)
    assert abs(eps.mean()) < 0.02 and abs(eps.std() - 1.0) < 0.02 and abs(sel.mean() - 1 / 64) < 0.01 and (unif < 1).all()
    assert not np.array_equal(eps, O.jitter_draws(3, 1, 4096, 8, 1 / 64)[0])
    for name in O.MUTATIONS:  # every mutation is another set of draws at a counter above 2^32
        e2, s2, u2 = O.mutated_draws(name, 3, 2 ** 32 + 5, 4096, 8, 1 / 64)
        e1, s1, u1 = O.jitter_draws(3, 2 ** 32 + 5, 4096, 8, 1 / 64)
        assert not (np.array_equal(e1, e2) and np.array_equal(u1, u2)), name


# ---- input conditions of the GPU comparisons -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES)
def test_few_resampling_positions_lie_within_delta_of_a_cdf_entry(dtype):
    """For every (B, weight pattern, u) of the resampling comparison: at most max(2, 1 % of B) positions within delta of a float64
    cdf entry (delta_32 = 4 * 2^-24, delta_64 = 8 B 2^-53).  Equal weights ("nothing finite") put EVERY position on or next to an
    entry for u = 0, 2^-53, 0.999999 and 1: that pattern is exact by construction - cdf (j + 1) / B and positions (i + u) / B, each
    one correctly rounded division - and the GPU test asserts it exactly, not through delta."""
    worst, total, cases = 0.0, 0, 0
    for b in TC.B_ALL:
        delta = TC.DELTA32 if dtype == "float32" else TC.delta64(b)
        for pattern in TC.WEIGHTS:
            if pattern == "nothing":
                continue
            lw = TC.logw(pattern, b, dtype)
            for u in TC.RESAMPLE_U:
                _, cdf, pos = O.systematic(lw, u, dtype)
                near = int(PR.near_boundary(pos, cdf, delta).sum())
                assert near <= TC.near_cap(b), (b, pattern, u, near)
                worst, total, cases = max(worst, near / b if b >= 200 else 0.0), total + near, cases + 1
    report(f"delta rule {dtype}: {cases} resampling cases, {total} positions within delta of a cdf entry in all, largest share at "
           f"B >= 200: {100 * worst:.2f} %")


def test_equal_weights_resample_exactly():
    """Equal weights: ancestor i - 1 for u = 0 (position i / B sits ON cdf[i - 1]; left-side search), i for 0 < u < 1 in float64."""
    for b in TC.B_ALL:
        lw = TC.logw("nothing", b, "float64")
        assert np.array_equal(O.systematic(lw, 0.0)[0], np.maximum(np.arange(b) - 1, 0))
        assert np.array_equal(O.systematic(lw, 0.3718)[0], np.arange(b))
        assert np.array_equal(O.systematic(lw, 0.0, "float32")[0], np.maximum(np.arange(b) - 1, 0))


def test_few_jitter_cases_have_an_ill_conditioned_quartile_pick():
    """The skip rule of ``tests/test_ness_gpu.py`` (``_quartile_gap >= 1e-9``) on the small sizes of the new sweep: at most 1 % of its
    cases fall under it.  (B = 1, 2: no second value whose weight moves the cdf past the pick - nothing to be ill-conditioned.)"""
    skipped = ran = 0
    for dtype in TC.DTYPES:
        for b in TC.JITTER_B:
            for p in TC.P_EVERY_B:
                for family in TC.JITTER_FAMILIES[:3]:
                    for discrete in (False, True):
                        c = TC.jitter_case(b, p, family, discrete, dtype)
                        ran += 1
                        skipped += TC.quartile_gap(c["x"], O.normalize(c["lw"])) < 1e-9
    report(f"quartile rule: {skipped} of {ran} small-B jitter cases ill-conditioned (cap 1 %)")
    assert skipped <= 0.01 * ran, (skipped, ran)


def test_no_select_uniform_sits_on_the_bernoulli_threshold():
    for b in TC.OWN_B:
        for p in TC.OWN_P:
            for seed in TC.OWN_SEEDS:
                for counter in TC.OWN_COUNTERS:
                    unif = O.jitter_draws(seed, counter, b, p, b ** -0.5)[2]
                    assert (np.abs(unif - b ** -0.5) > 1e-12).all(), (b, p, seed, counter)


@pytest.mark.parametrize("col", [0, 2])
def test_product_fit_with_a_nan_value_column(col):
    """What the torch route returns when one value is NaN (recorded here, required of ``pf_theta_fit`` by the GPU test): a NaN mean
    entry; ``cholesky_ex`` reports failure, so the diagonal fallback - NaN in that entry, the other columns' standard deviations next
    to it, zeros off the diagonal.  The oracle says the same."""
    import torch

    from pyfilter_amd.inference.utils import construct_mvn

    x = TC.values("correlated", 257, 3, "float64")
    x[7, col] = math.nan
    got = construct_mvn(torch.from_numpy(x), torch.full((257,), 1.0 / 257, dtype=torch.float64), 1.1)
    mean, chol, info = O.fit(x, None, 1.1)
    assert info["fallback"] and np.isnan(mean[col]) and np.isnan(chol[col, col]) and np.isnan(chol).sum() == 1 and np.isnan(mean).sum() == 1
    close(got.loc.numpy(), mean, "mean", rtol=THETA_RTOL, atol=THETA_ATOL)
    close(got.scale_tril.numpy(), chol, "factor", rtol=THETA_RTOL, atol=THETA_ATOL)
    assert np.array_equal(got.scale_tril.numpy() == 0.0, chol == 0.0)


def test_fit_floor():
    """The measured floor under the fit bars of the GPU test: the float64 oracle against its own evaluation in extended precision
    (``np.longdouble``) over the whole case list, in units of 2^-53 times the first-order error shape - at most ``theta_cases.FIT_K``.
    The GPU test's bars are the theta bar plus 8 x FIT_K x 2^-53 x shape: nothing next to rtol 1e-11 for a well-conditioned factor,
    the whole entry where a pivot is almost rounding (the ill-scaled cloud of the spread pattern)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this machine")
    worst = dict(mean=0.0, factor=0.0, diagonal=0.0)
    for dtype, (b, p) in ((d, bp) for d in TC.DTYPES for bp in TC.BP):  # (float32: the same arithmetic on inputs rounded to float32)
        for pattern in TC.WEIGHTS + ("null",):
            lw = None if pattern == "null" else TC.logw(pattern, b, dtype)
            for kind in ("correlated", "zero_column"):
                x = TC.values(kind, b, p, dtype)
                m, _, info = O.fit(x, lw, 1.1)
                hm, _, hp = O.fit(x, lw, 1.1, real=np.longdouble)
                unit = 2.0 ** -53
                worst["mean"] = max(worst["mean"], float(np.max(np.abs(m - hm.astype(np.float64)) / np.maximum(unit * info["abs_mean"], 1e-300))))
                if hp["first_bad"] is None and not (np.diag(info["cov"]) == 0.0).any():
                    shape = O.cholesky_error_shape(info["abs_cov"], info["cholesky"] / 1.1) * 1.1
                    err = np.abs(info["cholesky"] - hp["cholesky"].astype(np.float64))
                    worst["factor"] = max(worst["factor"], float(np.max(err / np.maximum(unit * shape, 1e-300))))
                shape = 1.1 * np.sqrt(np.diag(info["abs_cov"]))
                err = np.abs(np.diag(info["diagonal"]) - np.diag(hp["diagonal"]).astype(np.float64))
                worst["diagonal"] = max(worst["diagonal"], float(np.max(err / np.maximum(unit * shape, 1e-300))))
    report(f"floor fit: float64 oracle vs extended precision, in 2^-53 x shape: {worst} (FIT_K = {TC.FIT_K})")
    assert max(worst.values()) <= TC.FIT_K, worst
