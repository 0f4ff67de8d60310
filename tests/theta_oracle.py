"""Host oracle of the theta-level arithmetic (TEST INFRASTRUCTURE; numpy float64, no torch.distributions, nothing imported from
the product).

A restatement of what the reference does to the B theta-particles of an SMC^2 / PMMH / NESS run, written from the reference's
sources (file:line of ``pyfilter/``) and from the formulas of the distributions it composes - NOT from ``csrc/pf_theta.hpp`` or
``csrc/pf_jitter.hpp``, which are what it judges:

* ``normalize`` / ``ess``                  utils.py:49-64, :8-20
* ``fit``                                  inference/utils.py:42-76 (``calc_mean_chol`` / ``construct_mvn``)
* ``prior``                                inference/prior.py:47-62, :111-123 (``TransformedDistribution(prior, biject_to(support).inv)``)
* ``propose`` / ``log_accept``             inference/batch/mcmc/utils.py:48-50, :57-70
* ``systematic``                           resampling.py:24-52 behind sequential/kernels/mh.py:52-56 and online.py:30
* ``path``                                 inference/sequential/state.py:35-44 (``w += ll``, then ``get_ess``)
* ``robust_var`` and the jitter families   inference/sequential/kernels/jittering.py:49-83, :140-225, ``_jitter`` :11-22,
                                           the discrete mix of online.py:37-44
* ``jitter_draws``                         the kernel route's own Philox draws, on ``tests/philox_ref.py``; the address is an argument

``dtype`` ("float32" / "float64") selects the constants the reference evaluates per tensor type (``finfo(dtype).tiny`` and
``1 - finfo(dtype).eps`` of the sigmoid's clamp, ``EPS = sqrt(finfo.eps)`` of constants.py:7) and where a value is rounded to the
tensors' type; every formula is evaluated in float64."""
import math

import numpy as np

from tests import philox_ref as PR

NORMAL, LOGNORMAL, EXPONENTIAL, GAMMA, HALFNORMAL, BETA, UNIFORM = range(7)  # include/pf_amd.h: PF_PRIOR_*
NONSHRINKING, SHRINKING, LIUWEST, CONSTANT = range(4)                        # include/pf_amd.h: PF_JITTER_*
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
JITTER_STREAM = 0x4A495454  # "JITT" (tests/test_theta_oracle_cpu.py checks it against the sources)

def np_dtype(dtype):
    return np.float32 if PR._is32(dtype) else np.float64


def rounded(v, dtype):
    """``v`` rounded once to the tensors' type, as float64."""
    with np.errstate(over="ignore"):  # (beyond the type's range: the infinity the conversion gives)
        return np.asarray(v, dtype=np.float64).astype(np_dtype(dtype)).astype(np.float64)


def eps_of(dtype):
    """constants.py:7 ``EPS = sqrt(finfo(default dtype).eps)``."""
    return math.sqrt(float(np.finfo(np_dtype(dtype)).eps))


# ---- weights -----------------------------------------------------------------------------------------------------------------
def normalize(logw, real=np.float64):
    """utils.py:57-62: NaN and +inf become -inf (they carry no weight), softmax of (w - max); nothing finite -> 1 / B each (what
    the ``masked_fill_`` of line 62 is there for).  (The reference's ``nan_to_num_`` turns a -inf ENTRY into the lowest finite
    number, so among weights none of which is finite it gives the -inf ones equal shares and the NaN / +inf ones nothing; the
    kernels give every particle 1 / B there - INTEGRATION section 4b.  The cases of the tests have only -inf in that pattern.)
    ``real``: the type the arithmetic runs in (``np.longdouble``: the oracle's own error is measured against it)."""
    w = np.array(logw, dtype=real)
    w[np.isnan(w) | (w == np.inf)] = -np.inf
    m = w.max()
    if not m > -np.inf:
        return np.full(w.shape, real(1.0) / real(w.shape[0]), dtype=real)
    e = np.exp(w - m)
    return e / e.sum()


def ess(logw):
    """utils.py:17-20."""
    p = normalize(logw)
    return 1.0 / np.sum(p * p)


# ---- the Gaussian fit ----------------------------------------------------------------------------------------------------------
PIVOT_FLOOR = 2.0 ** -40  # a pivot below this share of its diagonal entry is rounding: B <= 4097 terms of 2^-53 each reach 2^-41


def cholesky(c):
    """Lower Cholesky factor (column by column), whether ``c`` was positive definite (``cholesky_ex``'s ``info == 0``; the columns left
    of the failing pivot are complete) and the first column whose pivot is not above ``PIVOT_FLOOR`` of its diagonal entry (None: the
    factor is well determined)."""
    p = c.shape[0]
    l = np.zeros_like(c)
    first_bad = None
    for j in range(p):
        d = c[j, j] - np.dot(l[j, :j], l[j, :j])
        if first_bad is None and not d > PIVOT_FLOOR * c[j, j]:
            first_bad = j
        if not d > 0.0:
            return l, False, first_bad
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, p):
            l[i, j] = (c[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return l, True, first_bad


def cholesky_error_shape(abs_cov, l):
    """First-order forward error of the column-by-column Cholesky factor ``l`` per unit roundoff: ``v[i, j] = c[i, j] - sum_k l[i, k]
    l[j, k]`` carries one unit of ``M[i, j] = sum |terms of c[i, j]| + sum_k |l[i, k] l[j, k]|`` plus what the columns to the left
    hand down; ``l[j, j] = sqrt(v[j, j])`` halves the relative error, ``l[i, j] = v[i, j] / l[j, j]`` adds that of the pivot.  A small
    pivot shows as a large entry here: the conditioning of an ill-scaled cloud.  (The measured error of the float64 oracle against
    extended precision is a multiple K of ``2^-53`` times this shape - tests/test_theta_oracle_cpu.py measures K.)"""
    l = np.abs(np.asarray(l, dtype=np.float64))
    p = l.shape[0]
    e = np.zeros((p, p))
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(p):
            for i in range(j, p):
                dv = abs_cov[i, j] + l[i, :j] @ l[j, :j] + e[i, :j] @ l[j, :j] + l[i, :j] @ e[j, :j]
                if i == j:
                    e[j, j] = dv / (2.0 * l[j, j])
                else:
                    e[i, j] = dv / l[j, j] + l[i, j] * e[j, j] / l[j, j]
    return e


def fit(values, logw, scale=1.0, real=np.float64):
    """inference/utils.py:47-56, :70-71: ``mean = w @ x``, ``cov = (w * c.T) @ c`` about it, its lower Cholesky factor - or
    ``cov.diag().sqrt().diag()`` (a negative entry counting as 0, the product's reading) where it is not positive definite -, times
    ``scale``.  ``logw = None``: equal weights.  Returns (mean, factor, info): ``abs_mean`` / ``abs_cov`` the sums of absolute terms
    the float32 bars are made of, ``fallback``, ``cov``, ``first_bad`` (``cholesky``), and both candidates - ``cholesky`` (complete
    left of a failing pivot) and ``diagonal`` - for a case whose choice between them is rounding."""
    x = np.asarray(values, dtype=real)
    b = x.shape[0]
    w = np.full(b, real(1.0) / real(b), dtype=real) if logw is None else normalize(logw, real)
    mean = w @ x
    c = x - mean
    cov = (w * c.T) @ c
    tri, ok, first_bad = cholesky(cov)
    d = np.diag(cov)
    with np.errstate(invalid="ignore"):
        diag = np.diag(np.sqrt(np.where(d < 0.0, 0.0, d)))
    return mean, real(scale) * (tri if ok else diag), dict(
        abs_mean=w @ np.abs(x), abs_cov=(w * np.abs(c).T) @ np.abs(c), fallback=not ok, cov=cov, first_bad=first_bad,
        cholesky=real(scale) * tri, diagonal=real(scale) * diag)


# ---- the priors in unconstrained space ---------------------------------------------------------------------------------------
def _softplus(v):
    return np.where(v > 0, v + np.log1p(np.exp(-np.abs(v))), np.log1p(np.exp(-np.abs(v))))


def _xlogy(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(y))


def sigmoid_clamped(u, dtype):
    """torch's ``SigmoidTransform._call``: ``clamp(sigmoid(u), min=finfo.tiny, max=1 - finfo.eps)`` with the tensors' finfo."""
    fi = np.finfo(np_dtype(dtype))
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-u))
    return np.clip(s, float(fi.tiny), 1.0 - float(fi.eps))


def prior(kind, a, b, u, dtype="float64"):
    """(constrained x, log density of u) of one prior family: prior.py:62 ``TransformedDistribution(prior, biject_to(support).inv)``
    at ``u`` is ``prior.log_prob(x) + log |dx / du|`` with ``x = biject_to(support)(u)`` - the identity on the reals, ``exp`` on the
    positive half line (log |dx/du| = u), the clamped sigmoid on the unit interval (log |dx/du| = -softplus(-u) - softplus(u)) and
    ``low + (high - low) sigmoid`` on an interval (+ log |high - low|).  The densities by their textbook formulas; parameters:
    Normal(loc a, scale b), LogNormal(a, b), Exponential(rate a), Gamma(concentration a, rate b), HalfNormal(scale a),
    Beta(a, b), Uniform(low a, high b)."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if kind == NORMAL:
            x = u
            z = (x - a) / b
            return x, -0.5 * z * z - np.log(b) - HALF_LOG_2PI
        if kind in (LOGNORMAL, EXPONENTIAL, GAMMA, HALFNORMAL):
            x = np.exp(u)
            if kind == LOGNORMAL:  # Normal density of log x, over x
                lx = np.log(x)
                z = (lx - a) / b
                return x, (-0.5 * z * z - math.log(b) - HALF_LOG_2PI) - lx + u
            if kind == EXPONENTIAL:
                return x, math.log(a) - a * x + u
            if kind == GAMMA:
                return x, a * math.log(b) + _xlogy(a - 1.0, x) - b * x - math.lgamma(a) + u
            z = x / a  # half normal: twice the Normal(0, a) density on x >= 0
            return x, (-0.5 * z * z - math.log(a) - HALF_LOG_2PI) + math.log(2.0) + u
        s = sigmoid_clamped(u, dtype)
        ladj = -_softplus(-u) - _softplus(u)
        if kind == BETA:
            lbeta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
            return s, _xlogy(a - 1.0, s) + _xlogy(b - 1.0, 1.0 - s) - lbeta + ladj
        assert kind == UNIFORM, kind
        x = a + (b - a) * s
        inside = (x >= a) & (x < b)  # torch's Uniform.log_prob: log(lb * ub) - log(high - low)
        return x, np.where(inside, 0.0, -np.inf) - math.log(b - a) + ladj + math.log(abs(b - a))


def prior_floor(kind, a, b, u, dtype="float64"):
    """What one ulp of 1.0 in the ROUNDED x = sigmoid(u) does to ``(b - 1) log(1 - x)`` of the Beta density: a relative
    ``2^-52 / (1 - x)`` in ``1 - x`` (1e-3 at u = 30 in float64; never above 2^-29 with the float32 clamp).  The kernel, the oracle
    and torch all evaluate that term from the rounded x and their ``exp`` need not agree in the last bit: the conditioning floor of
    the Beta family, 0 for the others (tests/test_theta_oracle_cpu.py measures the oracle against 50 digits under it)."""
    u = np.asarray(u, dtype=np.float64)
    if kind != BETA:
        return np.zeros(u.shape)
    s = sigmoid_clamped(u, dtype)
    return abs(b - 1.0) * 2.0 ** -52 * s / (1.0 - s)


def log_prior(kinds, a, b, u, dtype="float64"):
    """Summed log density of the rows of ``u (B, P)`` (left to right, as ``eval_priors`` sums), the constrained values ``(B, P)``
    the sum of the absolute terms and the summed conditioning floor."""
    u = np.asarray(u, dtype=np.float64)
    xs, total, mag, floor = [], np.zeros(u.shape[0]), np.zeros(u.shape[0]), np.zeros(u.shape[0])
    for p, k in enumerate(kinds):
        x, lp = prior(k, a[p], b[p], u[:, p], dtype)
        xs.append(x)
        with np.errstate(invalid="ignore"):
            total = total + lp
            mag = mag + np.abs(lp)
        floor = floor + prior_floor(k, a[p], b[p], u[:, p], dtype)
    return total, np.stack(xs, axis=1), mag, floor


def propose(mean, chol, eps, dtype="float64"):
    """mcmc/utils.py:48 through ``MultivariateNormal.rsample``: ``u = mean + L eps``; the stored value - what the prior is evaluated
    at and every later step starts from - is ``u`` rounded to the tensors' type.  Also ``|mean| + |L| |eps|``."""
    mean, chol, eps = (np.asarray(v, dtype=np.float64) for v in (mean, chol, eps))
    l = np.tril(chol)
    with np.errstate(over="ignore", invalid="ignore"):
        u = mean + eps @ l.T
        mag = np.abs(mean) + np.abs(eps) @ np.abs(l).T
    return rounded(u, dtype), mag


def mvn_logpdf(x, mean, chol):
    """log N(x; mean, L L^T) by forward substitution; also the sum of the absolute terms."""
    x, mean, l = np.asarray(x, dtype=np.float64), np.asarray(mean, dtype=np.float64), np.tril(np.asarray(chol, dtype=np.float64))
    p = l.shape[0]
    z = np.zeros_like(x)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(p):
            z[:, i] = (x[:, i] - mean[i] - z[:, :i] @ l[i, :i]) / l[i, i]
        half_log_det = np.sum(np.log(np.diag(l)))
        quad = 0.5 * np.sum(z * z, axis=1)
    cst = 0.5 * p * math.log(2.0 * math.pi)
    return -quad - half_log_det - cst, quad + abs(half_log_det) + cst


def log_accept(u_cur, u_star, fwd, rev, prior_cur, prior_star, ll_cur, ll_star):
    """mcmc/utils.py:57-66: ``[log q_r(u) - log q_f(u*)] + [prior* - prior] + [ll* - ll]``; (value, sum of absolute terms)."""
    qr, mr = mvn_logpdf(u_cur, *rev)
    qf, mf = mvn_logpdf(u_star, *fwd)
    t = [np.asarray(v, dtype=np.float64) for v in (prior_star, prior_cur, ll_star, ll_cur)]
    with np.errstate(invalid="ignore"):
        la = (qr - qf) + (t[0] - t[1]) + (t[2] - t[3])
        mag = mr + mf + sum(np.abs(v) for v in t)
    return la, mag


def accepted(unif, log_acc):
    """mcmc/utils.py:67: ``uniform.log() < log_acc`` (NaN: rejected)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(unif, dtype=np.float64)) < np.asarray(log_acc, dtype=np.float64)


# ---- resampling ----------------------------------------------------------------------------------------------------------------
def systematic(logw, u, dtype="float64"):
    """resampling.py:41-50 of the normalised weights: the running sum - accumulated in float64, rounded once to ``dtype``, last entry
    1 -, positions ``(i + u) / B`` in ``dtype`` arithmetic, left-side searchsorted, at most B - 1.
    Returns (ancestors, float64 cdf, float64 positions)."""
    w = normalize(logw)
    b = w.shape[0]
    cdf64 = PR.cdf64(w)
    if len(set(w.tolist())) == 1:  # equal weights: their running sum is (j + 1) / B, one division - not B roundings whose order decides ties
        cdf64 = np.arange(1, b + 1, dtype=np.float64) / b
    t = np_dtype(dtype)
    cdf = cdf64.astype(t)
    cdf[-1] = 1.0
    pos = (np.arange(b).astype(t) + t(u)) / t(b)
    idx = np.minimum(np.searchsorted(cdf, pos, side="left"), b - 1).astype(np.int64)
    return idx, cdf64, (np.arange(b, dtype=np.float64) + float(u)) / b


# ---- the running theta-weights ----------------------------------------------------------------------------------------------
def path(w0, ll, dtype="float64"):
    """state.py:42 applied n times, as ``w0 + ll.cumsum(0)`` does: the increments summed in order in ``dtype``, then added to w0."""
    t = np_dtype(dtype)
    w0, ll = np.asarray(w0, dtype=t), np.asarray(ll, dtype=t)
    out = np.empty_like(ll)
    with np.errstate(invalid="ignore", over="ignore"):
        c = ll[0].copy()
        out[0] = w0 + c
        for r in range(1, ll.shape[0]):
            c = (c + ll[r]).astype(t)
            out[r] = w0 + c
    return out


def path_stats(row):
    """(ESS, every weight finite) of one row of theta-weights."""
    row = np.asarray(row, dtype=np.float64)
    return ess(row), float(np.isfinite(row).all())


# ---- jittering -----------------------------------------------------------------------------------------------------------------
def robust_var(x, w, mean=None):
    """jittering.py:62-83 (the sort stable, as the reference's CPU sort is): per column, the weights accumulated in sorted order,
    the FIRST index that minimises |cdf - 0.25| / |cdf - 0.75|, ``iqr = (x_hi - x_lo) / 1.349``, ``var <- iqr^2`` where
    ``iqr^2 <= var``.  (A NaN variance - B = 1 has none of it: see the B = 1, 2 cases of the GPU test - fails ``<=`` and stays.)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    order = np.argsort(x, axis=0, kind="stable")
    srt = np.take_along_axis(x, order, axis=0)
    cw = np.cumsum(w[order], axis=0)
    lo, hi = np.argmin(np.abs(cw - 0.25), axis=0), np.argmin(np.abs(cw - 0.75), axis=0)
    cols = np.arange(x.shape[1])
    iqr = (srt[hi, cols] - srt[lo, cols]) / 1.349
    iqr2 = iqr ** 2
    if mean is None:
        mean = (w[:, None] * x).sum(0)
    var = (w[:, None] * (x - mean) ** 2).sum(0)
    return np.where(iqr2 <= var, iqr2, var)


def jitter_fit(kind, x, logw, par=0.0, scale=None, dtype="float64", min_std=None):
    """``JitterKernel.fit`` + the clamp of jittering.py:131-132: (weighted mean (P,), scale (P,), std (P,), ESS, bandwidth factor)."""
    x = np.asarray(x, dtype=np.float64)
    p = x.shape[1]
    e = eps_of(dtype)
    min_std = e if min_std is None else min_std
    if kind == CONSTANT:  # jittering.py:222-225
        sc = np.broadcast_to(np.asarray(par if scale is None else scale, dtype=np.float64), (p,)).copy()
        return np.zeros(p), sc, np.maximum(sc, min_std), 0.0, 0.0
    w = normalize(logw)
    n_eff = 1.0 / np.sum(w * w)
    bw = min(max(1.59 * n_eff ** (-1.0 / 3.0), e), 1.0 - e)  # jittering.py:150
    mean = (w[:, None] * x).sum(0)
    var = robust_var(x, w, mean)
    fac = math.sqrt(1.0 - par * par) if kind == LIUWEST else bw  # jittering.py:195, :203
    with np.errstate(invalid="ignore"):
        sc = fac * np.sqrt(var)
        std = np.where(sc < min_std, min_std, sc)  # (clamp leaves NaN alone)
    return mean, sc, std, n_eff, bw


def jitter_apply(kind, x, anc, fitted, eps, select=None, par=0.0):
    """jittering.py:156, :171, :201, :223 (the location per family), :22 (``location + std * eps``), online.py:44 (the discrete
    mix ``(1 - s) x[anc] + s jittered``): the jittered unconstrained values (B, P) and ``|location| + |std eps|``."""
    x, eps = np.asarray(x, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    mean, _, std, _, bw = fitted
    xa = x[np.asarray(anc)]
    if kind == SHRINKING:
        loc = mean + math.sqrt(1.0 - bw * bw) * (xa - mean)
    elif kind == LIUWEST:
        loc = xa * par + (1.0 - par) * mean
    else:
        loc = xa
    with np.errstate(invalid="ignore"):
        u = loc + std * eps
        mag = np.abs(loc) + np.abs(std * eps)
        if select is not None:
            s = np.asarray(select, dtype=np.float64)[:, None]
            u = (1.0 - s) * xa + s * u
    return u, mag


# ---- the kernel route's own draws ----------------------------------------------------------------------------------------------
def jitter_address(i, q, counter, P):
    """The four counter words of the call behind particle ``i``, "parameter" ``q`` (``q = P``: the Bernoulli draw of ``discrete``) of
    update ``counter`` (64 bits): (particle, parameter, counter low word, stream word ^ counter high word)."""
    return i, q, counter & 0xFFFFFFFF, JITTER_STREAM ^ (counter >> 32)


def jitter_draws(seed, counter, B, P, prob, address=jitter_address, select_q=None, second=False):
    """(eps (B, P), select (B,), the select uniforms): ``eps[i, p]`` the FIRST Box-Muller normal of call ``address(i, p, counter, P)``
    under key ``seed``, in double for both tensor types; ``select[i] = u01_d(x, y) < prob`` of call ``address(i, P, ...)``.
    ``address`` / ``select_q`` / ``second``: the mutations the tests must reject go in here."""
    seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    i = np.arange(B, dtype=np.uint64)[:, None]
    q = np.arange(P, dtype=np.uint64)[None, :]
    c = [np.broadcast_to(np.asarray(v, dtype=np.uint64), (B, P)) for v in address(i, q, counter, P)]
    x, y, z, w = PR.philox4x32_10(*c, k0, k1)
    rad, ang = np.sqrt(-2.0 * np.log(PR.u01_open0_d(x, y))), 2.0 * np.pi * PR.u01_d(z, w)
    eps = rad * (np.sin(ang) if second else np.cos(ang))
    qs = np.uint64(P if select_q is None else select_q)
    c = [np.broadcast_to(np.asarray(v, dtype=np.uint64), (B,)) for v in address(i[:, 0], qs, counter, P)]
    x, y, _, _ = PR.philox4x32_10(*c, k0, k1)
    unif = PR.u01_d(x, y)
    return eps, (unif < prob).astype(np.float64), unif


# the mutations of the host address (each must make the assertion next to it fail)
def _swapped(i, q, counter, P):
    return q, i, counter & 0xFFFFFFFF, JITTER_STREAM ^ (counter >> 32)


def _counter_plus_one(i, q, counter, P):
    return jitter_address(i, q, counter + 1, P)


def _no_xor(i, q, counter, P):
    return i, q, counter & 0xFFFFFFFF, JITTER_STREAM


MUTATIONS = {
    "words i and q swapped": dict(address=_swapped),
    "counter + 1": dict(address=_counter_plus_one),
    "select from call q = P - 1": dict(select_q=-1),  # (resolved to P - 1 by ``mutated_draws``)
    "stream word without the xor": dict(address=_no_xor),
    "second Box-Muller normal": dict(second=True),
}


def mutated_draws(name, seed, counter, B, P, prob):
    kw = dict(MUTATIONS[name])
    if kw.get("select_q") == -1:
        kw["select_q"] = P - 1
    return jitter_draws(seed, counter, B, P, prob, **kw)
