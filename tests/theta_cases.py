"""TEST INFRASTRUCTURE - the case list of ``tests/test_theta_parity_gpu.py`` as numpy generators, so that
``tests/test_theta_oracle_cpu.py`` can assert the INPUT CONDITIONS of those comparisons (few resampling positions within delta of a
cdf entry, well-conditioned quartile picks) on exactly the inputs the GPU tests use.  No torch, no product import."""
import math

import numpy as np

from tests import theta_oracle as O

DTYPES = ("float64", "float32")
# the one-workgroup kernels split B into ceil(B / 256) entries per thread: one thread holds anything (1, 2), one wave (63 .. 65), one
# thread owns nothing / every thread one / half the threads nothing (255, 256, 257), the same one chunk size up (511, 513), ragged
# chunks (1000), and 17 entries per thread with a single entry in the last chunk that holds anything (4097)
B_ALL = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4097)
P_ALL = tuple(range(1, 9))
B_EVERY_P = (1, 65, 257, 1000)
P_EVERY_B = (1, 3, 8)
BP = tuple(sorted({(b, p) for b in B_EVERY_P for p in P_ALL} | {(b, p) for b in B_ALL for p in P_EVERY_B}))

WEIGHTS = ("plain", "nonfinite", "first", "last", "nothing", "spread")  # (pf_theta_fit also takes logw = NULL)
RESAMPLE_U = (0.0, 2.0 ** -53, 0.3718, 0.999999, 1.0)

# the seven families with the parameter values of tests/test_theta_kernels_gpu.py::PRIORS and tests/test_ness_gpu.py::_priors
PRIORS = ((O.NORMAL, 0.3, 1.7), (O.LOGNORMAL, -2.0, 0.8), (O.EXPONENTIAL, 4.0, 0.0), (O.GAMMA, 2.5, 3.0), (O.HALFNORMAL, 0.7, 0.0),
          (O.BETA, 2.0, 5.0), (O.UNIFORM, -0.4, 1.3))
NESS_PRIORS = ((O.NORMAL, 0.0, 1.0), (O.LOGNORMAL, -2.0, 1.0), (O.EXPONENTIAL, 10.0, 0.0), (O.GAMMA, 2.0, 3.0), (O.HALFNORMAL, 1.0, 0.0),
               (O.BETA, 2.0, 3.0), (O.UNIFORM, -1.0, 2.0), (O.NORMAL, 0.5, 2.0))
TAIL_U = (-800.0, -90.0, -40.0, -17.5, -1e-3, 0.0, 17.5, 20.0, 40.0, 90.0, 800.0)  # exp and sigmoid tails in both dtypes

DELTA32 = 4.0 * 2.0 ** -24  # one rounding of the cdf, three of the position ((float) i + (float) u, the sum, the quotient)


def delta64(b):
    return 8.0 * b * 2.0 ** -53  # the running sum of B terms in another order, with room


# the float64 oracle's own error in the Gaussian fit, in units of 2^-53 times its first-order shape (the sum of absolute terms of the
# mean; ``theta_oracle.cholesky_error_shape`` for the factor): measured against extended precision over the whole case list by
# tests/test_theta_oracle_cpu.py::test_fit_floor (28.4 for the mean, 24.6 for the factor - sums of up to 4097 terms), rounded up
FIT_K = 32.0


def near_cap(b):
    return max(2, 0.01 * b)


def _stable(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def seed_of(*key):
    return [(_stable(k) if isinstance(k, str) else int(k)) for k in key]


def logw(pattern, b, dtype, salt=0):
    """The log-weights of one pattern, already rounded to ``dtype`` (float64 array)."""
    g = np.random.default_rng(seed_of("logw", pattern, b, salt))
    w = 3.0 * g.standard_normal(b)
    if pattern == "nonfinite":  # NaN, +inf and -inf entries (they carry no weight)
        for k, v in zip(g.permutation(b)[: min(b - 1, 3)], (math.nan, math.inf, -math.inf)):
            w[k] = v
        if b >= 8:
            w[g.random(b) < 0.1] = -math.inf
            w[b // 2] = 0.25  # (at least one particle carries weight)
    elif pattern in ("first", "last"):  # all the mass on one particle
        w[:] = -math.inf
        w[0 if pattern == "first" else b - 1] = 0.5
    elif pattern == "nothing":  # nothing finite: equal weights
        w[:] = -math.inf
    elif pattern == "spread":
        w = g.standard_normal(b) * 30.0 - 700.0
    else:
        assert pattern == "plain", pattern
    return O.rounded(w, dtype)


def values(kind, b, p, dtype, salt=0):
    """Value patterns of the Gaussian fit: correlated columns; one column of exactly 0.0 (the diagonal fallback with exact zeros)."""
    g = np.random.default_rng(seed_of("values", kind, b, p, salt))
    mix = g.standard_normal((p, p))
    x = g.standard_normal((b, p)) @ mix + g.standard_normal(p)
    if kind == "zero_column":
        x[:, p - 1] = 0.0
    else:
        assert kind == "correlated", kind
    return O.rounded(x, dtype)


def rotated(priors, k):
    return tuple(priors[(i + k) % len(priors)] for i in range(len(priors)))


def propose_case(rot, dtype):
    """P = 8, the seven families rotated by ``rot`` (so that over rot = 0 .. 6 every family sits first, last - position 6 - and at
    p = 7, which repeats the family at position 0): mean, a lower factor with a zero row, and eps rows that drive EVERY parameter to
    each of ``TAIL_U`` (the factor's rows are solved for it), followed by plain rows."""
    pri = rotated(PRIORS, rot)
    pri = pri + (pri[0],)
    p = len(pri)
    g = np.random.default_rng(seed_of("propose", rot))
    mean = O.rounded(0.5 * g.standard_normal(p), dtype)
    chol = np.tril(0.6 * g.standard_normal((p, p)))
    chol[np.arange(p), np.arange(p)] = 0.5 + np.abs(np.diag(chol))
    chol[3, :] = 0.0  # a zero row: that parameter stays at its mean
    chol = O.rounded(chol, dtype)
    rows = []
    for target in TAIL_U:  # forward substitution: eps with mean + L eps = target in every row (row 3 keeps its mean)
        e = np.zeros(p)
        for i in range(p):
            e[i] = 0.0 if chol[i, i] == 0.0 else (target - mean[i] - chol[i, :i] @ e[:i]) / chol[i, i]
        rows.append(e)
    eps = np.concatenate([np.array(rows), g.standard_normal((300 - len(rows), p))])
    return pri, mean, chol, O.rounded(eps, dtype)


def accept_case(b, p, dtype, diag):
    """Forward / reverse factors with diagonal ``diag`` (1e-3 / 1e3 / 1), plain inputs, and the special entries of the issue when B
    has room for them: ``ll_star`` NaN / -inf / +inf, ``ll_cur`` -inf, ``unif`` exactly 0 and 1 - 2^-24."""
    g = np.random.default_rng(seed_of("accept", b, p, diag))
    r = g.standard_normal
    fac = lambda: np.tril(0.3 * r((p, p)), -1) * diag + np.diag(diag * (1.0 + 0.2 * g.random(p)))  # noqa: E731
    fwd, rev = (O.rounded(r(p), dtype), O.rounded(fac(), dtype)), (O.rounded(r(p), dtype), O.rounded(fac(), dtype))
    u_cur = O.rounded(rev[0] + r((b, p)) @ np.tril(rev[1]).T, dtype)
    u_star = O.rounded(fwd[0] + r((b, p)) @ np.tril(fwd[1]).T, dtype)
    pr_cur, pr_star, ll_cur, ll_star = (O.rounded(r(b), dtype) for _ in range(4))
    unif = g.random(b)
    for k, (arr, v) in enumerate(((ll_star, math.nan), (ll_star, -math.inf), (ll_star, math.inf), (ll_cur, -math.inf), (unif, 0.0),
                                  (unif, 1.0 - 2.0 ** -24))):
        if b > 2 * k + 8:
            arr[2 * k + 3] = v
    if b > 40:
        ll_cur[21], unif[21] = -math.inf, 0.0  # a log ratio of +inf against log(0) = -inf: accepted (unif > 0 is not needed for it)
    return dict(u_cur=u_cur, u_star=u_star, fwd=fwd, rev=rev, prior_cur=pr_cur, prior_star=pr_star, ll_cur=ll_cur, ll_star=ll_star,
                unif=O.rounded(unif, dtype))


JITTER_B = (1, 2, 3, 255, 256, 257)  # what SIZES of tests/test_ness_gpu.py (from 7) leaves out
JITTER_FAMILIES = ("nonshrinking", "shrinking", "liuwest", "constant", "constant_vector")
JITTER_KIND = dict(nonshrinking=O.NONSHRINKING, shrinking=O.SHRINKING, liuwest=O.LIUWEST, constant=O.CONSTANT, constant_vector=O.CONSTANT)
LIUWEST_A = 0.98


def jitter_case(b, p, family, discrete, dtype):
    """Values ``randn (B, P)``, log-weights ``2 randn``, ancestors by the oracle's systematic resampling, the draws."""
    g = np.random.default_rng(seed_of("jitter", b, p, family, int(discrete)))
    x = O.rounded(g.standard_normal((b, p)), dtype)
    lw = O.rounded(2.0 * g.standard_normal(b), dtype)
    anc = O.systematic(lw, 0.37, "float64")[0]
    eps = O.rounded(g.standard_normal((b, p)), dtype)
    sel = (g.random(b) < b ** -0.5).astype(np.float64)
    par, scale = 0.0, None
    if family == "liuwest":
        par = LIUWEST_A
    elif family == "constant":
        par = 0.125
    elif family == "constant_vector":
        scale = np.arange(1, p + 1) / 16.0
    return dict(x=x, lw=lw, anc=anc, eps=eps, sel=sel if discrete else None, kind=JITTER_KIND[family], par=par, scale=scale)


def quartile_gap(x, w):
    """``_quartile_gap`` of tests/test_ness_gpu.py in numpy: the smallest margin by which a quartile pick of ``robust_var`` beats a
    position holding another value whose weight moves the cdf."""
    order = np.argsort(x, axis=0, kind="stable")
    srt = np.take_along_axis(x, order, axis=0)
    cdf = np.cumsum(w[order], axis=0)
    gap = math.inf
    for q in (0.25, 0.75):
        d = np.abs(cdf - q)
        best = np.argmin(d, axis=0)
        for c in range(x.shape[1]):
            moved = np.ones(x.shape[0], dtype=bool)
            moved[1:] = cdf[1:, c] != cdf[:-1, c]
            other = (srt[:, c] != srt[best[c], c]) & moved
            if other.any():
                gap = min(gap, float((d[other, c] - d[best[c], c]).min()))
    return gap


OWN_B, OWN_P = (1, 255, 257, 1000), (1, 3, 8)
OWN_SEEDS, OWN_COUNTERS = (0, 2 ** 32 + 7), (0, 1, 2 ** 32 + 5)
