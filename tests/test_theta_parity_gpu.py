"""The theta-level kernels (``csrc/pf_theta.hpp``: ``pf_theta_fit / _propose / _accept / _resample / _path / _step``) and the
jittering kernels (``csrc/pf_jitter.hpp``: ``pf_jitter_fit / _apply``) against the host oracle ``tests/theta_oracle.py`` - numpy
float64 written from the reference's sources, pinned without a GPU by ``tests/test_theta_oracle_cpu.py`` (the reference's
recordings, scipy, mpmath, the product's torch route) - at every P, at the sizes around the one-workgroup kernels' tiling edges
(``tests/theta_cases.py``: B = 1, 2, 63 .. 65, 255 .. 257, 511, 513, 1000, 4097), in both tensor types.

Bars.  float64: the project's theta bar, rtol 1e-11 / atol 1e-12, plus - where the oracle's own float64 error does not leave it a
factor of 8 - eight times that error: the conditioning floor of the Beta density (``theta_oracle.prior_floor``, measured against
50 digits on the CPU) and, for the Gaussian fit, ``theta_cases.FIT_K`` x 2^-53 x the first-order error shape of the case (measured
against extended precision on the CPU; only an ill-scaled cloud, whose pivots are almost rounding, feels it).  Never from the
kernels' output.
float32: the kernels compute in double from the float32 inputs and round once - elementwise outputs (u, x, w_path) within rtol
2^-22 of the float32 rounding of the oracle, sums that can cancel (mean, factor, summed log prior, log_acc) within 2^-22 of the
oracle's sum of absolute terms.  Non-finite entries are compared, not masked: -inf matches -inf, NaN matches NaN.

Figures go to the file named by ``THETA_PARITY_REPORT`` when it is set (``profiles/theta_parity.txt`` is assembled from it)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from pyfilter_amd import _lib, ops
from pyfilter_amd.inference.pmmh import ThetaDraws
from tests import philox_ref as PR
from tests import theta_cases as TC
from tests import theta_oracle as O

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-11, 1e-12
ULP32 = 2.0 ** -22
TORCH = dict(float64=torch.float64, float32=torch.float32)
WORST = {}


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(TORCH[dtype]).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def packed(priors):
    pk = _lib.PfThetaPriors()
    pk.P = len(priors)
    for i, (kind, a, b) in enumerate(priors):
        pk.kind[i], pk.a[i], pk.b[i] = kind, a, b
    return pk


def note(key, share):
    WORST[key] = max(WORST.get(key, 0.0), float(share))


def check(got, want, bar, what, key):
    """Every entry: non-finite ones identical (NaN = NaN, the infinities by sign), finite ones within ``bar`` (an array or a number);
    the largest difference as a share of its bar is kept for the report."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
    odd = ~fin & ~np.isnan(want)
    assert np.array_equal(got[odd], want[odd]), f"{what}: infinities {got[odd][:5]} vs {want[odd][:5]}"
    if fin.any():
        diff = np.abs(got[fin] - want[fin])
        share = diff / np.maximum(bar[fin], 1e-300)
        k = int(np.argmax(share))
        assert share[k] <= 1.0, f"{what}: |{got[fin][k]!r} - {want[fin][k]!r}| = {diff[k]:.3g} > {bar[fin][k]:.3g} (entry {np.argwhere(fin)[k].tolist()})"
        note(key, share[k])


def bar_elementwise(want, dtype, extra=0.0):
    return ATOL64 + RTOL64 * np.abs(want) + extra if dtype == "float64" else ULP32 * np.abs(O.rounded(want, dtype))


def bar_sum(want, mag, dtype, extra=0.0):
    return ATOL64 + RTOL64 * np.abs(want) + extra if dtype == "float64" else ULP32 * mag


def as_dtype(want, dtype):
    with np.errstate(over="ignore"):
        return O.rounded(want, dtype)


# ---- fit -----------------------------------------------------------------------------------------------------------------------
def _fit_case(x, lw, dtype, what, key):
    """One launch against the oracle: mean and factor within their bars, the factor lower-triangular bit for bit.  Returns how the
    factor was decided: "cholesky", "fallback" (a covariance that is singular in ANY arithmetic: a zero column, one weighted point) or
    "rounding" - a cloud of fewer weighted points than parameters, whose pivot from ``first_bad`` on is rounding noise about 0, so that
    whether ``cholesky_ex`` succeeds depends on the summation order, in the reference too: there the kernel must give either the
    diagonal fallback or a factor whose columns left of that pivot are the oracle's."""
    b, p = x.shape
    mean, chol = ops.theta_fit(dev(x, dtype), None if lw is None else dev(lw, dtype), 1.1)
    got_m, got_l = host(mean), host(chol)
    assert np.array_equal(got_l, np.tril(got_l)), f"{what}: factor not lower-triangular"
    want_m, want_l, info = O.fit(x, lw, 1.1)
    unit = 8.0 * TC.FIT_K * 2.0 ** -53  # eight times the oracle's own measured error (tests/test_theta_oracle_cpu.py::test_fit_floor)
    sd = 1.1 * np.sqrt(np.diag(info["abs_cov"]))  # |L[i, j]| <= scale * sqrt(cov[i, i]) <= this
    bar_m = unit * info["abs_mean"] + (ATOL64 + RTOL64 * np.abs(want_m) if dtype == "float64" else ULP32 * info["abs_mean"])
    check(got_m, as_dtype(want_m, dtype), bar_m, f"{what}: mean", key + ("mean",))

    def bar_l(want, shape):
        return unit * shape + (ATOL64 + RTOL64 * np.abs(want) if dtype == "float64" else ULP32 * sd[:, None] + np.zeros_like(want))

    diag_shape = np.diag(sd)
    bad = info["first_bad"]
    if (np.diag(info["cov"]) == 0.0).any():  # singular whatever the arithmetic: a row of the covariance is exactly 0, its pivot too
        assert info["fallback"], what
        check(got_l, as_dtype(info["diagonal"], dtype), bar_l(info["diagonal"], diag_shape), f"{what}: fallback", key + ("factor",))
        return "fallback", got_m, got_l
    shape = 1.1 * O.cholesky_error_shape(info["abs_cov"], info["cholesky"] / 1.1)
    if bad is None:
        assert not info["fallback"], what
        check(got_l, as_dtype(want_l, dtype), bar_l(want_l, shape), f"{what}: factor", key + ("factor",))
        return "cholesky", got_m, got_l
    if np.array_equal(got_l, np.diag(np.diag(got_l))) and p > 1:
        check(got_l, as_dtype(info["diagonal"], dtype), bar_l(info["diagonal"], diag_shape), f"{what}: fallback by rounding", key + ("factor",))
    else:
        left = info["cholesky"][:, :bad]
        check(got_l[:, :bad], as_dtype(left, dtype), bar_l(left, shape[:, :bad]), f"{what}: columns left of the rounding pivot", key + ("factor",))
    return "rounding", got_m, got_l


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("b,p", TC.BP)
def test_fit_is_the_oracles_weighted_gaussian(dtype, b, p):
    """Every weight pattern (plain, NaN / +inf / -inf entries, all the mass on the first / last particle, nothing finite, ``logw =
    NULL``, the spread ``30 randn - 700``) on correlated columns and on a column of exactly 0.0, which takes the diagonal fallback with
    exact zeros - as does B = 1, whose covariance is 0.  (No non-zero constant column: whether its variance comes out as 0 or as 1e-34
    depends on the summation order, in the reference too.)"""
    how = dict(cholesky=0, fallback=0, rounding=0)
    for pattern in TC.WEIGHTS + ("null",):
        lw = None if pattern == "null" else TC.logw(pattern, b, dtype)
        for kind in ("correlated", "zero_column"):
            x = TC.values(kind, b, p, dtype)
            decided, got_m, got_l = _fit_case(x, lw, dtype, f"B={b} P={p} {pattern} {kind}", ("fit", dtype))
            how[decided] += 1
            if b == 1 or pattern in ("first", "last") or (kind == "zero_column" and p == 1):
                assert decided == "fallback", (pattern, kind, decided)
                assert not got_l.any(), "one weighted point: no covariance"
            elif kind == "zero_column":
                assert decided == "fallback" and np.array_equal(got_l, np.diag(np.diag(got_l))), (pattern, kind, decided)
            if kind == "zero_column":
                assert got_l[p - 1, p - 1] == 0.0 and not got_l[p - 1].any() and got_m[p - 1] == 0.0
            if b == 1:
                assert np.array_equal(got_m, as_dtype(x[0], dtype))
    if b >= 63:
        assert how["cholesky"] >= 3, how  # (plain, nonfinite and NULL weights on correlated columns are well determined)
    for name, count in how.items():
        WORST[("fit", dtype, f"cases decided by {name}")] = WORST.get(("fit", dtype, f"cases decided by {name}"), 0) + count


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("col", [0, 2])
def test_fit_with_a_nan_value_keeps_the_nan_as_the_torch_route_does(dtype, col):
    """A NaN in one value column: ``construct_mvn`` on torch returns a NaN mean entry and - ``cholesky_ex`` reporting failure - the
    diagonal fallback with NaN in that entry and the other columns' standard deviations next to it
    (``tests/test_theta_oracle_cpu.py`` records it on the CPU); so does the kernel."""
    x = TC.values("correlated", 257, 3, dtype)
    x[7, col] = math.nan
    mean, chol = ops.theta_fit(dev(x, dtype), None, 1.1)
    got_m, got_l = host(mean), host(chol)
    want_m, want_l, info = O.fit(x, None, 1.1)
    assert info["fallback"] and np.isnan(want_m[col]) and np.isnan(want_l[col, col]) and np.isnan(want_l).sum() == 1
    check(got_m, as_dtype(want_m, dtype), bar_sum(want_m, info["abs_mean"], dtype), "mean", ("fit", dtype, "mean"))
    sd = np.nan_to_num(np.sqrt(np.diag(info["abs_cov"])))
    check(got_l, as_dtype(want_l, dtype), bar_sum(want_l, 1.1 * sd[:, None] + np.zeros_like(want_l), dtype), "factor", ("fit", dtype, "factor"))


# ---- propose -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("rot", range(7))
def test_propose_is_the_oracles_bijections_and_densities(dtype, rot):
    """P = 8 with the family list rotated (every family first, last and at p = 7), a factor with a zero row, eps rows that drive every
    parameter to u = -800 .. 800: the stored u, every constrained x and the summed log prior - non-finite entries included - against
    the oracle evaluated at the u the kernel stored (what every later evaluation starts from)."""
    pri, mean, chol, eps = TC.propose_case(rot, dtype)
    p, b = len(pri), eps.shape[0]
    out = [torch.empty(b, device="cuda", dtype=TORCH[dtype]) for _ in range(p)]
    u, lp = ops.theta_propose(packed(pri), dev(mean, dtype), dev(chol, dtype), dev(eps, dtype), out)
    want_u, mag_u = O.propose(mean, chol, eps, dtype)
    got_u = host(u)
    check(got_u, want_u, bar_sum(want_u, mag_u, dtype) if dtype == "float64" else ULP32 * np.abs(want_u), f"rot={rot}: u", ("propose", dtype, "u"))
    assert np.array_equal(got_u[:, 3], np.broadcast_to(mean[3], (b,))), "the zero row keeps its mean"
    reached = {round(float(v), 3) for v in got_u[: len(TC.TAIL_U), 0]}
    assert {round(v, 3) for v in TC.TAIL_U} <= reached, reached
    kinds, pa, pb = zip(*pri)
    total, xs, mag, floor = O.log_prior(kinds, pa, pb, got_u, dtype)
    got_x = np.stack([host(o) for o in out], axis=1)
    for k, (kind, a, b_) in enumerate(pri):
        want_x = as_dtype(xs[:, k], dtype)
        check(got_x[:, k], want_x, bar_elementwise(xs[:, k], dtype), f"rot={rot} p={k} kind={kind}: x", ("propose", dtype, "x"))
        if dtype == "float32" and kind in (O.BETA, O.UNIFORM):  # the open support, and the float32 clamp where it binds
            lo, hi = (0.0, 1.0) if kind == O.BETA else (a, b_)
            x32 = got_x[:, k].astype(np.float32)
            assert (x32 < np.float32(hi)).all() and ((x32 > np.float32(lo)) if kind == O.BETA else (x32 >= np.float32(lo))).all(), (kind, k)
            top = lo + (hi - lo) * (1.0 - 2.0 ** -23)
            binds = got_u[:, k] > 17.0
            assert (binds.sum() >= 4 or k == 3) and np.array_equal(x32[binds], np.full(int(binds.sum()), top, dtype=np.float32)), (kind, x32[binds])
            if kind == O.BETA:
                assert np.array_equal(x32[got_u[:, k] < -88.0], np.full(int((got_u[:, k] < -88.0).sum()), 2.0 ** -126, dtype=np.float32))
    with np.errstate(over="ignore"):
        want_lp = as_dtype(total, dtype)
    check(host(lp), want_lp, bar_sum(total, mag, dtype, 8.0 * floor), f"rot={rot}: summed log prior", ("propose", dtype, "log prior"))
    assert (~np.isfinite(want_lp)).sum() >= 2, "the tails reach non-finite densities"


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("b,p", TC.BP)
def test_propose_at_every_size(dtype, b, p):
    """The first P families at the tiling sizes (one thread per theta-particle: a ragged last workgroup at 257, 513, 1000, 4097)."""
    pri = TC.PRIORS[:p] if p <= 7 else TC.PRIORS + (TC.PRIORS[0],)
    g = np.random.default_rng(TC.seed_of("propose_size", b, p))
    mean = O.rounded(0.5 * g.standard_normal(p), dtype)
    chol = O.rounded(np.tril(0.6 * g.standard_normal((p, p))), dtype)
    eps = O.rounded(g.standard_normal((b, p)), dtype)
    out = [torch.empty(b, device="cuda", dtype=TORCH[dtype]) for _ in range(p)]
    u, lp = ops.theta_propose(packed(pri), dev(mean, dtype), dev(chol, dtype), dev(eps, dtype), out)
    want_u, mag_u = O.propose(mean, chol, eps, dtype)
    got_u = host(u)
    check(got_u, want_u, bar_sum(want_u, mag_u, dtype) if dtype == "float64" else ULP32 * np.abs(want_u), f"B={b} P={p}: u", ("propose", dtype, "u"))
    kinds, pa, pb = zip(*pri)
    total, xs, mag, floor = O.log_prior(kinds, pa, pb, got_u, dtype)
    check(np.stack([host(o) for o in out], axis=1), as_dtype(xs, dtype), bar_elementwise(xs, dtype), f"B={b} P={p}: x", ("propose", dtype, "x"))
    check(host(lp), as_dtype(total, dtype), bar_sum(total, mag, dtype, 8.0 * floor), f"B={b} P={p}: log prior", ("propose", dtype, "log prior"))


# ---- accept --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("diag", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("b,p", TC.BP)
def test_accept_is_the_oracles_metropolis_hastings_step(dtype, b, p, diag):
    """log_acc against the oracle (P = 8: all 64 loader threads fill the LDS factor, no identity row left; P = 1: one entry);
    ``accepted`` against ``log(unif) < log_acc`` on the ORACLE's log_acc wherever the two are further apart than the comparison bar
    (at most 1 % of the entries are closer: those are compared on the kernel's own stored log_acc); ``rate`` = mean of the mask."""
    c = TC.accept_case(b, p, dtype, diag)
    d = lambda v: dev(v, dtype)  # noqa: E731
    log_acc, acc, rate = ops.theta_accept(d(c["u_cur"]), d(c["u_star"]), (d(c["fwd"][0]), d(c["fwd"][1])), (d(c["rev"][0]), d(c["rev"][1])),
                                          d(c["prior_cur"]), d(c["prior_star"]), d(c["ll_cur"]), d(c["ll_star"]), d(c["unif"]))
    want, mag = O.log_accept(c["u_cur"], c["u_star"], c["fwd"], c["rev"], c["prior_cur"], c["prior_star"], c["ll_cur"], c["ll_star"])
    got = host(log_acc)
    what = f"B={b} P={p} diag={diag}"
    bar = bar_sum(want, mag, dtype)
    check(got, as_dtype(want, dtype), bar, f"{what}: log_acc", ("accept", dtype, "log_acc"))
    got_acc = acc.cpu().numpy()
    assert got_acc.dtype == np.bool_
    with np.errstate(divide="ignore", invalid="ignore"):
        log_u = np.log(c["unif"])
        far = ~(np.abs(log_u - want) <= np.where(np.isfinite(want), bar, 0.0))  # (NaN, infinities: decided whatever the rounding)
    assert (~far).sum() <= 0.01 * b, (what, int((~far).sum()))
    note(("accept", dtype, "entries within the bar of log(unif) (of all entries)"), (~far).sum())
    assert np.array_equal(got_acc[far], O.accepted(c["unif"], want)[far]), f"{what}: accepted mask"
    assert np.array_equal(got_acc[~far], O.accepted(c["unif"], got)[~far]), f"{what}: accepted mask near the threshold"
    assert abs(float(rate) - got_acc.mean()) <= (1e-12 if dtype == "float64" else 2.0 ** -23), what
    if b > 40:  # NaN / -inf proposals rejected; +inf ratios accepted (also against unif = 0: log 0 = -inf < +inf)
        assert not got_acc[3] and not got_acc[5] and got_acc[7] and got_acc[9] and got_acc[21] and want[21] == math.inf
        assert c["unif"][11] == 0.0 and got_acc[11] == (want[11] > -math.inf) and c["unif"][13] == 1.0 - 2.0 ** -24


# ---- resample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("b", TC.B_ALL)
def test_resample_is_the_oracles_systematic_resampling(dtype, b):
    """Every weight pattern and u = 0, 2^-53, 0.3718, 0.999999, 1.  An ancestor may differ from the oracle's only where the position
    lies within delta of the float64 cdf entry that separates the two (delta_64 = 8 B 2^-53, delta_32 = 4 * 2^-24:
    ``philox_ref.valid_ancestor``; ``tests/test_theta_oracle_cpu.py`` bounds how many positions are that close); ancestors are
    monotone and inside [0, B - 1]; equal weights are exact by construction and asserted exactly."""
    delta = TC.DELTA32 if dtype == "float32" else TC.delta64(b)
    for pattern in TC.WEIGHTS:
        lw = TC.logw(pattern, b, dtype)
        for u in TC.RESAMPLE_U:
            got = ops.theta_resample(dev(lw, dtype), u).cpu().numpy()
            what = f"B={b} {pattern} u={u!r}"
            assert got.dtype == np.int64 and got.min() >= 0 and got.max() <= b - 1 and (np.diff(got) >= 0).all(), what
            want, cdf, pos = O.systematic(lw, u, dtype)
            if pattern == "nothing":
                assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
                if u == 0.0:
                    assert np.array_equal(got, np.maximum(np.arange(b) - 1, 0)), what  # position i / B sits ON cdf[i - 1]
                continue
            assert PR.valid_ancestor(got, pos, cdf, delta).all(), (what, np.argwhere(~PR.valid_ancestor(got, pos, cdf, delta))[:5].tolist())
            differ = int((got != want).sum())
            assert differ <= TC.near_cap(b), (what, differ)
            note(("resample", dtype, "ancestors that differ from the oracle's (all within delta), largest count in a case"), differ)
            if pattern in ("first", "last"):
                k = 0 if pattern == "first" else b - 1
                assert (got[1:] == k).all() and got[0] in ((0, k) if u == 0.0 else (k,)), what


def test_resample_refuses_a_uniform_outside_the_unit_interval_and_bad_sizes():
    """Return codes only - nothing here launches (every pointer is null or the call is refused before it is read)."""
    lib = _lib.load()
    one = torch.zeros(8, device="cuda", dtype=torch.float64)
    idx = torch.zeros(8, device="cuda", dtype=torch.int64)
    for u in (-1e-9, 1.0 + 1e-9, math.nan):
        assert lib.pf_theta_resample(one.data_ptr(), 8, C.c_double(u), _lib.PF_F64, idx.data_ptr(), one.data_ptr(), None) != 0, u
    assert lib.pf_theta_resample(one.data_ptr(), 0, C.c_double(0.5), _lib.PF_F64, idx.data_ptr(), one.data_ptr(), None) != 0
    for p in (0, 9):
        assert lib.pf_theta_fit(one.data_ptr(), None, 8, p, C.c_double(1.0), _lib.PF_F64, one.data_ptr(), one.data_ptr(), None) != 0, p
        assert lib.pf_theta_accept(*([one.data_ptr()] * 11), 8, p, _lib.PF_F64, one.data_ptr(), idx.data_ptr(), one.data_ptr(), None) != 0, p
        assert lib.pf_jitter_fit(one.data_ptr(), one.data_ptr(), 8, p, 0, C.c_double(0.0), None, C.c_double(0.0), C.c_double(0.0),
                                 C.c_double(1.0), _lib.PF_F64, one.data_ptr(), None, None, None) != 0, p
    assert lib.pf_theta_fit(one.data_ptr(), None, 0, 1, C.c_double(1.0), _lib.PF_F64, one.data_ptr(), one.data_ptr(), None) != 0
    assert lib.pf_theta_accept(*([one.data_ptr()] * 11), 0, 1, _lib.PF_F64, one.data_ptr(), idx.data_ptr(), one.data_ptr(), None) != 0
    ptrs = (C.c_void_p * 8)(*([one.data_ptr()] * 8))
    for p, kind in ((0, 0), (9, 0), (1, 7), (1, -1)):  # P = 0, P = 9, an unknown prior kind
        pk = packed([(0, 0.0, 1.0)])
        pk.P, pk.kind[0] = p, kind
        assert lib.pf_theta_propose(C.byref(pk), one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, _lib.PF_F64, one.data_ptr(), ptrs,
                                    one.data_ptr(), None) != 0, (p, kind)
        assert lib.pf_jitter_apply(C.byref(pk), one.data_ptr(), idx.data_ptr(), one.data_ptr(), 1, 0, C.c_double(0.0), C.c_double(0.0),
                                   C.c_double(1.0), 0, None, None, 0, 0, _lib.PF_F64, one.data_ptr(), ptrs, None) != 0, (p, kind)
    ok = packed([(0, 0.0, 1.0)])
    assert lib.pf_theta_propose(C.byref(ok), one.data_ptr(), one.data_ptr(), one.data_ptr(), 0, _lib.PF_F64, one.data_ptr(), ptrs,
                                one.data_ptr(), None) != 0  # B = 0
    for par in (-0.01, 1.01, math.nan):  # Liu-West `a` outside [0, 1]
        assert lib.pf_jitter_fit(one.data_ptr(), one.data_ptr(), 8, 1, _lib.JITTER_LIUWEST, C.c_double(par), None, C.c_double(0.0),
                                 C.c_double(0.0), C.c_double(1.0), _lib.PF_F64, one.data_ptr(), None, None, None) != 0, par
        assert lib.pf_jitter_apply(C.byref(ok), one.data_ptr(), idx.data_ptr(), one.data_ptr(), 1, _lib.JITTER_LIUWEST, C.c_double(par),
                                   C.c_double(0.0), C.c_double(1.0), 0, None, None, 0, 0, _lib.PF_F64, one.data_ptr(), ptrs, None) != 0, par
    assert lib.pf_jitter_fit(one.data_ptr(), one.data_ptr(), 0, 1, 0, C.c_double(0.0), None, C.c_double(0.0), C.c_double(0.0),
                             C.c_double(1.0), _lib.PF_F64, one.data_ptr(), None, None, None) != 0


# ---- path / step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("n", [1, 8, 9, 17])
@pytest.mark.parametrize("b", [1, 255, 257])
def test_path_and_step_are_the_oracles_ordered_additions(dtype, n, b):
    """The kernel's unrolled groups of 8 end at 8 and 16: bit-equal to the additions in order in the tensors' type, the statistics
    rows against ``ess``; n = 1 also through ``pf_theta_step``, where ``w_path`` IS ``w0``."""
    g = np.random.default_rng(TC.seed_of("path", n, b))
    w0 = O.rounded(g.standard_normal(b), dtype)
    ll = O.rounded(2.0 * g.standard_normal((n, b)), dtype)
    if n > 4 and b > 8:
        ll[3, 7], ll[2, 5] = math.nan, -math.inf
    w_path, stats = ops.theta_path(dev(w0, dtype), dev(ll, dtype))
    want = O.path(w0, ll, dtype).astype(np.float64)
    got = host(w_path)
    assert np.array_equal(got, want, equal_nan=True), (n, b, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist())
    st = host(stats)
    for r in range(n):
        e, fin = O.path_stats(want[r])
        assert st[r, 1] == fin, (r, st[r], fin)
        check(st[r, 0], as_dtype(e, dtype), bar_elementwise(np.float64(e), dtype), f"n={n} B={b} row {r}: ESS",
              ("path", dtype, "ESS"))
    if n == 1:
        w = dev(w0, dtype)
        stats1 = ops.theta_step(w, dev(ll[0], dtype))
        assert np.array_equal(host(w), want[0], equal_nan=True) and torch.equal(stats1, stats[0])


# ---- jitter fit / apply at the sizes the existing sweep skips ------------------------------------------------------------------------
def _jitter_launch(c, pri, dtype, discrete, eps, sel, seed=0, counter=0):
    e = O.eps_of(dtype)
    b, p = c["x"].shape
    scale = None if c["scale"] is None else torch.from_numpy(c["scale"])
    fit, _, _ = ops.jitter_fit(dev(c["x"], dtype), dev(c["lw"], dtype), c["kind"], c["par"], scale, e, (e, 1 - e))
    out = [torch.empty(b, device="cuda", dtype=TORCH[dtype]) for _ in range(p)]
    u = ops.jitter_apply(packed(pri), dev(c["x"], dtype), torch.from_numpy(c["anc"]).cuda(), fit, c["kind"], c["par"], out, discrete,
                         None if eps is None else dev(eps, dtype), None if sel is None else dev(sel, dtype), seed, counter, (e, 1 - e))
    return host(fit), host(u), np.stack([host(o) for o in out], axis=1)


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("discrete", [False, True], ids=["all", "discrete"])
@pytest.mark.parametrize("family", TC.JITTER_FAMILIES)
@pytest.mark.parametrize("p", TC.P_EVERY_B)
@pytest.mark.parametrize("b", TC.JITTER_B)
def test_jitter_kernels_at_small_and_block_sized_b(dtype, b, p, family, discrete):
    """B = 1, 2, 3, 255, 256, 257 against the oracle at the bars of ``tests/test_ness_gpu.py`` (float64 rtol 1e-8 / atol 1e-10,
    float32 1 ulp).  What the reference's ``robust_var`` returns at the smallest sizes, and is required here: B = 1 - both quartile
    picks are the one particle, iqr = 0 <= var = 0, variance 0, so std is the ``min_std`` clamp; B = 2 - |cdf - 0.25| and
    |cdf - 0.75| over the two sorted particles pick per weight (the heavier one twice, or one each), variance min(iqr^2, var)."""
    c = TC.jitter_case(b, p, family, discrete, dtype)
    pri = TC.NESS_PRIORS[:p]
    fitted = O.jitter_fit(c["kind"], c["x"], c["lw"], c["par"], c["scale"], dtype)
    if c["kind"] != O.CONSTANT:
        assert TC.quartile_gap(c["x"], O.normalize(c["lw"])) >= 1e-9  # (test_theta_oracle_cpu.py: none of these cases is ill-conditioned)
    fit, u, x = _jitter_launch(c, pri, dtype, discrete, c["eps"], c["sel"])
    what = f"B={b} P={p} {family} discrete={discrete}"
    loose = lambda w: 1e-10 + 1e-8 * np.abs(w)  # noqa: E731
    check(fit[1], fitted[1], loose(fitted[1]), f"{what}: scale", ("jitter", dtype, "fit"))
    check(fit[2], fitted[2], loose(fitted[2]), f"{what}: std", ("jitter", dtype, "fit"))
    if b == 1 and c["kind"] != O.CONSTANT:
        assert (fit[1] == 0.0).all() and (fit[2] == O.eps_of(dtype)).all(), "one particle: no variance, the min_std clamp"
    want_u, _ = O.jitter_apply(c["kind"], c["x"], c["anc"], fitted, c["eps"], c["sel"], c["par"])
    kinds, pa, pb = zip(*pri)
    want_x = O.log_prior(kinds, pa, pb, want_u, dtype)[1]
    if dtype == "float64":
        check(u, want_u, loose(want_u), f"{what}: jittered (unconstrained)", ("jitter", dtype, "u"))
        check(x, want_x, loose(want_x), f"{what}: jittered (constrained)", ("jitter", dtype, "x"))
    else:
        check(u, as_dtype(want_u, dtype), ULP32 * np.abs(want_u), f"{what}: jittered (unconstrained)", ("jitter", dtype, "u"))
        check(x, as_dtype(want_x, dtype), ULP32 * np.abs(want_x), f"{what}: jittered (constrained)", ("jitter", dtype, "x"))


# ---- the jitter kernel's own draws --------------------------------------------------------------------------------------------------
def _own_vs_taped(c, pri, dtype, discrete, seed, counter, draws):
    """(largest share of the bar between the launch with its own draws and the taped launch fed ``draws``, select mask equal?)."""
    b, p = c["x"].shape
    eps, sel, _ = draws
    _, own_u, own_x = _jitter_launch(c, pri, dtype, discrete, None, None, seed, counter)
    fit, tap_u, tap_x = _jitter_launch(c, pri, dtype, discrete, eps, sel if discrete else None)
    if dtype == "float64":
        bar_u, bar_x = 1e-12 * np.maximum(1.0, np.abs(tap_u)), 1e-12 * np.maximum(1.0, np.abs(tap_x))
    else:  # the tape carries eps rounded to float32, the kernel keeps it in double: 2 ulp of |loc| + |std eps|
        fitted = O.jitter_fit(c["kind"], c["x"], c["lw"], c["par"], c["scale"], dtype)
        mag = O.jitter_apply(c["kind"], c["x"], c["anc"], fitted, O.rounded(eps, dtype), None, c["par"])[1]
        bar_u = 2.0 * 2.0 ** -23 * mag
        bar_x = None
    moved = np.any(own_u != c["x"][c["anc"]], axis=1)  # (a particle that is not selected keeps its ancestor's values bit for bit)
    mask_equal = (not discrete) or np.array_equal(moved, sel.astype(bool))
    share = float(np.max(np.abs(own_u - tap_u) / np.maximum(bar_u, 1e-300)))
    if bar_x is not None:
        share = max(share, float(np.max(np.abs(own_x - tap_x) / bar_x)))
    return share, mask_equal


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("discrete", [False, True], ids=["all", "discrete"])
@pytest.mark.parametrize("p", TC.OWN_P)
@pytest.mark.parametrize("b", TC.OWN_B)
def test_jitter_apply_draws_what_the_oracle_says(dtype, b, p, discrete):
    """``pf_jitter_apply`` with ``eps = select = None`` against the TAPED launch of the same call fed ``theta_oracle.jitter_draws`` -
    seeds 0 and 2^32 + 7, update counters 0, 1 and 2^32 + 5.  The select mask (read off which particles moved) is bit-equal; float64
    u and x within the Philox suite's 1e-12; float32 u within 2 ulp of |location| + |std eps| (the tape rounds eps to float32, the kernel
    keeps it in double - the only permitted difference).  Next to it the mutations of the host address, each of which must fail:
    words i and q swapped, counter + 1, select from call q = P - 1, the stream word without the xor, the second Box-Muller normal."""
    c = TC.jitter_case(b, p, "shrinking", discrete, dtype)
    pri = TC.NESS_PRIORS[:p]
    prob = b ** -0.5
    for seed in TC.OWN_SEEDS:
        for counter in TC.OWN_COUNTERS:
            draws = O.jitter_draws(seed, counter, b, p, prob)
            assert (np.abs(draws[2] - prob) > 1e-12).all()
            share, mask_equal = _own_vs_taped(c, pri, dtype, discrete, seed, counter, draws)
            assert mask_equal and share <= 1.0, (b, p, seed, counter, share, mask_equal)
            note(("own draws", dtype, "u / x"), share)
    seed, counter = TC.OWN_SEEDS[1], TC.OWN_COUNTERS[2]  # (a counter above 2^32: the xor is in play)
    for name in O.MUTATIONS:
        if name.startswith("select") and not discrete:
            continue
        wrong = O.mutated_draws(name, seed, counter, b, p, prob)
        if name.startswith("select"):
            if np.array_equal(wrong[1], O.jitter_draws(seed, counter, b, p, prob)[1]):
                continue  # (B = 1 and the like: the two calls happen to select the same particles)
        elif b * p == 1 and name.startswith("words"):
            continue  # (i = q = 0: swapping them is no mutation)
        share, mask_equal = _own_vs_taped(c, pri, dtype, discrete, seed, counter, wrong)
        rejected = (not mask_equal) if name.startswith("select") else share > 1.0
        assert rejected, f"mutation '{name}' passes at B={b} P={p} {dtype}"
        note(("own draws", dtype, f"mutation rejected: {name}"), 1)


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("discrete", [False, True], ids=["all", "discrete"])
def test_ness_updates_are_keyed_by_the_update_count(dtype, discrete):
    """Three consecutive ``OnlineKernel`` updates on the kernel route with ``seed = s``: update k equals the taped update fed
    ``jitter_draws(s, k)`` - the counter passed down is the update count (an update counter that does not advance, or starts at 1,
    fails here)."""
    from torch.distributions import Exponential, LogNormal, Normal

    from pyfilter_amd.inference import ThetaParticles
    from pyfilter_amd.inference.ness import OnlineKernel, ShrinkingKernel

    class Draws(ThetaDraws):
        taped = True

        def __init__(self, u, eps, sel):
            self.u, self.eps, self.sel, self.generator = u, eps, sel, None

        def uniform(self, shape):
            return torch.tensor(self.u, dtype=torch.float64)

        def normal(self, shape):
            return torch.from_numpy(self.eps)

        def bernoulli(self, shape, p):
            return torch.from_numpy(self.sel)

    class State:  # what ``OnlineKernel.update`` touches of an ``SMC2State``
        class filter_state:
            @staticmethod
            def resample(indices, entire_history=False):
                pass

    class Filter:
        @staticmethod
        def initialize_model(theta):
            pass

    b, s = 257, 2 ** 32 + 7
    pri = {"kappa": Exponential(10.0), "gamma": Normal(0.0, 1.0), "sigma": LogNormal(-2.0, 1.0)}
    thetas, kernels = [], []
    for _ in range(2):
        thetas.append(ThetaParticles(pri, b, "cuda", TORCH[dtype]).initialize_parameters(torch.Generator().manual_seed(3)))
        kernels.append(OnlineKernel(ShrinkingKernel(), discrete=discrete, seed=s))
    g = np.random.default_rng(TC.seed_of("ness", int(discrete)))
    for k in range(3):
        lw = dev(2.0 * g.standard_normal(b), dtype)
        u = float(g.random())
        eps, sel, unif = O.jitter_draws(s, k, b, 3, b ** -0.5)
        assert (np.abs(unif - b ** -0.5) > 1e-12).all()
        outs = []
        for theta, kernel, draws in ((thetas[0], kernels[0], PlainU(u)), (thetas[1], kernels[1], Draws(u, eps, sel))):
            st = State()
            st.w = lw.clone()
            assert kernel.updates == k
            kernel.update(theta, Filter, st, generator=draws)
            assert kernel.last_route == "kernels"
            outs.append(host(theta.stack_parameters(False)))
        # (each update adds the bar of one launch - 1e-12, or 2 float32 ulp - and carries what the two copies differed by before)
        scale = np.maximum(1.0, np.abs(outs[1]))
        bar = (k + 1) * (1e-12 if dtype == "float64" else 2.0 * 2.0 ** -23) * scale
        assert (np.abs(outs[0] - outs[1]) <= bar).all(), (k, float(np.max(np.abs(outs[0] - outs[1]) / scale)))
        wrong = O.jitter_draws(s, k + 1, b, 3, b ** -0.5)[0]
        assert np.abs(wrong - eps).max() > 1.0  # (so a counter off by one is a visibly different update)


class PlainU(ThetaDraws):
    """Only the resampling uniform is given: the kernel route draws eps / select itself."""

    taped = False

    def __init__(self, u):
        self.u, self.generator = u, None

    def uniform(self, shape):
        return torch.tensor(self.u, dtype=torch.float64)


def test_write_the_report():
    """Runs last (file order): the largest differences as shares of their bars, per kernel and tensor type."""
    path = os.environ.get("THETA_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            for key in sorted(WORST, key=str):
                f.write(f"gpu {' / '.join(str(k) for k in key)}: {WORST[key]:.3g}\n")
