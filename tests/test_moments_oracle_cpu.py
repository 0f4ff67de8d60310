"""Without a GPU: the input conditions of ``tests/test_moments_parity_gpu.py`` on exactly its inputs (``tests/moment_cases.py``), and
the two torch-route formulas that compute a variance of a cloud far from zero.

1. The float64 oracle (``cpu_ref.get_filter_mean_and_variance``: centre, then square) resolves every finite case of the grid to
   1e-12 relative of an extended-precision two-pass - so no GPU case needs excusing for the oracle's sake.
2. A plain float64 restatement of the raw one-pass formula ``S2 - 2 mu S1 + mu^2 S0`` MISSES the GPU test's float64 variance bar
   on the cases at level / spread >= 1e4: the grid can see the bug it was written for.  (About the restatement, not the library.)
3. ``_weighted`` (through ``torch_forecast`` of a user-lambda AR(1)) and ``mix_forecasts`` on CPU tensors at a level of 1e6
   against a two-pass.
4. The golden runs at a level (``oracle/cases.py: LEVEL_CASES``) sit at level / spread >= 1e5 at every recorded step."""
import math

import numpy as np
import pytest
import torch

from oracle.cases import LEVEL_CASES
from tests import moment_cases as mc
from tests.helpers import load_golden

F64_VAR_RTOL = 1e-11  # the GPU test's float64 variance bar
HAVE_EXTENDED = np.finfo(np.longdouble).eps < 1e-18


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    zero = ref == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - ref)[~zero] / np.abs(ref)[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.skipif(not HAVE_EXTENDED, reason="numpy's longdouble is no wider than float64 on this machine")
def test_oracle_resolves_every_finite_case():
    worst = {}
    for c in mc.cases():
        if not c.finite:
            continue
        mean, var = c.oracle()
        lm, lv = mc.two_pass_longdouble(c.x, c.w)
        if c.equal is not None:  # one value: the exact variance is (sum W - 1)^2 c^2-small; what the oracle's two-pass leaves is bounded
            assert bool((var >= 0).all()) and float(var.max()) <= (16.0 * 2.0 ** -52 * abs(c.equal)) ** 2, c
            assert _rel(mean.numpy(), lm) <= 1e-12, c
            continue
        em, ev = _rel(mean.numpy(), lm), _rel(var.numpy(), lv)
        assert em <= 1e-12 and ev <= 1e-12, (c, em, ev)
        worst[c.ratio] = max(worst.get(c.ratio, 0.0), em, ev)
    print("worst relative error of the float64 oracle against extended precision, per ratio:", worst)


def test_grid_covers_the_axes():
    cs = [c for c in mc.cases() if c.equal is None and c.finite]
    assert {c.n for c in cs} >= set(mc.N_ALL) and {c.d for c in cs} >= set(mc.D_ALL) and {c.b for c in cs} >= set(mc.B_ALL)
    assert {c.ratio for c in cs} >= set(mc.RATIOS) | {mc.RATIO_F64_ONLY}
    for kind in mc.WEIGHTS:
        assert any(c.name.endswith("-" + kind) for c in cs), kind
    assert all(("float32" in c.dtypes) == (c.ratio != mc.RATIO_F64_ONLY and c.equal != 123456789.125) for c in mc.cases())
    # float32 cases hold numbers float32 holds
    for c in mc.cases():
        if "float32" in c.dtypes:
            fin = ~c.x.isnan()
            assert torch.equal(c.x[fin].float().double(), c.x[fin]) and torch.equal(c.w.float().double(), c.w), c
    half = next(c for c in cs if c.name.endswith("sum_half"))
    assert bool(((half.w.sum(0) - 0.5).abs() < 1e-6).all())
    assert mc.tile_elems(4100, 3) == 1024 and mc.last_tile_start(4100, 3) == 4096 and mc.last_tile_start(70001, 3) == 69632
    assert mc.tile_elems(70001, 300) == 80 * 256


def test_raw_one_pass_formula_misses_the_float64_bar():
    """Every case at level / spread >= 1e4 with more than two weighted particles: the raw formula is off by more than the
    float64 variance bar.  (Left out: the single-weight cases, which cancel exactly - ``x^2 - 2 x^2 + x^2``; and weights summing to
    0.5, whose mean is half the level, so that the variance about it is of the order of level^2 and loses nothing.)"""
    seen = 0
    for c in mc.cases():
        if not c.finite or c.equal is not None or c.single or c.n < 7 or c.ratio < 1e4 or c.name.endswith("sum_half"):
            continue
        _, var = c.oracle()
        _, raw = mc.raw_one_pass(c.x, c.w)
        err = mc.rel_err(raw, var)
        assert err > F64_VAR_RTOL, (c, err)
        seen += 1
    assert seen >= 50
    # ... and at ratio 0 the same formula is fine: the grid does not fail everything
    for c in mc.cases():
        if c.finite and c.equal is None and c.ratio == 0.0 and c.n >= 7:
            assert mc.rel_err(mc.raw_one_pass(c.x, c.w)[1], c.oracle()[1]) <= F64_VAR_RTOL, c


def test_nan_cases_poison_one_component_in_the_oracle():
    for c in mc.cases():
        if c.finite:
            continue
        mean, var = c.oracle()
        col, comp = c.nan_at
        assert bool(mean[col, comp].isnan() and var[col, comp].isnan()), c
        keep = torch.ones_like(mean, dtype=torch.bool)
        keep[col, comp] = False
        assert bool(mean[keep].isfinite().all() and var[keep].isfinite().all() and (var[keep] > 0).all()), c


# ---- the torch-route formulas -------------------------------------------------------------------------------------------------
def test_torch_forecast_of_a_user_model_at_a_level():
    """A user-lambda AR(1) ``x' = 0.99 x + 1e4 + 0.05 e`` (fixed point 1e6) under ``y = x + 0.15 v``, the cloud at 1e6 with spread
    1e-3 .. : the torch route's moments against the two-pass oracle formulas on the same moves."""
    from torch.distributions import Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle.forecast import torch_forecast

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    n, b, h = 1000, 3, 4
    gen = torch.Generator().manual_seed(5)
    x = 1e6 + 0.05 * torch.randn(n, b, generator=gen, dtype=torch.float32).double()
    w = torch.softmax(torch.randn(n, b, generator=gen, dtype=torch.float64), 0)
    z = torch.randn(h, n, b, generator=gen, dtype=torch.float64)
    hidden = ts.AffineProcess(lambda s, a, be, sg: (a + be * s.value, sg), (t(1e4), t(0.99), t(0.05)), Normal(t(0.0), t(1.0)),
                              initial_kernel=lambda a, be, sg: Normal(a / (1.0 - be), sg))
    ssm = ts.LinearStateSpaceModel(hidden, (t(1.0), t(0.15)))
    fc = torch_forecast(ssm, ts.TimeseriesState(0, x, torch.Size([])), w, h, False, z, None, 0)
    cur = x
    for k in range(h):
        cur = 1e4 + 0.99 * cur + 0.05 * z[k]
        mean = (w * cur).sum(0)
        var = (w * (cur - mean) ** 2).sum(0)
        torch.testing.assert_close(fc.x_mean[k], mean, rtol=1e-12, atol=0)
        torch.testing.assert_close(fc.x_variance[k], var, rtol=1e-10, atol=0)
        torch.testing.assert_close(fc.y_mean[k], mean, rtol=1e-12, atol=0)
        torch.testing.assert_close(fc.y_variance[k], var + 0.15 ** 2, rtol=1e-10, atol=0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_mix_forecasts_at_a_level(dtype):
    """Member means at 1e6 with spread 1e-3 and member variances 1e-6: ``sum w (v + (m - mu)^2)`` to 1e-10 (float32 members: the
    same numbers rounded, the result within float32's rounding of the two-pass on them)."""
    from pyfilter_amd.filters.particle import Forecast, mix_forecasts

    gen = torch.Generator().manual_seed(8)
    steps, b = 3, 64
    m = (1e6 + 1e-3 * torch.randn(steps, b, generator=gen, dtype=torch.float64)).to(dtype)
    v = (1e-6 * (0.5 + torch.rand(steps, b, generator=gen, dtype=torch.float64))).to(dtype)
    w = torch.softmax(torch.randn(b, generator=gen, dtype=torch.float64), 0)
    mixed = mix_forecasts(w, Forecast(m, v, -m, 2.0 * v))
    md, vd = m.double(), v.double()
    mu = (w * md).sum(1)
    want = (w * (vd + (md - mu[:, None]) ** 2)).sum(1)
    want_y = (w * (2.0 * vd + (md - mu[:, None]) ** 2)).sum(1)
    rtol = 1e-10 if dtype == torch.float64 else 2.0 ** -23
    torch.testing.assert_close(mixed.x_mean.double(), mu, rtol=1e-12 if dtype == torch.float64 else 2.0 ** -23, atol=0)
    torch.testing.assert_close(mixed.x_variance.double(), want, rtol=rtol, atol=0)
    torch.testing.assert_close(mixed.y_mean.double(), -mu, rtol=1e-12 if dtype == torch.float64 else 2.0 ** -23, atol=0)
    torch.testing.assert_close(mixed.y_variance.double(), want_y, rtol=rtol, atol=0)
    assert mixed.x_variance.dtype == dtype


# ---- the golden runs at a level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", [(c["name"], d) for c in LEVEL_CASES for d in c["dtypes"]])
def test_level_fixtures_sit_at_their_level(name, dt):
    g = load_golden(name, dt)
    mean, var = g["filter_means"].double(), g["filter_variance"].double()
    assert bool((var > 0).all())
    ratio = mean.abs() / var.sqrt()
    print(f"{name}/{dt}: level / spread over the recorded steps {float(ratio.min()):.3g} .. {float(ratio.max()):.3g}")
    assert float(ratio.min()) >= 1e5
    assert {c["filter"] + "+" + c["proposal"] for c in LEVEL_CASES} == {"sisr+bootstrap", "apf+lgo"}
    assert math.isfinite(float(g["loglikelihood"].sum()))
