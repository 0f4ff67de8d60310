"""Weighted means and variances of clouds far from zero, on every kernel that forms them, against the centred two-pass of the
reference (``cpu_ref.get_filter_mean_and_variance`` in float64; ``tests/forecast_oracle.forecast``), and ``pf_normalize`` /
``pf_loglik`` around the same tile edges.  Inputs: ``tests/moment_cases.py``; their conditions - the oracle resolves every case,
the raw one-pass formula does not - are asserted without a GPU in ``tests/test_moments_oracle_cpu.py``.

The variance's error is taken RELATIVE TO THE VARIANCE (a reference of exactly 0 must be met exactly), never to ``1 + |ref|``: a
cloud at level / spread = 1e6 has a variance 1e-12 of its second moment, and an error that is small against the second moment
is the whole of it.  Every test prints its worst figures before it asserts (``profiles/moments_parity.txt``).

Float32 bars of ``pf_forecast`` at a level (test 3): as in ``tests/test_forecast_gpu.py``, four times what ``oracle/models.py``
evaluated in float32 differs from its float64 self on exactly these inputs - per model and level, for the two means and the two
paths scaled by ``1 + |ref|`` and for the two variances relative to the variance (``tools/forecast_f32_bar.py cpu``, recorded in
``profiles/forecast.txt``):

    model       level   means      variances  paths
    lg1d        1e4     5.96e-08   2.17e-03   4.57e-07
    lg1d        1e6     5.93e-08   2.82e-01   2.54e-07
    ou_level    1e4     5.08e-08   1.90e-03   4.11e-07
    ou_level    1e6     8.31e-08   5.67e-01   2.73e-07
    rw2d_theta  1e4     9.48e-08   1.18e-03   3.92e-07
    rw2d_theta  1e6     5.05e-08   2.26e-01   3.44e-07

(A float32 particle at 1e6 is a multiple of 1/16 and a move of 0.05 mostly rounds away: float32 arithmetic itself leaves a
quarter to a half of such a cloud's variance undetermined, and the bar says so.  The float64 runs carry the weight there.)"""
import math

import pytest
import torch

from oracle import cpu_ref
from oracle.cases import CASE_BY_NAME, LEVEL_CASES
from pyfilter_amd.hints import HINTS
from tests import forecast_oracle as fo
from tests import moment_cases as mc
from tests.conftest import both_routes
from tests.helpers import DT, build_filter_from_case, load_golden
from tests.test_filters_gpu import _tols

pytestmark = pytest.mark.gpu

TDT = {"float64": torch.float64, "float32": torch.float32}
EPS64 = 2.0 ** -52


# ---- 1. pf_moments on the whole grid ---------------------------------------------------------------------------------------------
def _moments(c, dtype):
    from pyfilter_amd import ops

    mean, var = ops.moments_soa(ops.to_soa(c.x.to(dtype).cuda(), True, True), ops.to_cols(c.w.to(dtype).cuda()))
    return mean.cpu().double(), var.cpu().double()


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_moments_soa_at_every_level(dt):
    """f64: mean rtol 1e-12 / atol 1e-14 max|x|, variance rtol 1e-11; f32: 2e-6 relative on both (``test_gather_moments``' bars,
    the variance's relative to the variance) - at every ratio, N, D and kind of weights of the grid.  Variance >= 0 everywhere and
    exactly 0 for one particle of weight 1; a cloud of one value c: at most (16 eps |c|)^2; a NaN poisons its own component only."""
    dtype = TDT[dt]
    m_rtol, v_rtol = (1e-12, 1e-11) if dt == "float64" else (2e-6, 2e-6)
    worst, failures, ran = {}, [], 0
    for c in mc.cases():
        if dt not in c.dtypes:
            continue
        ran += 1
        mean, var = _moments(c, dtype)
        rm, rv = c.oracle()
        assert mean.shape == rm.shape == (c.b, c.d)
        keep = torch.ones_like(rm, dtype=torch.bool)
        if not c.finite:
            col, comp = c.nan_at
            keep[col, comp] = False
            if not bool(mean[col, comp].isnan() and var[col, comp].isnan()):
                failures.append((c.name, "the NaN component is not NaN", float(mean[col, comp]), float(var[col, comp])))
        xmax = float(c.x[~c.x.isnan()].abs().max())
        m_atol = 1e-14 * xmax if dt == "float64" else 0.0
        m_units = float(((mean - rm).abs()[keep] / (m_rtol * rm.abs()[keep] + m_atol + 1e-300)).max())
        m_rel = float(((mean - rm).abs()[keep] / (rm.abs()[keep] + 1e-2 * xmax + 1e-300)).max())
        if not bool((var[keep] >= 0).all()):
            failures.append((c.name, "negative variance", float(var[keep].min())))
        if c.equal is not None:
            v_err = float(var.max())
            if v_err > (16.0 * EPS64 * abs(c.equal)) ** 2:
                failures.append((c.name, "variance of a cloud of one value", v_err))
            v_rel = 0.0
        else:
            v_rel = mc.rel_err(var[keep], rv[keep])
            if c.single and not bool((var == 0).all()):
                failures.append((c.name, "single weight: variance not exactly 0", float(var.abs().max())))
            if not v_rel <= v_rtol:
                failures.append((c.name, "variance", v_rel))
        if not m_units <= 1.0:
            failures.append((c.name, "mean (units of its bar)", m_units))
        key = "nan" if not c.finite else ("equal" if c.equal is not None else f"{c.ratio:.0e}")
        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0)), (m_rel, v_rel)))
    for key, (m, v) in sorted(worst.items()):
        print(f"pf_moments {dt} ratio {key:6s}: worst mean error {m:.2e} (of |ref| + 1e-2 max|x|)   worst variance error {v:.2e} (relative)")
    print(f"pf_moments {dt}: {ran} cases, {len(failures)} failures")
    assert not failures, failures[:12]


# ---- 2. get_filter_mean_and_variance through its layouts -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["float64", "float32"])
@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("has_event", [True, False])
def test_get_filter_mean_and_variance_layouts_at_a_level(dt, batched, has_event):
    from pyfilter_amd.filters.particle.utils import get_filter_mean_and_variance
    from pyfilter_amd.timeseries import TimeseriesState

    c = next(c for c in mc.cases() if c.name == "r1e+06-N4100-B3-D2-cubed")
    x, w = c.x, c.w
    if not batched:
        x, w = x[:, 1], w[:, 1]
    if not has_event:
        x = x[..., 1]
    dtype = TDT[dt]
    state = TimeseriesState(0, x.to(dtype).cuda(), torch.Size([c.d]) if has_event else torch.Size([]))
    mean, var = get_filter_mean_and_variance(state, w.to(dtype).cuda())
    rm, rv = cpu_ref.get_filter_mean_and_variance(x, w, has_event)
    assert mean.shape == rm.shape and var.shape == rv.shape and mean.dtype == dtype
    m_rtol, v_rtol = (1e-12, 1e-11) if dt == "float64" else (2e-6, 2e-6)
    m_err, v_err = mc.rel_err(mean, rm), mc.rel_err(var, rv)
    print(f"get_filter_mean_and_variance {dt} batched={batched} event={has_event}: mean {m_err:.2e} variance {v_err:.2e}")
    assert m_err <= m_rtol and v_err <= v_rtol and bool((var >= 0).all())


# ---- 3. pf_forecast at a level ---------------------------------------------------------------------------------------------------
ORACLE_F32_ERR_AT_LEVEL = {  # (means, variances relative to the variance, paths): measured, module docstring
    ("lg1d", 1e4): (5.96e-08, 2.17e-03, 4.57e-07), ("lg1d", 1e6): (5.93e-08, 2.82e-01, 2.54e-07),
    ("ou_level", 1e4): (5.08e-08, 1.90e-03, 4.11e-07), ("ou_level", 1e6): (8.31e-08, 5.67e-01, 2.73e-07),
    ("rw2d_theta", 1e4): (9.48e-08, 1.18e-03, 3.92e-07), ("rw2d_theta", 1e6): (5.05e-08, 2.26e-01, 3.44e-07),
}


@pytest.mark.parametrize("level", fo.LEVELS)
@pytest.mark.parametrize("model", fo.LEVEL_MODELS)
def test_forecast_at_a_level_f64(model, level):
    """All four moment arrays within 1e-9 of the value itself (the means: plus the 1e-9 absolute of ``test_kernel_matches_oracle_f64``),
    paths at that test's bars; moments with and without paths bit-equal."""
    worst, failures = {k: 0.0 for k in fo.KEYS[:4]}, []
    for inp in fo.level_grid((model,), (level,)):
        got, ref = fo.run_kernel(inp), inp.reference()
        lean = fo.run_kernel(inp, paths=False)
        for k in fo.KEYS[:4]:
            assert got[k].shape == ref[k].shape, (inp, k)
            assert torch.equal(lean[k], got[k]), (inp, k)
            g, r = got[k].cpu(), ref[k]
            atol = 1e-9 if k.endswith("mean") else 0.0
            units = float(((g - r).abs() / (1e-9 * r.abs() + atol + 1e-300)).max())
            worst[k] = max(worst[k], fo.relative_error(g, r))
            if not units <= 1.0:
                failures.append((repr(inp), k, fo.relative_error(g, r)))
        for k in fo.KEYS[4:]:
            torch.testing.assert_close(got[k].cpu(), ref[k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{inp} {k}: {m}")
    print(f"pf_forecast float64 {model} level {level:.0e}: worst relative error " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not failures, failures[:8]


@pytest.mark.parametrize("level", fo.LEVELS)
@pytest.mark.parametrize("model", fo.LEVEL_MODELS)
def test_forecast_at_a_level_within_float32_bar(model, level):
    worst = (0.0, 0.0, 0.0)
    for inp in fo.level_grid((model,), (level,)):
        got = fo.run_kernel(inp, torch.float32)
        assert all(got[k].dtype == torch.float32 for k in fo.KEYS)
        worst = tuple(max(a, b) for a, b in zip(worst, fo.level_errors(got, inp.reference(torch.float32))))
        assert bool((got["x_var"] >= 0).all() and (got["y_var"] > 0).all()), inp
    bar = tuple(4.0 * v for v in ORACLE_F32_ERR_AT_LEVEL[(model, level)])
    print(f"pf_forecast float32 {model} level {level:.0e}: means {worst[0]:.2e} variances (relative) {worst[1]:.2e} paths {worst[2]:.2e}; "
          f"bars {bar[0]:.2e} {bar[1]:.2e} {bar[2]:.2e}")
    assert all(w <= b for w, b in zip(worst, bar))


# ---- 4. the same filter on every route, on reference runs at a level of 1e4 ----------------------------------------------------
LEVEL_PARAMS = [(c["name"], d) for c in LEVEL_CASES for d in c["dtypes"]]


def _compare_level_run(means, variance, ll, name, dt, what):
    """float64: the bars of ``tests/test_partial_nan_gpu.py: _compare_run`` (1e-9 / 1e-11 on values, 1e-8 on the variance - here
    relative to the variance alone).  float32: the bar of ``tests/test_filters_gpu.py: check_fused_batch_filter`` - each filter's
    whole run within 6 Monte-Carlo standard errors of the reference's float32 run or of its float64 run on the same draws - and for
    the variance, which that bar does not cover, 6 standard errors of a variance estimated from N draws, ``sqrt(2 / (N - 1))``
    relative (float32 trajectories part from the reference's after the first moved ancestor; what this excludes is a variance
    that cancelled: wrong by its own size or more, or clamped to 0)."""
    case = CASE_BY_NAME[name]
    g = load_golden(name, dt)
    means, variance, ll = means.cpu().double(), variance.cpu().double(), ll.cpu().double()
    assert means.shape == g["filter_means"].shape and variance.shape == g["filter_variance"].shape
    v_rel = mc.rel_err(variance, g["filter_variance"].double())
    m_rel = mc.rel_err(means, g["filter_means"].double())
    print(f"{what} {dt}: filter_means {m_rel:.2e}  filter_variance {v_rel:.2e} (relative)  "
          f"loglikelihood {float((ll - g['loglikelihood'].double()).abs().max()):.2e} (absolute)")
    if dt == "f64":
        tol = _tols("f64")
        torch.testing.assert_close(means, g["filter_means"], **tol)
        torch.testing.assert_close(variance, g["filter_variance"], rtol=tol["rtol"] * 10, atol=0.0)
        torch.testing.assert_close(ll, g["loglikelihood"], **tol)
        return
    n, t_len, b = case["N"], g["y"].shape[0], case["B"]
    ok = torch.zeros(b, dtype=torch.bool)
    for ref in (g, load_golden(name, "f64")):
        fm = ref["filter_means"].double().reshape(t_len + 1, b, -1)
        fv = ref["filter_variance"].double().reshape(fm.shape)
        se = (fv / n).sqrt()
        diff = (means.reshape(fm.shape) - fm).abs()
        dll = (ll.reshape(-1) - ref["loglikelihood"].double().reshape(-1)).abs()
        dv = (variance.reshape(fm.shape) - fv).abs()
        ok |= ((diff <= 6.0 * se + 1e-5 * fm.abs() + 1e-6).all(2).all(0) & (dll <= 0.05 * math.sqrt(t_len) + 1e-3)
               & (dv <= 6.0 * math.sqrt(2.0 / (n - 1)) * fv).all(2).all(0))
    assert bool((variance > 0).all())
    assert ok.all(), "a float32 filter is further than 6 standard errors from both of the reference's runs"


@both_routes
@pytest.mark.parametrize("name,dt", LEVEL_PARAMS)
def test_fused_routes_at_a_level(name, dt, kernel_route):
    g = load_golden(name, dt)
    filt = build_filter_from_case(CASE_BY_NAME[name], g, DT[dt], "cuda")
    res = filt.batch_filter(g["y"].cuda(), bar=False)
    _compare_level_run(res.filter_means, res.filter_variance, res.loglikelihood, name, dt, f"{name}/{kernel_route}")


@pytest.mark.parametrize("fused_step", [False, True])
@pytest.mark.parametrize("name,dt", LEVEL_PARAMS)
def test_step_by_step_routes_at_a_level(name, dt, fused_step, monkeypatch):
    """``filter()`` move by move, ``FilterResult.append`` taking ``pf_moments`` of every state: through the stand-alone primitives
    (``fused_step`` off) and through the fused single step."""
    monkeypatch.setattr(HINTS, "fused_step", fused_step)
    g = load_golden(name, dt)
    filt = build_filter_from_case(CASE_BY_NAME[name], g, DT[dt], "cuda")
    state = filt.initialize()
    result = filt.initialize_with_result(state)
    y = g["y"].cuda()
    for t in range(y.shape[0]):
        state = filt.filter(y[t], state, result=result)
    _compare_level_run(result.filter_means, result.filter_variance, result.loglikelihood, name, dt,
                       f"{name}/{'fused step' if fused_step else 'primitives'}")


# ---- 5. pf_normalize / pf_loglik at the tile edges -------------------------------------------------------------------------------
def _norm_cases():
    """Every kind at every N for B = 3; B = 1 and 300 at the N around a tile edge (300 columns of 70 001: tiles of 20 480)."""
    for kind in mc.LOGW_KINDS:
        for n in mc.N_ALL:
            for b in mc.NORM_B:
                if b == 3 or n in (1, 1025, 4100) or (b == 300 and n == 70001 and kind == "range"):
                    yield kind, n, b


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_normalize_and_ess_at_tile_edges(dt):
    """W, ESS and the in-place sanitising (exact) against ``cpu_ref.normalize`` / ``get_ess`` in float64 on the same rounded
    log-weights; bars of ``test_normalize_and_systematic_vs_reference_golden``: f64 1e-12; f32 5e-5 on W, 2e-4 on ESS."""
    import pyfilter_amd as pf

    dtype = TDT[dt]
    w_tol = dict(rtol=1e-12, atol=1e-300) if dt == "float64" else dict(rtol=5e-5, atol=1e-38)
    e_rtol = 1e-12 if dt == "float64" else 2e-4
    worst_w = worst_e = 0.0
    for kind, n, b in _norm_cases():
        lw = mc.logw(kind, n, b, dtype)
        what = f"{kind} N={n} B={b}"
        ref_in = lw.clone()
        cpu_ref.normalize(ref_in)  # (in place, in the dtype under test: nan_to_num_'s lowest finite value is the dtype's)
        ref_w = cpu_ref.normalize(lw.clone().double())
        ref_ess = cpu_ref.get_ess(lw.clone().double())
        dev = lw.clone().cuda()
        W = pf.utils.normalize(dev)
        assert torch.equal(dev.cpu(), ref_in), f"{what}: in-place sanitising"
        assert W.shape == (n, b) and W.dtype == dtype
        torch.testing.assert_close(W.cpu().double(), ref_w, equal_nan=True, msg=lambda m: f"{what} W: {m}", **w_tol)
        ess = pf.utils.get_ess(lw.clone().cuda())
        torch.testing.assert_close(ess.cpu().double(), ref_ess, rtol=e_rtol, atol=0, equal_nan=True, msg=lambda m: f"{what} ESS: {m}")
        fin = ref_w > (1e-290 if dt == "float64" else 1e-30)
        worst_w = max(worst_w, float(((W.cpu().double() - ref_w).abs()[fin] / ref_w[fin]).max()))
        worst_e = max(worst_e, mc.rel_err(ess, ref_ess))
    print(f"pf_normalize {dt}: worst relative error W {worst_w:.2e}  ESS {worst_e:.2e}")


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_log_likelihood_at_tile_edges(dt):
    """``log_likelihood(v)`` and ``log_likelihood(v, W)`` against ``cpu_ref.log_likelihood`` in float64 on the same rounded inputs
    (f64 1e-12; f32 rtol 1e-5 / atol 1e-6); a NaN in ``v`` and an all -inf column: what the reference returns there (NaN)."""
    from pyfilter_amd.filters.particle.utils import log_likelihood

    dtype = TDT[dt]
    tol = dict(rtol=1e-12, atol=1e-12) if dt == "float64" else dict(rtol=1e-5, atol=1e-6)
    worst = 0.0
    for kind in mc.LOGLIK_KINDS:
        for n in mc.N_ALL:
            for b in mc.NORM_B:
                if not (b == 3 or n in (1, 1025, 4100) or (b == 300 and n == 70001 and kind == "max_last_tile")):
                    continue
                v, w = mc.loglik_inputs(kind, n, b, dtype)
                what = f"{kind} N={n} B={b}"
                for W in (None, w):
                    ref = cpu_ref.log_likelihood(v.double(), None if W is None else W.double())
                    got = log_likelihood(v.cuda(), None if W is None else W.cuda()).cpu().double()
                    assert got.shape == ref.shape
                    torch.testing.assert_close(got, ref, equal_nan=True, msg=lambda m: f"{what} W={'given' if W is not None else '1/N'}: {m}", **tol)
                    fin = ref.isfinite()
                    if bool(fin.any()):
                        worst = max(worst, float(((got - ref).abs()[fin] / (1.0 + ref.abs()[fin])).max()))
    print(f"pf_loglik {dt}: worst error / (1 + |ref|) {worst:.2e}")
