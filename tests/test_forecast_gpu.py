"""Forecasting on the GPU: ``pf_forecast`` (``csrc/pf_forecast.hpp``) against the float64 oracle (``tests/forecast_oracle.py``) on
tapes, its own Philox draws, ``ParticleFilter.forecast`` end to end, the routing, and the posterior predictive of SMC2 / NESS.

Float32 bar (test 2): the scaled error ``max |d| / (1 + |ref|)`` against the float64 oracle on the same rounded inputs may be at
most four times what ``oracle/models.py`` evaluated in float32 differs from its float64 self on exactly those inputs - per
model, for the four moment arrays and for the two paths (``tools/forecast_f32_bar.py cpu``, recorded in ``profiles/forecast.txt``):

    model        moments    paths
    lg1d         2.81e-09   8.38e-08
    sine         4.70e-08   3.88e-07
    sv_batched   3.67e-08   3.11e-07
    ou_batched   1.82e-08   2.01e-07
    rw2d_theta   1.47e-08   1.49e-07
    lorenz_o1    3.03e-07   3.02e-06
    lorenz_o3    3.94e-07   1.85e-06

Four times is the margin the nested proposal's float32 bar uses (``tests/test_nested_gpu.py``)."""
import math

import pytest
import torch

from oracle import models as M
from oracle.cases import CASE_BY_NAME, build_spec
from tests import forecast_oracle as fo
from tests.helpers import build_filter_from_case, build_ssm_from_case, load_golden

pytestmark = pytest.mark.gpu

ORACLE_F32_ERR = {  # (moments, paths): measured, module docstring
    "lg1d": (2.81e-09, 8.38e-08), "sine": (4.70e-08, 3.88e-07), "sv_batched": (3.67e-08, 3.11e-07), "ou_batched": (1.82e-08, 2.01e-07),
    "rw2d_theta": (1.47e-08, 1.49e-07), "lorenz_o1": (3.03e-07, 3.02e-06), "lorenz_o3": (3.94e-07, 1.85e-06),
}
F32_BAR = {k: (4.0 * v[0], 4.0 * v[1]) for k, v in ORACLE_F32_ERR.items()}


# ---- 1. taped, float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", fo.GPU_MODELS)
def test_kernel_matches_oracle_f64(model):
    for inp in fo.grid((model,)):
        got, ref = fo.run_kernel(inp), inp.reference()
        for k in fo.KEYS:
            assert got[k].shape == ref[k].shape, (inp, k)
            torch.testing.assert_close(got[k].cpu(), ref[k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{inp} {k}: {m}")


# ---- 2. taped, float32 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", fo.GPU_MODELS)
def test_kernel_within_float32_bar(model):
    worst = (0.0, 0.0)
    for inp in fo.grid((model,), torch.float32):
        got = fo.run_kernel(inp, torch.float32)
        assert all(got[k].dtype == torch.float32 for k in fo.KEYS)
        worst = tuple(max(a, b) for a, b in zip(worst, fo.errors(got, inp.reference(torch.float32))))
    print(f"{model}: float32 scaled error moments {worst[0]:.2e} paths {worst[1]:.2e}; bars {F32_BAR[model][0]:.2e} {F32_BAR[model][1]:.2e}")
    assert worst[0] <= F32_BAR[model][0] and worst[1] <= F32_BAR[model][1]


# ---- 3. own Philox draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,n,b", [("sine", 5003, 3), ("rw2d_theta", 200, 4), ("lorenz_o3", 1000, 1)])
def test_philox_draws_are_a_function_of_the_seed(model, n, b, dtype):
    inp = fo.Inputs(model, n, b, 4, "random")
    a, again, other = (fo.run_kernel(inp, dtype, tapes=False, seed=s) for s in (21, 21, 22))
    for k in fo.KEYS:
        assert torch.equal(a[k], again[k]), k
    assert not torch.equal(a["x_path"], other["x_path"]) and not torch.equal(a["y_path"], other["y_path"])
    assert not torch.equal(a["x_mean"], other["x_mean"])


@pytest.mark.parametrize("model,n,b", [("sine", 5003, 3), ("rw2d_theta", 200, 4), ("sv_batched", 1000, 1)])
def test_moments_with_and_without_paths_and_against_pf_moments(model, n, b):
    from pyfilter_amd import ops

    inp = fo.Inputs(model, n, b, 5, "random")
    lean = fo.run_kernel(inp, paths=False, tapes=False, seed=33)
    full = fo.run_kernel(inp, paths=True, tapes=False, seed=33)
    assert lean["x_path"] is None and lean["y_path"] is None
    for k in fo.KEYS[:4]:
        assert torch.equal(lean[k], full[k]), k
    W = ops.to_cols(inp.w.cuda())
    for h in range(inp.h):
        mean, var = ops.moments_soa(ops.to_soa(full["x_path"][h].contiguous(), True, inp.has_d), W)  # (B, D)
        for got, ref in ((full["x_mean"][h], mean), (full["x_var"][h], var)):
            torch.testing.assert_close(got.reshape(ref.shape), ref, rtol=1e-12, atol=1e-12)


def test_philox_forecast_of_the_ar1_within_monte_carlo_error():
    """lg1d: ``x' = 0.99 x + 0.05 e``.  Given the cloud, ``x_mean_h = sum W_i (0.99^h x_i + noise_ih)`` with independent
    ``noise_ih ~ N(0, v_h)``, ``v_h = 0.05^2 (1 - 0.99^(2h)) / (1 - 0.99^2)``: its expectation is the closed form
    ``0.99^h sum W x``, its standard error ``sqrt(v_h sum W^2)`` - derived, not measured."""
    beta, sigma = 0.99, 0.05
    inp = fo.Inputs("lg1d", 65536, 2, 5, "random")
    got = fo.run_kernel(inp, paths=False, tapes=False, seed=5)
    w = inp.w
    hs = torch.arange(1, 6, dtype=torch.float64)
    exact = (beta ** hs)[:, None] * (w * inp.x).sum(0)
    se = (sigma ** 2 * (1 - beta ** (2 * hs)) / (1 - beta ** 2))[:, None].sqrt() * (w * w).sum(0).sqrt()
    dev = (got["x_mean"].cpu() - exact).abs() / se
    print("deviations in standard errors:", dev.flatten().tolist())
    assert bool((dev < 6.0).all())


@pytest.mark.parametrize("model,n,b", [("sv_batched", 20000, 4), ("lorenz_o3", 20000, 2)])
def test_observation_noise_of_the_paths_is_standard_normal(model, n, b):
    inp = fo.Inputs(model, n, b, 3, "none")
    got = fo.run_kernel(inp, paths=True, tapes=False, seed=77)
    x, y = got["x_path"].cpu(), got["y_path"].cpu()
    m, s = M.obs_loc_scale(fo.rounded_spec(inp.case, torch.float64), x)
    r = ((y - m) / M._t(s, m)).flatten()
    k = r.numel()
    # mean of k standard normals: standard error 1 / sqrt(k); their sample variance: sqrt(2 / k)
    assert abs(float(r.mean())) < 6.0 / math.sqrt(k)
    assert abs(float(r.var()) - 1.0) < 6.0 * math.sqrt(2.0 / k)


# ---- 4. filt.forecast end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sine_apf_lgo", "lorenz_sisr_boot"])
def test_filter_forecast_shapes_and_untouched_run(name):
    from pyfilter_amd.filters.particle import APF, SISR, Forecast

    case = CASE_BY_NAME[name]
    g = load_golden(name, "f64")
    y = g["y"].cuda()
    spec = build_spec(case)
    d_tail = (spec.dim,) if spec.dim > 0 else ()
    o_tail = (spec.obs_dim,) if spec.obs_dim > 0 else ()
    n, b, steps = case["N"], case["B"], 7

    def run(with_forecast):
        filt = build_filter_from_case(case, g, torch.float64, "cuda", tape=False, seed=17)
        state, fc = filt.initialize(), None
        for t in range(10):
            state = filt.filter(y[t], state)
            if with_forecast and t == 4:
                before = state.weights.clone()
                fc = filt.forecast(state, steps, paths=True)
                lean = filt.forecast(state, steps, seed=3)
                assert torch.equal(before, state.weights)
                assert lean.paths is None
        torch.cuda.synchronize()
        return state, fc

    plain, _ = run(False)
    forecasting, fc = run(True)
    assert torch.equal(plain.timeseries_state.value, forecasting.timeseries_state.value)
    assert torch.equal(plain.weights, forecasting.weights)
    assert torch.equal(plain.get_loglikelihood(), forecasting.get_loglikelihood())

    assert isinstance(fc, Forecast)
    assert fc.x_mean.shape == fc.x_variance.shape == (steps, b) + d_tail
    assert fc.y_mean.shape == fc.y_variance.shape == (steps, b) + o_tail
    xp, yp = fc.paths.get_paths()
    assert xp.shape == (steps, n, b) + d_tail and yp.shape == (steps, n, b) + o_tail
    assert bool(torch.isfinite(fc.x_mean).all() and torch.isfinite(fc.y_variance).all() and (fc.x_variance > 0).all())
    # a FilterResult stands for its latest state; the same seed gives the same forecast
    filt = build_filter_from_case(case, g, torch.float64, "cuda", tape=False, seed=17)
    res = filt.batch_filter(y[:5], bar=False)
    a, c = filt.forecast(res, steps, seed=9), filt.forecast(res.latest_state, steps, seed=9)
    assert torch.equal(a.x_mean, c.x_mean) and torch.equal(a.y_variance, c.y_variance)

    # without the batch dimension
    ssm = build_ssm_from_case(dict(case, B=1), torch.float64, "cuda")
    solo = {"sisr": SISR, "apf": APF}[case["filter"]](ssm, n, seed=4)
    res = solo.batch_filter(y[:5, 0] if y.dim() > 1 + len(o_tail) else y[:5], bar=False)
    fc = solo.forecast(res, 3, paths=True)
    assert fc.x_mean.shape == (3,) + d_tail and fc.y_variance.shape == (3,) + o_tail
    xp, yp = fc.paths.get_paths()
    assert xp.shape == (3, n) + d_tail and yp.shape == (3, n) + o_tail


# ---- 5. routing --------------------------------------------------------------------------------------------------------------------
def test_user_lambda_model_takes_the_torch_route_and_agrees_with_the_kernel(monkeypatch):
    from torch.distributions import Normal

    from pyfilter_amd import ops, timeseries as ts
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.timeseries import models

    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")  # noqa: E731
    dt = 0.1
    user = ts.AffineEulerMaruyama(lambda x, gamma, sigma: (torch.sin(x.value - gamma), sigma), (t(0.0), t(1.0)), Normal(t(0.0), t(math.sqrt(dt))),
                                  dt=dt, initial_kernel=lambda gamma, sigma: Normal(torch.zeros_like(gamma), torch.ones_like(gamma)))
    ssm_user = ts.LinearStateSpaceModel(user, (t(1.0), t(0.1)))
    ssm_builtin = ts.LinearStateSpaceModel(models.SineDiffusion(t(0.0), t(1.0), dt=dt), (t(1.0), t(0.1)))
    inp = fo.Inputs("sine", 1000, 3, 6, "random")
    calls = []
    real = ops.forecast_soa
    monkeypatch.setattr(ops, "forecast_soa", lambda *a, **k: calls.append(1) or real(*a, **k))
    out = []
    for ssm in (ssm_user, ssm_builtin):
        filt = SISR(ssm, inp.n, seed=2)
        filt.set_batch_shape(torch.Size([inp.b]))
        state = filt.initialize()
        state["_x"] = state["_x"].copy(values=inp.x.cuda())
        state["_w"] = inp.w.log().cuda()
        out.append(fo.as_dict(filt.forecast(state, inp.h, paths=True, z=inp.z.cuda(), e=inp.e.cuda())))
        assert len(calls) == (0 if ssm is ssm_user else 1)
    for k in fo.KEYS:
        torch.testing.assert_close(out[0][k], out[1][k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{k}: {m}")


def test_linear_model_runs_on_the_torch_route():
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.timeseries.models import LinearModel

    d, o, n, b = 4, 2, 300, 2
    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")  # noqa: E731
    inc = Independent(Normal(t(0.0), t(1.0)).expand(torch.Size([d])), 1)
    hidden = LinearModel((0.9 * torch.eye(d, dtype=torch.float64, device="cuda"), t([0.1] * d)), inc,
                         lambda *_: Independent(Normal(torch.zeros(d, dtype=torch.float64, device="cuda"), torch.ones(d, dtype=torch.float64, device="cuda")), 1))
    a_obs = torch.ones((o, d), dtype=torch.float64, device="cuda")
    filt = SISR(ts.LinearStateSpaceModel(hidden, (a_obs, t([0.2] * o)), torch.Size([o])), n, seed=1)
    filt.set_batch_shape(torch.Size([b]))
    fc = filt.forecast(filt.initialize(), 3, paths=True)
    assert fc.x_mean.shape == fc.x_variance.shape == (3, b, d) and fc.y_mean.shape == fc.y_variance.shape == (3, b, o)
    xp, yp = fc.paths.get_paths()
    assert xp.shape == (3, n, b, d) and yp.shape == (3, n, b, o)
    assert bool(torch.isfinite(fc.x_variance).all() and torch.isfinite(fc.y_variance).all())


def test_unsupported_shapes_are_invalid_arguments():
    from pyfilter_amd import _lib as L, ops
    from pyfilter_amd.timeseries import KernelKind

    def kind(hid, d, o):
        k = KernelKind(hid, d, 1.0, 1.0)
        k.obs_kind, k.obs_dim = L.OBS_LINEAR, o
        return k

    n, b = 64, 2
    for hid, d, o, steps in ((L.HID_LINEAR, 4, 2, 3), (L.HID_LINEAR, 2, 4, 3), (L.HID_LINEAR_MAT, 2, 2, 3), (L.HID_USER_AFFINE, 2, 2, 3),
                             (L.HID_LINEAR, 2, 2, 0)):
        x = torch.zeros((d, b, n), dtype=torch.float64, device="cuda")
        params = torch.ones((b, 4 * d + d * d + o * d + 2 * o + 2 * d), dtype=torch.float64, device="cuda")
        with pytest.raises(L.PfAmdError, match=r"pf_forecast failed: invalid argument \(code -1\)"):
            ops.forecast_soa(kind(hid, d, o), params, steps, x, None)
    torch.cuda.synchronize()


# ---- 6. SMC2 / NESS ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg_name", ["smc2", "ness"])
def test_posterior_predictive_is_the_mixture_of_the_filters_forecasts(alg_name):
    from torch.distributions import Exponential, LogNormal, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import APF, mix_forecasts
    from pyfilter_amd.inference import NESS, SMC2
    from pyfilter_amd.inference.utils import theta_normalize
    from pyfilter_amd.timeseries import models

    dev, dt = torch.device("cuda"), torch.float64
    g = torch.Generator().manual_seed(3)
    y = (0.05 * torch.randn(12, generator=g, dtype=dt)).cumsum(0).to(dev)
    priors = {"kappa": Exponential(10.0), "gamma": Normal(0.0, 1.0), "sigma": LogNormal(-2.0, 1.0)}
    obs = (torch.tensor(1.0, device=dev, dtype=dt), torch.tensor(0.05, device=dev, dtype=dt))
    filt = APF(lambda th: ts.LinearStateSpaceModel(models.OrnsteinUhlenbeck(th["kappa"], th["gamma"], th["sigma"], dt=1.0), obs), 128, seed=5)
    alg = (SMC2(filt, 8, priors, threshold=0.5, device=dev, dtype=dt, seed=9) if alg_name == "smc2"
           else NESS(filt, 8, priors, device=dev, dtype=dt, seed=9))
    state = alg.initialize()
    for t in range(y.shape[0]):
        state = alg.step(y[t], state)
    fc = alg.forecast(state, 4, seed=31)
    ref = mix_forecasts(theta_normalize(state.w), alg.filter.forecast(state.filter_state, 4, seed=31))
    for got, want in ((fc.x_mean, ref.x_mean), (fc.x_variance, ref.x_variance), (fc.y_mean, ref.y_mean), (fc.y_variance, ref.y_variance)):
        assert got.shape == (4,) and torch.equal(got, want)
    assert fc.paths is None and bool(torch.isfinite(fc.y_variance).all() and (fc.y_variance > 0).all())
