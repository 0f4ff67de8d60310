"""Forecasting without a GPU: the oracle (``tests/forecast_oracle.py``) against the AR(1)'s closed form, the package's torch route
against the oracle on tapes, ``mix_forecasts`` against hand numbers, and the C ABI's declarations."""
import os

import pytest
import torch

from tests import forecast_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ar1_closed_form(x, w, h_max, alpha=0.0, beta=0.99, sigma=0.05):
    """The exact h-step predictive law of ``x' = alpha + beta x + sigma e`` from the cloud ``(x_i, W_i)``, ``sum W = 1``:

        mean_h = sum_i W_i (beta^h x_i + alpha (1 - beta^h) / (1 - beta))
        var_h  = beta^(2h) sum_i W_i (x_i - mean_0)^2  +  sigma^2 (1 - beta^(2h)) / (1 - beta^2)

    returned as (mean (H, B), variance of the cloud's image (H, B), the noise term (H,)) for h = 1 .. h_max."""
    mean0 = (w * x).sum(0)
    var0 = (w * (x - mean0) ** 2).sum(0)
    hs = torch.arange(1, h_max + 1, dtype=torch.float64)
    bh = beta ** hs
    mean = bh[:, None] * mean0 + (alpha * (1 - bh) / (1 - beta))[:, None]
    return mean, (bh ** 2)[:, None] * var0, sigma ** 2 * (1 - bh ** 2) / (1 - beta ** 2)


def test_oracle_matches_the_ar1_closed_form():
    inp = fo.Inputs("lg1d", 400, 2, 6, "random")
    spec = fo.build_spec(inp.case, torch.float64)
    w = inp.w / inp.w.sum(0)  # (the inputs' weights are rounded to float32: the closed form is stated for sum W = 1)
    ref = fo.forecast(spec, inp.x, w, torch.zeros_like(inp.z))  # a tape of zeros: every particle follows its conditional mean
    mean, var_cloud, noise = ar1_closed_form(inp.x, w, inp.h)
    torch.testing.assert_close(ref["x_mean"], mean, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ref["x_var"], var_cloud, rtol=1e-10, atol=1e-16)
    # ... so the exact predictive variance is the oracle's on the zero tape plus the known noise term; and y = x + 0.15 v
    torch.testing.assert_close(ref["y_mean"], mean, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ref["y_var"], var_cloud + 0.15 ** 2, rtol=1e-10, atol=1e-16)
    # on real draws the oracle's variance estimates var_cloud + noise: N = 400 x 2 particles, a loose sanity band of 25 %
    drawn = fo.forecast(spec, inp.x, w, inp.z)
    assert bool(((drawn["x_var"] / (var_cloud + noise[:, None]) - 1.0).abs() < 0.25).all())


@pytest.mark.parametrize("model", fo.CPU_MODELS)
def test_torch_route_matches_oracle_on_cpu(model):
    for (n, b), h, weights in (((300, 1), 1, "none"), ((257, 3), 5, "random"), ((200, 4), 3, "half_zero")):
        inp = fo.Inputs(model, n, b, h, weights)
        got, ref = fo.torch_route(inp), inp.reference()
        for k in fo.KEYS:
            assert got[k].shape == ref[k].shape, (inp, k)
            torch.testing.assert_close(got[k], ref[k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{inp} {k}: {m}")


def test_torch_route_without_paths_and_without_tapes():
    inp = fo.Inputs("sine", 300, 2, 4, "random")
    a = fo.torch_route(inp, paths=False, tapes=False, seed=5)
    b = fo.torch_route(inp, paths=True, tapes=False, seed=5)
    c = fo.torch_route(inp, paths=False, tapes=False, seed=6)
    assert a["x_path"] is None and a["y_path"] is None
    for k in fo.KEYS[:4]:
        assert torch.equal(a[k], b[k]), k  # the same seed: the same x with or without paths
    assert not torch.equal(a["x_mean"], c["x_mean"])


def test_mix_forecasts_hand_numbers():
    from pyfilter_amd.filters.particle import Forecast, mix_forecasts

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    # one step, two filters, scalar state and observation: weights 1/4, 3/4
    fc = Forecast(t([[1.0, 3.0]]), t([[0.5, 0.25]]), t([[2.0, -2.0]]), t([[1.0, 1.0]]))
    mixed = mix_forecasts(t([0.25, 0.75]), fc)
    # mean = 0.25 * 1 + 0.75 * 3 = 2.5; second moment = 0.25 * (0.5 + 1) + 0.75 * (0.25 + 9) = 7.3125; var = 7.3125 - 6.25
    torch.testing.assert_close(mixed.x_mean, t([2.5]))
    torch.testing.assert_close(mixed.x_variance, t([1.0625]))
    # mean = 0.5 - 1.5 = -1; second moment = 0.25 * 5 + 0.75 * 5 = 5; var = 4
    torch.testing.assert_close(mixed.y_mean, t([-1.0]))
    torch.testing.assert_close(mixed.y_variance, t([4.0]))
    # a vector state keeps its last dimension: (steps, B, D) -> (steps, D)
    fc3 = Forecast(torch.ones(2, 2, 3, dtype=torch.float64), torch.zeros(2, 2, 3, dtype=torch.float64), t([[2.0, -2.0]] * 2), t([[1.0, 1.0]] * 2))
    assert mix_forecasts(t([0.5, 0.5]), fc3).x_mean.shape == (2, 3)
    assert mixed.paths is None


def test_c_abi_declares_pf_forecast():
    from pyfilter_amd import _lib

    assert "pf_forecast" in _lib.EXPORTS and "pf_forecast_workspace_bytes" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "pf_amd.h")) as f:
        header = f.read()
    assert "int pf_forecast(const pf_model* model, int steps," in header
    assert "int pf_forecast_workspace_bytes(" in header
    assert "#define PF_ABI_VERSION 4" in header


@pytest.mark.parametrize("model", ["lg1d_o2", "lorenz", "sine"])
def test_filter_forecast_on_cpu_tensors_takes_the_torch_route(model):
    """``ParticleFilter.forecast`` without a GPU: the state's log-weights are normalised (a copy: the state keeps its own), the
    filter's draw counter does not move, two calls without a seed draw different numbers."""
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.filters.particle.forecast import normalized_weights
    from pyfilter_amd.filters.particle.state import ParticleFilterCorrection
    from pyfilter_amd.timeseries import TimeseriesState
    from tests.helpers import build_ssm_from_case

    inp = fo.Inputs(model, 200, 3, 4, "half_zero")
    ssm = build_ssm_from_case(inp.case, torch.float64, "cpu")
    filt = SISR(ssm, inp.n, seed=3)
    filt.set_batch_shape(torch.Size([inp.b]))
    log_w = inp.w.log()  # (-inf where the weight is exactly 0)
    state = ParticleFilterCorrection(TimeseriesState(0, inp.x, ssm.hidden.event_shape), log_w.clone(), torch.zeros(inp.b, dtype=torch.float64),
                                     torch.arange(inp.n).unsqueeze(-1).expand(inp.n, inp.b))
    draws = filt._draws
    got = fo.as_dict(filt.forecast(state, inp.h, paths=True, z=inp.z, e=inp.e))
    assert filt._draws == draws and torch.equal(state.weights, log_w)
    w = normalized_weights(log_w)
    assert bool((w[::2, 0] == 0).all()) and bool(((w.sum(0) - 1.0).abs() < 1e-12).all())
    ref = fo.forecast(fo.rounded_spec(inp.case, torch.float64), inp.x, w, inp.z, inp.e)
    for k in fo.KEYS:
        assert got[k].shape == ref[k].shape, k
        torch.testing.assert_close(got[k], ref[k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{k}: {m}")
    a, b = filt.forecast(state, 2), filt.forecast(state, 2)
    assert a.paths is None and not torch.equal(a.x_mean, b.x_mean)
    c, d = filt.forecast(state, 2, seed=8), filt.forecast(state, 2, seed=8)
    assert torch.equal(c.x_mean, d.x_mean) and torch.equal(c.y_variance, d.y_variance)
