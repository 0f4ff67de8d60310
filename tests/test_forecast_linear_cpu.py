"""``pf_forecast_linear`` and predictive covariances without a GPU: the covariance oracle's own consistency, ``torch_forecast`` with
``covariance=True`` against it, ``mix_forecasts`` of covariances, the ``route`` argument, the C ABI's declarations, and the
conditions the float32 bars of ``tests/test_forecast_linear_gpu.py`` rest on."""
import os

import numpy as np
import pytest
import torch

from tests import forecast_oracle as fo
from tests import linmat_forecast_cases as FC
from tests import linmat_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _normalised(inp):
    w = torch.full((inp.n, inp.b), 1.0 / inp.n, dtype=torch.float64) if inp.w is None else inp.w
    return w / w.sum(0)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,o", [(1, 1), (4, 2), (3, 5), (8, 8)])
@pytest.mark.parametrize("weights", FC.WEIGHTS)
def test_covariance_oracle_is_consistent_with_the_moments_oracle(d, o, weights):
    inp = FC.inputs(d, o, 65, 3, 3, weights)
    ref = inp.reference()
    assert ref["x_cov"].shape == (3, 3, d, d) and ref["y_cov"].shape == (3, 3, o, o)
    torch.testing.assert_close(ref["x_cov"].diagonal(dim1=-2, dim2=-1), ref["x_var"], rtol=1e-13, atol=0.0)
    torch.testing.assert_close(ref["y_cov"].diagonal(dim1=-2, dim2=-1), ref["y_var"], rtol=1e-13, atol=0.0)
    for k in ("x_cov", "y_cov"):  # (symmetric up to the order in which torch adds the particles of either triangle)
        torch.testing.assert_close(ref[k], ref[k].transpose(-1, -2), rtol=1e-13, atol=1e-15)
    # sum W = 1: the observation's covariance is the image of the state's plus the observation's own
    w = _normalised(inp)
    spec = inp.case.spec(torch.float64)
    xc, yc = FC.covariances(spec, inp.x, w, inp.z)
    ao, _, so = spec.obs_params  # (B, O, D), (B, O)
    image = ao @ xc @ ao.transpose(-1, -2) + torch.diag_embed(so * so)
    v = yc.diagonal(dim1=-2, dim2=-1)
    assert float(((yc - image).abs() / (v.unsqueeze(-1) * v.unsqueeze(-2)).sqrt()).max()) <= 1e-12
    # ... and numpy's weighted covariance of the oracle's own paths
    paths = fo.forecast(spec, inp.x, w, inp.z)["x_path"]  # (H, N, B, D)
    for h in range(3):
        for k in range(inp.b):
            want = np.cov(paths[h, :, k].numpy().T, aweights=w[:, k].numpy(), ddof=0).reshape(d, d)
            vv = np.sqrt(np.outer(np.diag(want), np.diag(want)))
            assert float((np.abs(xc[h, k].numpy() - want) / vv).max()) <= 1e-12


# ---- torch_forecast(covariance=True) ------------------------------------------------------------------------------------------------
def _check_against(got, ref):
    for k in FC.KEYS:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        torch.testing.assert_close(got[k], ref[k], rtol=1e-9, atol=1e-9, msg=lambda m: f"{k}: {m}")


def test_torch_route_covariances_of_a_linear_model():
    from pyfilter_amd.filters.particle.forecast import torch_forecast
    from pyfilter_amd.timeseries import TimeseriesState

    inp = FC.inputs(4, 2, 65, 3, 3, "random")
    ssm = FC.linear_ssm(inp, torch.float64, "cpu")
    fc = torch_forecast(ssm, TimeseriesState(0, inp.x, ssm.hidden.event_shape), inp.w, inp.h, True, inp.z, inp.e, 0, covariance=True)
    _check_against(FC.forecast_dict(fc), inp.reference())
    plain = torch_forecast(ssm, TimeseriesState(0, inp.x, ssm.hidden.event_shape), inp.w, inp.h, False, inp.z, None, 0)
    assert plain.x_covariance is None and plain.y_covariance is None and torch.equal(plain.x_mean, fc.x_mean)
    assert "covariances: True" in repr(fc) and "covariances: False" in repr(plain)


@pytest.mark.parametrize("model,d,o", [("rw2d", 2, 2), ("sine", 1, 1)])
def test_torch_route_covariances_of_built_in_models(model, d, o):
    """The 2-D random walk, and a scalar state under a scalar observation: ``(steps, B, 1, 1)``"""
    from pyfilter_amd.filters.particle.forecast import torch_forecast
    from pyfilter_amd.timeseries import TimeseriesState
    from tests.helpers import build_ssm_from_case

    inp = fo.Inputs(model, 200, 3, 4, "random")
    ssm = build_ssm_from_case(inp.case, torch.float64, "cpu")
    fc = torch_forecast(ssm, TimeseriesState(0, inp.x, ssm.hidden.event_shape), inp.w, inp.h, True, inp.z, inp.e, 0, covariance=True)
    spec = fo.rounded_spec(inp.case, torch.float64)
    ref = fo.forecast(spec, inp.x, inp.w, inp.z, inp.e)
    ref["x_cov"], ref["y_cov"] = FC.covariances(spec, inp.x, inp.w, inp.z)
    assert fc.x_covariance.shape == (4, 3, d, d) and fc.y_covariance.shape == (4, 3, o, o)
    _check_against(FC.forecast_dict(fc), ref)
    # without the batch dimension
    solo = fo.Inputs(model, 200, 1, 2, "none")
    ssm1 = build_ssm_from_case(dict(solo.case, B=1), torch.float64, "cpu")
    fc1 = torch_forecast(ssm1, TimeseriesState(0, solo.x[:, 0], ssm1.hidden.event_shape), None, 2, False, solo.z[:, :, 0], None, 0, covariance=True)
    assert fc1.x_covariance.shape == (2, d, d) and fc1.y_covariance.shape == (2, o, o)


# ---- mix_forecasts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.0, 1e6])
def test_mix_forecasts_mixes_covariances(level):
    from pyfilter_amd.filters.particle import Forecast, mix_forecasts

    g = np.random.default_rng(5)
    steps, b, d, o = 3, 6, 4, 2
    w = g.uniform(0.1, 1.0, b)
    w /= w.sum()

    def member(k):
        mean = level + g.standard_normal((steps, b, k))
        root = g.standard_normal((steps, b, k, k))
        cov = root @ root.transpose(0, 1, 3, 2)
        return mean, cov

    (xm, xc), (ym, yc) = member(d), member(o)
    t = torch.from_numpy
    var = lambda c: np.ascontiguousarray(np.diagonal(c, axis1=-2, axis2=-1))  # noqa: E731
    fc = Forecast(t(xm), t(var(xc)), t(ym), t(var(yc)), None, x_covariance=t(xc), y_covariance=t(yc))
    mixed = mix_forecasts(t(w), fc)
    for mean, cov, got, got_var in ((xm, xc, mixed.x_covariance, mixed.x_variance), (ym, yc, mixed.y_covariance, mixed.y_variance)):
        mu = np.einsum("b,sbk->sk", w, mean)
        dm = mean - mu[:, None]
        want = np.einsum("b,sbij->sij", w, cov + dm[..., :, None] * dm[..., None, :])
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np.diagonal(got.numpy(), axis1=-2, axis2=-1), got_var.numpy(), rtol=1e-12, atol=1e-12)
    # a forecast without covariances mixes as before
    bare = mix_forecasts(t(w), Forecast(t(xm), t(var(xc)), t(ym), t(var(yc))))
    assert bare.x_covariance is None and bare.y_covariance is None and torch.equal(bare.x_variance, mixed.x_variance)
    # scalar members: means (steps, B), covariances (steps, B, 1, 1)
    sm, sc = t(xm[..., 0]), t(xc[..., :1, :1])
    scalar = mix_forecasts(t(w), Forecast(sm, sc[..., 0, 0], sm, sc[..., 0, 0], None, sc, sc))
    assert scalar.x_covariance.shape == (steps, 1, 1)
    torch.testing.assert_close(scalar.x_covariance[..., 0, 0], scalar.x_variance, rtol=1e-12, atol=1e-12)


# ---- ParticleFilter.forecast: route and covariance ----------------------------------------------------------------------------------------
def test_route_argument_and_covariance_slots_on_cpu_tensors():
    from pyfilter_amd import _lib as L
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.filters.particle.forecast import normalized_weights

    inp = FC.inputs(4, 2, 65, 3, 3, "half_zero")
    ssm = FC.linear_ssm(inp, torch.float64, "cpu")
    filt = SISR(ssm, inp.n, seed=3)
    filt.set_batch_shape(torch.Size([inp.b]))
    state = FC.filter_state(inp, ssm, torch.float64, "cpu")
    with pytest.raises(ValueError, match="route"):
        filt.forecast(state, 3, route="fastest")
    with pytest.raises(L.PfAmdError, match="no kernel"):
        filt.forecast(state, 3, route="kernel")
    with pytest.raises(L.PfAmdError, match="no kernel"):
        filt.forecast(state, 3, route="kernel", covariance=True)
    plain = filt.forecast(state, 3, z=inp.z, e=inp.e, paths=True)
    assert plain.x_covariance is None and plain.y_covariance is None
    # (the filter normalises the state's log-weights: the oracle gets what it makes of them)
    ref = FC.full_oracle(inp.case.spec(torch.float64), inp.x, normalized_weights(state.weights), inp.z, inp.e)
    for route in ("auto", "torch"):
        got = FC.forecast_dict(filt.forecast(state, 3, z=inp.z, e=inp.e, paths=True, route=route, covariance=True))
        _check_against(got, ref)
        assert torch.equal(got["x_mean"], plain.x_mean) and torch.equal(got["y_var"], plain.y_variance)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_pf_forecast_linear():
    from pyfilter_amd import _lib

    assert "pf_forecast_linear" in _lib.EXPORTS and "pf_forecast_linear_workspace_bytes" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "pf_amd.h")) as f:
        header = f.read()
    assert "int pf_forecast_linear(const pf_model* model, int steps," in header
    assert "int pf_forecast_linear_workspace_bytes(int64_t N, int64_t B, int steps, int64_t D, int64_t O, int covariance, size_t* bytes);" in header
    assert "#define PF_ABI_VERSION 4" in header
    with open(os.path.join(ROOT, "pyfilter_amd", "csrc", "pf_kernels.hip")) as f:
        source = f.read()
    assert source.index('#include "pf_linear_smooth.hpp"') < source.index('#include "pf_forecast_linear.hpp"')


# ---- the conditions the float32 bars rest on -------------------------------------------------------------------------------------------
def test_float32_cases_meet_the_conditions_of_their_bar():
    """For every float32 case of the GPU tests: the oracle's own float32 run is finite, has ``x_var >= 0`` and ``y_var > 0``, and
    differs from the float64 run (a bar of 4 x 0 would be the floor alone).  A case that fails goes into ``F32_EXCLUDED`` with a
    comment; no more than one in ten may."""
    cases = FC.float32_inputs()
    assert len(cases) >= 0.9 * (len(cases) + len(FC.F32_EXCLUDED))
    bad = []
    for inp in cases:
        low = inp.oracle_f32()
        finite = all(bool(torch.isfinite(low[k]).all()) for k in FC.KEYS)
        signs = bool((low["x_var"] >= 0).all()) and bool((low["y_var"] > 0).all())
        errs = FC.group_errors(low, inp.reference())
        if not (finite and signs and max(errs.values()) > 0.0 and all(np.isfinite(v) for v in errs.values())):
            bad.append((repr(inp), finite, signs, errs))
    assert not bad, bad


def test_edge_sizes_cover_the_tile_and_a_ragged_tail():
    for d in (1, 4, 5, 8):
        t, items = FC.ASSUMED_TILE[d], FC.ASSUMED_ITEMS[d]
        ns = FC.edge_n(t, items)
        assert ns[:4] == (1, t - 1, t, t + 1) and ns[4] > 3 * t and ns[4] % items != 0 and ns[4] % t != 0


def test_oracle_pack_row_layout_is_the_kernels():
    """``[A | b | s | A_o | b_o | s_o]``: the layout ``pf_forecast_linear`` reads is the one the cases pack"""
    inp = FC.inputs(3, 5, 65, 3, 3, "none")
    a, off, s, ao, bo, so = LO.split_row(inp.case.rows[1], 3, 5)
    assert a.shape == (3, 3) and ao.shape == (5, 3) and inp.case.rows.shape[1] == 9 + 6 + 15 + 10
    spec = inp.case.spec(torch.float64)
    assert np.array_equal(spec.hidden_params[0][1].numpy(), a) and np.array_equal(spec.obs_params[2][1].numpy(), so)
