"""Pins the oracle (``oracle/cpu_ref.py``) against golden vectors produced by the unmodified reference
(``oracle/make_golden.py``): per-step states, ancestors, log-likelihoods and the final FilterResult moments."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from oracle.cases import CASE_BY_NAME, CASES, CLUSTER_CASES, LEVEL_CASES, PARTIAL_NAN_CASES, build_spec
from tests.helpers import assert_close_nan_aware

DT = {"f64": torch.float64, "f32": torch.float32}
PARTIAL_PARAMS = [(c["name"], d) for c in PARTIAL_NAN_CASES for d in c["dtypes"]]
PARAMS = [(c["name"], d) for c in CASES for d in c["dtypes"]]
# (+ the reference's runs at column-cluster sizes, round 6: filtering arrays only)
# (+ the runs at a level of 1e4, oracle/cases.py: LEVEL_CASES)
FILTER_PARAMS = PARAMS + [(c["name"], d) for c in CLUSTER_CASES + LEVEL_CASES for d in c["dtypes"]]


def load(golden_dir, name, dt):
    with np.load(os.path.join(golden_dir, f"{name}_{dt}.npz")) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


@pytest.mark.parametrize("name,dt", FILTER_PARAMS)
def test_filter_matches_reference(golden_dir, name, dt):
    case = CASE_BY_NAME[name]
    dtype = DT[dt]
    g = load(golden_dir, name, dt)
    spec = build_spec(case, dtype)

    out = cpu_ref.batch_filter(
        spec, case["filter"], case["proposal"], g["y"], g["x0"], g["z_tape"].to(dtype), g["u_tape"].to(dtype),
        ess_threshold=case["ess_threshold"], record_steps=True,
    )

    # ancestors: exact
    assert torch.equal(out["step_idx"], g["step_idx"]), "ancestor indices differ from the reference"
    tol = dict(rtol=1e-12, atol=1e-13) if dt == "f64" else dict(rtol=2e-5, atol=2e-6)
    for k in ("step_x", "step_w", "step_ll"):
        torch.testing.assert_close(out[k], g[k], equal_nan=True, **tol)
    torch.testing.assert_close(out["filter_means"], g["filter_means"], **tol)
    torch.testing.assert_close(out["filter_variance"], g["filter_variance"], **tol)
    torch.testing.assert_close(out["loglikelihood"], g["loglikelihood"], **tol)


def _tol(dt):
    return dict(rtol=1e-12, atol=1e-13) if dt == "f64" else dict(rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("name,dt", PARTIAL_PARAMS)
def test_half_observed_rows_match_reference(golden_dir, name, dt):
    """Rows that are NaN in only SOME elements (``oracle/cases.py: PARTIAL_NAN_CASES``): the reference weighs them
    (``y.isnan().all()``, filters/base.py:212) and the affected columns go NaN / -inf for the step.  The oracle against the
    unmodified reference's arrays: identical ancestors, identical NaN and +-inf patterns, the rest at this file's tolerances."""
    case = CASE_BY_NAME[name]
    dtype = DT[dt]
    g = load(golden_dir, name, dt)
    spec = build_spec(case, dtype)
    out = cpu_ref.batch_filter(
        spec, case["filter"], case["proposal"], g["y"], g["x0"], g["z_tape"].to(dtype), g["u_tape"].to(dtype),
        ess_threshold=case["ess_threshold"], record_steps=True,
    )
    assert torch.equal(out["step_idx"], g["step_idx"]), "ancestor indices differ from the reference"
    for k in ("step_x", "step_w", "step_ll", "filter_means", "filter_variance", "loglikelihood"):
        assert_close_nan_aware(out[k], g[k], what=f"{name}/{dt} {k}", **_tol(dt))


def half_observed_steps(case, g):
    """``(T, B)`` bool: column b weighs a partly-NaN observation at step t (some NaN, not all) - per column for a per-series
    ``(T, B)`` y, every column for a shared ``(T, O)`` row - and ``(T,)`` bool: the whole row is NaN (a propagate-only move)."""
    y = g["y"]
    t_len, b = y.shape[0], case["B"]
    nan = y.isnan().reshape(t_len, -1)
    whole = nan.all(1)
    if case["model"] == "sv_batched":  # one scalar series per column
        return nan & ~whole.unsqueeze(1), whole
    return (nan.any(1) & ~whole).unsqueeze(1).expand(t_len, b), whole


@pytest.mark.parametrize("name,dt", PARTIAL_PARAMS)
def test_half_observed_fixtures_hold_the_semantics_they_pin(golden_dir, name, dt):
    """What the reference does to a half-observed column, read off the fixtures themselves - so that a regenerated fixture
    cannot silently lose its half-observed steps.  At such a step t of column b: ``step_ll`` NaN, recorded weights all -inf,
    moments row t + 1 NaN, an APF's ancestors all N - 1 (searchsorted over a NaN cdf whose last entry is 1), the run's
    log-likelihood NaN.  Columns that never see one stay finite throughout.  Under Bootstrap the column RECOVERS at its next
    fully observed step (finite ll and moments; a SISR column then sits at the lowest finite log-weight); under
    LinearGaussianObservations the proposal's mean takes the NaN, the particles are NaN from that step to the end of the run
    and nothing recovers - the fixture is asserted to show exactly that."""
    case = CASE_BY_NAME[name]
    g = load(golden_dir, name, dt)
    n, b, t_len = case["N"], case["B"], case["T"]
    half, whole = half_observed_steps(case, g)
    assert half.any(), "no half-observed step in the fixture"
    ll, w, idx = g["step_ll"].reshape(t_len, b), g["step_w"], g["step_idx"]
    means = g["filter_means"].reshape(t_len + 1, b, -1)
    lgo = case["proposal"] == "lgo"
    lowest = torch.finfo(DT[dt]).min
    recovered = 0
    for col in range(b):
        dead = prev_hit = False  # (dead - lgo: the column's particles are NaN from its first half-observed step on)
        for t in range(t_len):
            if whole[t]:
                continue
            x_nan = g["step_x"][t][:, col].isnan()
            if bool(half[t, col]) or dead:
                assert ll[t, col].isnan() and means[t + 1, col].isnan().all(), (t, col)
                assert (w[t][:, col] == -math.inf).all(), (t, col)
                if case["filter"] == "apf":
                    assert (idx[t][:, col] == n - 1).all(), (t, col)
                assert x_nan.all() if lgo else not x_nan.any(), (t, col)
                dead, prev_hit = lgo, True
            else:
                assert ll[t, col].isfinite() and means[t + 1, col].isfinite().all() and not x_nan.any(), (t, col)
                if prev_hit:  # the next fully observed step: the column is back
                    recovered += 1
                    if case["filter"] == "sisr":
                        assert (w[t][:, col] == lowest).all(), (t, col)
                prev_hit = False
        touched = bool(half[:, col].any())
        assert g["loglikelihood"].reshape(b)[col].isnan() == touched, col
        if not touched:
            assert ll[:, col].isfinite().all() and means[:, col].isfinite().all() and w[:, :, col].isfinite().all(), col
    assert lgo or recovered >= 1, "no column recovers at a fully observed step"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_primitives_match_reference(golden_dir, dt):
    g = load(golden_dir, "primitives", dt)
    # the reference's own known-answer arrangement (tests/test_resampling.py:31-47)
    idx = cpu_ref.systematic(g["ka_w"].moveaxis(0, 1), u=g["ka_u"], normalized=True).moveaxis(0, 1)
    assert torch.equal(idx, g["ka_idx"])

    for nm in "abc":
        lw = g[f"norm_{nm}_in"].clone()
        W = cpu_ref.normalize(lw)
        assert torch.equal(lw, g[f"norm_{nm}_inplace"])  # in-place nan_to_num semantics
        assert torch.equal(W, g[f"norm_{nm}_W"])
        assert torch.equal(cpu_ref.get_ess(W, normalized=True), g[f"norm_{nm}_ess"])
        assert torch.equal(cpu_ref.systematic(W, normalized=True, u=g[f"norm_{nm}_u"]), g[f"norm_{nm}_idx"])
        v = g[f"norm_{nm}_v"]
        torch.testing.assert_close(cpu_ref.log_likelihood(v, W), g[f"norm_{nm}_ll_w"], rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(cpu_ref.log_likelihood(v), g[f"norm_{nm}_ll"], rtol=0, atol=0)


def _recorded(g, case, dtype):
    """The reference's T + 1 recorded states from a fixture: (xs, ws, prev_inds) lists."""
    n, b = case["N"], case["B"]
    xs = [g["x0"]] + list(g["step_x"].unbind(0))
    ws = [torch.zeros(n, b, dtype=dtype)] + list(g["step_w"].unbind(0))
    idx0 = torch.arange(n).unsqueeze(-1).expand(n, b)
    return xs, ws, [idx0] + list(g["step_idx"].unbind(0))


@pytest.mark.parametrize("name,dt", PARAMS)
def test_fixed_lag_smoothing_matches_reference(golden_dir, name, dt):
    """``smooth(states, "fl")`` of the reference (particle/base.py:136-152) is pure index chasing: exact."""
    case = next(c for c in CASES if c["name"] == name)
    if case.get("observe_every_step", 1) != 1:
        pytest.skip("recorded states of a thinned run skip moves: no ancestor chain to follow")
    g = load(golden_dir, name, dt)
    xs, _, inds = _recorded(g, case, DT[dt])
    assert torch.equal(cpu_ref.smooth_fl(xs, inds), g["smooth_fl"])


@pytest.mark.parametrize("name", ["lg1d_sisr_boot", "sine_apf_lgo", "lorenz_sisr_boot", "sv_apf_boot", "rw2d_sisr_boot"])
def test_ffbs_oracle_against_reference_statistics(golden_dir, name):
    """``smooth(states, "ffbs")``: the reference's ``Categorical`` draws cannot be injected, so the oracle (inverse CDF on
    the same logits) is pinned statistically - the per-time mean over trajectories of 4 independent backward passes of
    the reference (fixture) against the oracle's, within Monte-Carlo error."""
    case = next(c for c in CASES if c["name"] == name)
    g = load(golden_dir, name, "f64")
    spec = build_spec(case, torch.float64)
    xs, ws, _ = _recorded(g, case, torch.float64)
    n, b = case["N"], case["B"]
    gen = torch.Generator().manual_seed(11)
    W = cpu_ref.normalize(ws[-1].clone())
    start_idx = cpu_ref.systematic(W, normalized=True, u=g["ffbs_u_last"].double().reshape(-1, 1))
    start = cpu_ref.batched_gather(xs[-1], start_idx, 0)
    draws = [cpu_ref.smooth_ffbs(spec, xs, ws, start, torch.rand((len(xs) - 1, n, b), generator=gen, dtype=torch.float64))
             for _ in range(4)]
    traj = torch.stack(draws)
    mean = traj.mean(dim=(0, 2))
    # both sides average 4 N trajectories that share ancestors heavily: allow 6 standard errors of N effective draws
    se = (g["ffbs_var"] / n).sqrt() * math.sqrt(2.0)
    assert ((mean - g["ffbs_mean"]).abs() <= 6.0 * se + 1e-9).all(), ((mean - g["ffbs_mean"]).abs() / (se + 1e-12)).max()
    # the last state is the resampled one on both sides, given the same uniform: exact
    torch.testing.assert_close(traj[0, -1].mean(dim=0), traj[1, -1].mean(dim=0), rtol=0, atol=0)
