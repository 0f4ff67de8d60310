"""``pf_smooth_ffbs_linear`` (``k_ffbs_linmat``, ``csrc/pf_linear_smooth.hpp``) - backward simulation for the ``PF_HID_LINEAR_MAT``
kind - called directly against the float64 oracle in both dtypes, and ``ParticleFilter.smooth(..., route=...)`` end to end (inputs:
``tests/linmat_smoothing_cases.py``; bars: ``tests/smoothing_cases.py``, those of ``tests/test_smoothing_kernels_gpu.py``).

A backward draw is checked on its own: the oracle's step t is teacher-forced with the kernel's output at t + 1.  A draw that agrees
with the float64 oracle is a bit-for-bit copy of that particle; one that differs lies within delta of every cdf boundary between the
two picks, and at most 1e-3 of a case's draws may differ.  float64: delta = N 2^-52 x 8.  float32: delta = 4 x the float32 oracle's
own cdf error against the float64 oracle on the same inputs.  Every filter has its own parameter row."""
import ctypes as C
import math

import pytest
import torch

from oracle import cpu_ref
from oracle import models as M
from tests import linear_cases as LC
from tests import linmat_smoothing_cases as lsc
from tests import smoothing_cases as sc
from tests.helpers import DT

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3  # include/pf_amd.h


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _run_ffbs(h, u=True, seed=3):
    from pyfilter_amd import ops

    kind, params = h.context()
    x_hist, logw, x_last, tape = h.soa()
    out = ops.smooth_ffbs_linear(kind, params, x_hist, logw, x_last, tape if u else None, seed)
    torch.cuda.synchronize()
    return h.from_soa(out)


def _check_against_oracle(h, out, label):
    """Every backward draw of ``out (S, N, B, D)`` over the history ``h`` against the float64 oracle; returns the oracle pass."""
    assert torch.equal(_bits(out[-1]), _bits(h.x_last)), f"{label}: the start of the backward pass is not x_last"
    nxt = lambda t: out[t]  # noqa: E731
    ref = sc.oracle_pass(h, torch.float64, x_next_of=nxt)
    if h.dtype == torch.float32:
        delta = sc.f32_delta(sc.oracle_pass(h, torch.float32, x_next_of=nxt), ref, 4.0)
    else:
        delta = sc.f64_delta(h.n)
    picks = [sc.recover_picks(h.x[t], out[t], prefer=ref["idx"][t]) for t in range(h.s - 1)]
    bad, total, worst = sc.compare_draws(h, picks, ref, delta, label)
    print(f"linmat-smoothing-parity: {label} {str(h.dtype)[6:]}: {bad} of {total} draws differ, largest boundary distance {worst:.3e}, delta {delta:.3e}")
    return ref, picks


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("d,n,b,s", lsc.DRAW_CASES, ids=[f"D{d}-{n}x{b}x{s}" for d, n, b, s in lsc.DRAW_CASES])
def test_every_draw_against_the_oracle(d, n, b, s, dt):
    h = lsc.synthetic(d, n, b, s, DT[dt])
    label = f"D{d} {n}x{b}x{s}"
    if s > 1:
        _check_against_oracle(h, _run_ffbs(h), label)
        return
    # S = 1: the output is x_last bit for bit and nothing else is written (a buffer twice the size, its tail a sentinel)
    from pyfilter_amd import _lib as L, ops

    kind, params = h.context()
    x_hist, logw, x_last, _ = h.soa()
    out = torch.full((2,) + tuple(x_hist.shape), -77.0, dtype=h.dtype, device="cuda")
    m = ops.make_model_struct(kind, params)
    L.check(L.load().pf_smooth_ffbs_linear(C.byref(m), x_hist.data_ptr(), logw.data_ptr(), x_last.data_ptr(), None, 3, out.data_ptr(), 1, n,
                                           b, L.dtype_code(h.dtype), L.stream_ptr()), "pf_smooth_ffbs_linear")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[0, 0]), _bits(x_last))
    assert bool((out[1] == -77.0).all())
    assert torch.equal(_bits(_run_ffbs(h)[0]), _bits(h.x_last))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("d,n,b,s", lsc.EDGE_CASES, ids=[f"D{d}-{n}x{b}x{s}" for d, n, b, s in lsc.EDGE_CASES])
def test_weight_and_offset_edges(d, n, b, s, dt):
    """A whole staged tile without mass (state 1, candidates 256..511); NaN, +inf and the lowest finite value among state 0's
    weights and, in column 1, all of its mass on candidate N - 1; u = 0 (the first candidate of positive mass) and u = 1 - eps
    (the last one, through the fallback)."""
    h = lsc.edge_history(d, n, b, s, DT[dt])
    out = _run_ffbs(h)
    ref, picks = _check_against_oracle(h, out, f"edges D{d} {n}x{b}x{s}")
    for t in range(s - 1):
        dead = cpu_ref.ffbs_sanitize_logw(h.logw[t]) == -math.inf
        assert not bool(dead.gather(0, picks[t]).any()), f"state {t}: a candidate without mass was drawn"
    assert bool((picks[0][:, 1] == n - 1).all())
    assert bool((picks[0][:10, 0] >= 3).all())  # (u = 0 over three leading candidates without mass)
    assert bool((picks[1] < 256).logical_or(picks[1] >= 512).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("d", [4, 8])
def test_philox_draws_follow_the_oracle_distribution(d, dt):
    """``u == NULL``: every trajectory of a column starts from the same value, so its N first backward draws are independent
    draws from one categorical the oracle knows - a chi-square over 32 equal-mass bins of the oracle's cdf (31 degrees of freedom:
    P(chi2 > 90) ~ 1e-7; fixed seed).  Same seed: same bits; another seed, and the other column (counter b N + j): other picks."""
    import numpy as np

    n, b = 4096, 2
    base = lsc.synthetic(d, n, 1, 2, DT[dt], seed=2)
    # both columns hold the same history and the same parameter row: only the Philox counter tells them apart
    both = lambda v: v.expand(v.shape[:1] + (b,) + v.shape[2:]).contiguous()  # noqa: E731
    h = lsc.History(np.repeat(base.rows, b, axis=0), d, DT[dt], [both(x) for x in base.x], [both(w) for w in base.logw],
                    both(base.x_last[:1].expand_as(base.x_last)), both(base.u[0])[None])
    out = _run_ffbs(h, u=False, seed=11)
    assert torch.equal(_bits(out), _bits(_run_ffbs(h, u=False, seed=11)))
    assert not torch.equal(_bits(out[0]), _bits(_run_ffbs(h, u=False, seed=12)[0]))
    picks = sc.recover_picks(h.x[0], out[0])
    assert bool((picks >= 0).all())
    assert torch.equal(_bits(out[1]), _bits(h.x_last))
    spec = h.spec(torch.float64)
    w = cpu_ref.ffbs_sanitize_logw(h.logw[0]).double()
    _, cdf = cpu_ref.ffbs_backward_step(spec, h.x[0].double(), w, h.x_last[:1].double(), torch.zeros(1, b, dtype=torch.float64))
    for c in range(b):
        cd = cdf[0, c]
        p = torch.diff(cd, prepend=torch.zeros(1, dtype=torch.float64))
        bins = torch.clamp((cd * 32).long(), max=31)
        mass = torch.zeros(32, dtype=torch.float64).scatter_add_(0, bins, p)
        obs = torch.bincount(bins[picks[:, c]], minlength=32).double()
        live = mass > 0
        assert bool((obs[~live] == 0).all())
        chi2 = ((obs[live] - n * mass[live]) ** 2 / (n * mass[live])).sum().item()
        print(f"linmat-smoothing-parity: philox D{d} {dt} column {c}: chi2 {chi2:.2f} over {int(live.sum())} bins")
        assert chi2 < 90.0, chi2
    assert not torch.equal(picks[:, 0], picks[:, 1])  # identical columns, draw counters b N + j


def test_entry_points_refuse_what_they_do_not_serve():
    """``pf_smooth_ffbs_linear``, ``pf_path_score_linear`` and the latter's workspace query: ``PF_EUNSUPPORTED`` for every built-in
    kind, ``PF_HID_USER_AFFINE``, ``PF_OBS_SV`` and D or O of 0 and 9; ``PF_EINVAL`` for S < 1 (S < 2 for the score), N or B < 1, a
    ``y_rows`` that is neither 1 nor B and null pointers - all before any launch: the outputs are untouched, and a good call
    afterwards works."""
    from pyfilter_amd import _lib as L

    lib = L.load()
    s, d, o, b, n = 3, 2, 2, 2, 64
    dev = "cuda"
    h = lsc.synthetic(d, n, b, s, torch.float64)
    kind, rows = h.context()
    x_hist, logw, x_last, _ = h.soa()
    y = torch.randn((s - 1, b, o), device=dev, dtype=torch.float64)
    out = torch.full((s, d, b, n), -77.0, device=dev, dtype=torch.float64)
    value = torch.full((b,), -77.0, device=dev, dtype=torch.float64)
    grad = torch.full((b, rows.shape[1]), -77.0, device=dev, dtype=torch.float64)
    ws = torch.empty(1 << 16, device=dev, dtype=torch.uint8)

    def model(hid=L.HID_LINEAR_MAT, obs=L.OBS_LINEAR, dim=d, obs_dim=o, params=rows):
        m = L.PfModel()
        m.hid_kind, m.obs_kind, m.dim, m.obs_dim, m.dt, m.inc_scale = hid, obs, dim, obs_dim, 1.0, 1.0
        m.params = params.data_ptr() if params is not None else None
        return m

    def ffbs(m, x=x_hist, S=s, N=n, B=b, dst=out):
        return lib.pf_smooth_ffbs_linear(C.byref(m) if m is not None else None, L.ptr(x), logw.data_ptr(), x_last.data_ptr(), None, 1,
                                         L.ptr(dst), S, N, B, L.PF_F64, L.stream_ptr())

    def score(m, p=x_hist, yy=y, rows_y=b, S=s, N=n, B=b, v=value, g=grad, w=ws):
        return lib.pf_path_score_linear(C.byref(m) if m is not None else None, L.ptr(p), L.ptr(yy), rows_y, L.ptr(v), L.ptr(g), L.ptr(w),
                                        ws.numel(), S, N, B, L.PF_F64, L.stream_ptr())

    for call in (ffbs, score):
        for hid in (L.HID_LINEAR, L.HID_SINE_EM, L.HID_VERHULST_EM, L.HID_LORENZ63_EM, L.HID_OU, L.HID_USER_AFFINE):
            assert call(model(hid=hid, dim=3 if hid == L.HID_LORENZ63_EM else d)) == EUNSUPPORTED, hid
        assert call(model(obs=L.OBS_SV)) == EUNSUPPORTED
        for bad in (0, 9):
            assert call(model(dim=bad)) == EUNSUPPORTED and call(model(obs_dim=bad)) == EUNSUPPORTED
        assert call(model(), N=0) == EINVAL and call(model(), B=0) == EINVAL
        assert call(None) == EINVAL and call(model(params=None)) == EINVAL
    good = model()
    assert ffbs(good, S=0) == EINVAL and ffbs(good, x=None) == EINVAL and ffbs(good, dst=None) == EINVAL
    assert score(good, S=1) == EINVAL and score(good, rows_y=3) == EINVAL and score(good, rows_y=0) == EINVAL
    assert score(good, p=None) == EINVAL and score(good, yy=None) == EINVAL and score(good, v=None) == EINVAL
    assert score(good, g=None) == EINVAL and score(good, w=None) == EINVAL
    nbytes = C.c_size_t(7)
    query = lib.pf_path_score_linear_workspace_bytes
    assert query(n, b, s, 0, o, C.byref(nbytes)) == EUNSUPPORTED and query(n, b, s, d, 9, C.byref(nbytes)) == EUNSUPPORTED
    assert query(n, b, 1, d, o, C.byref(nbytes)) == EINVAL and query(0, b, s, d, o, C.byref(nbytes)) == EINVAL
    assert query(n, b, s, d, o, None) == EINVAL and nbytes.value == 7
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()) and bool((value == -77.0).all()) and bool((grad == -77.0).all())
    assert query(n, b, s, d, o, C.byref(nbytes)) == 0 and 0 < nbytes.value <= ws.numel()
    assert ffbs(good) == 0 and score(good) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(value).all() and torch.isfinite(grad).all()
    assert torch.equal(out[-1], x_last) and not bool((grad == -77.0).any())


# ---------------------------------------------------------------------------------------------------- smooth(route=...) end to end
class _FixtureHistory(sc.History):
    """Recorded states of a ``tests/linear_cases.py`` fixture: the model's parameters (shared by the filters) from the fixture."""

    def __init__(self, g, dtype, x, logw, x_last, u):
        super().__init__("linmat-fixture", dtype, x, logw, x_last, u)
        self.g = g

    def spec(self, dtype):
        p = {k: self.g[k].to(dtype) for k in ("hid_A", "hid_b", "hid_s", "obs_A", "obs_b", "obs_s")}
        d, o = p["hid_A"].shape[0], p["obs_A"].shape[0]
        return M.ModelSpec(M.HID_LINEAR_MAT, (p["hid_A"], p["hid_b"], p["hid_s"]), d, 1.0, None, M.OBS_LINEAR,
                           (p["obs_A"], p["obs_b"], p["obs_s"]), o)


def _recorded(name="cv4d_apf_lgo", how="model"):
    g = LC.load(name, "f64")
    filt = LC.build_filter(name, g, torch.float64, "cuda", how=how, record_states=True)
    res = filt.batch_filter(g["y"].cuda(), bar=False, init_state=LC.start_at_x0(filt, g, "cuda"))
    return g, filt, list(res.states)


def test_smooth_routes_end_to_end():
    """``cv4d_apf_lgo`` in float64, states recorded by the HIP filter.  ``route="kernel"`` under a tape: every backward draw as in
    ``test_every_draw_against_the_oracle``, teacher-forced from the recorded states.  ``"auto"`` and ``"torch"`` under one torch
    seed: the same bits.  ``"kernel"`` for a lambda-built copy and for CPU states: ``PfAmdError``; another route: ``ValueError``."""
    from pyfilter_amd import _lib as L
    from pyfilter_amd import resampling
    from pyfilter_amd.filters.utils import batched_gather

    g, filt, states = _recorded()
    assert filt._model.kernel_kind.hid_kind == L.HID_LINEAR_MAT
    n, b, t_len = g["x0"].shape[0], g["x0"].shape[1], g["y"].shape[0]
    assert len(states) == t_len + 1
    gen = torch.Generator().manual_seed(17)
    u_back = torch.rand((t_len, n, b), generator=gen, dtype=torch.float64)
    u_last = torch.rand(b, generator=gen, dtype=torch.float64)
    filt._resampler = lambda w, normalized=False: resampling.systematic(w, normalized=normalized, u=u_last.cuda())
    filt.set_smoothing_tape(u_back)
    sm = filt.smooth(states, "ffbs", route="kernel")
    start = batched_gather(states[-1].timeseries_state.value, filt._resampler(states[-1].weights), 0)
    torch.cuda.synchronize()
    sm, start = sm.cpu(), start.cpu()
    assert sm.shape[0] == t_len + 1 and torch.equal(_bits(sm[-1]), _bits(start))
    h = _FixtureHistory(g, torch.float64, [s.timeseries_state.value.cpu() for s in states], [s.weights.cpu() for s in states], start, u_back)
    _check_against_oracle(h, sm, "cv4d_apf_lgo route=kernel")
    spec = h.spec(torch.float64)
    want = cpu_ref.smooth_ffbs(spec, h.x, h.logw, start, u_back)
    agree = (sm == want).all(-1).double().mean().item()
    print(f"linmat-smoothing-parity: cv4d_apf_lgo whole pass: {agree:.5f} of the path elements are the oracle's")
    filt.set_smoothing_tape(None)

    torch.manual_seed(11)
    auto = filt.smooth(states, "ffbs")
    torch.manual_seed(11)
    by_torch = filt.smooth(states, "ffbs", route="torch")
    assert torch.equal(_bits(auto), _bits(by_torch))
    assert torch.equal(_bits(filt.smooth(states, "fl", route="kernel")), _bits(filt.smooth(states, "fl")))

    with pytest.raises(ValueError):
        filt.smooth(states, "ffbs", route="hip")
    lam = LC.build_filter("cv4d_apf_lgo", g, torch.float64, "cuda", how="lambda")
    lam._ensure_context()
    with pytest.raises(L.PfAmdError, match="no backward-simulation kernel"):
        lam.smooth(states, "ffbs", route="kernel")
    from types import SimpleNamespace

    on_host = [SimpleNamespace(timeseries_state=SimpleNamespace(value=s.timeseries_state.value.cpu()), weights=s.weights.cpu()) for s in states]
    with pytest.raises(L.PfAmdError, match="no backward-simulation kernel"):
        filt.smooth(on_host, "ffbs", route="kernel")


def test_the_two_routes_draw_from_one_law():
    """The same recorded states of a 2 048-particle run smoothed by ``route="kernel"`` (Philox) and by ``route="torch"``: per (t,
    filter, component) the path means differ by at most ``5 sqrt(var_k / N + var_t / N)``, the two routes' own sample variances -
    FFBS paths are independent given the history, so that is the standard error of the difference; 5 sigma over a few hundred
    comparisons keeps the false-alarm rate near 1e-4."""
    name, n = "cv4d_apf_lgo", 2048
    g = LC.load(name, "f64")
    torch.manual_seed(5)
    filt = _with_particles(name, g, n)
    res = filt.batch_filter(g["y"].cuda(), bar=False)
    states = list(res.states)
    assert states[0].timeseries_state.value.shape[0] == n
    torch.manual_seed(6)
    k = filt.smooth(states, "ffbs", route="kernel").double()
    t = filt.smooth(states, "ffbs", route="torch").double()
    assert k.shape == t.shape == (len(states), n) + tuple(g["x0"].shape[1:])
    diff = (k.mean(1) - t.mean(1)).abs()
    se = (k.var(1) / n + t.var(1) / n).sqrt()
    live = se > 0  # (a component every path agrees on - the recorded state holds one value there - compares 0 <= 0)
    print(f"linmat-smoothing-parity: kernel vs torch route, {int(live.sum())} of {diff.numel()} comparisons with spread, "
          f"largest z {float((diff[live] / se[live]).max()):.2f}")
    print("linmat-smoothing-parity: states without spread:", sorted({int(i) for i in (~live).nonzero()[:, 0]}))
    assert int(live.sum()) >= diff.numel() // 2
    assert bool((diff <= 5.0 * se).all()), (diff / se).max()
    assert not torch.equal(k, t)


def _with_particles(name, g, n):
    from pyfilter_amd.filters.particle import APF, proposals

    ssm = LC.build_ssm(name, g, torch.float64, "cuda")
    filt = APF(ssm, n, proposal=proposals.LinearGaussianObservations(), ess_threshold=LC.CASES[name][2], record_states=True, seed=31)
    filt.set_batch_shape(torch.Size([g["x0"].shape[1]]))
    return filt
