"""``pf_smooth_mh`` (``k_smooth_mh_cdf`` / ``k_smooth_mh``, ``csrc/pf_smooth_mh.hpp``) - backward simulation by Metropolis-Hastings -
called directly through ``ops.smooth_mh`` in both dtypes, then through ``ParticleFilter.smooth(states, "ffbs-mh")`` and
``GradientBasedProposal(method="ffbs-mh")``.  Oracle, cases and bars: ``tests/smoothing_mh_oracle.py``.

Every chain of every step is compared with the float64 oracle teacher-forced with the kernel's own ``(out[t + 1], idx_out[t + 1])``.
``out[t]`` is a bit-for-bit copy of ``x_hist[t]`` at ``idx_out[t]``; a chain whose pick differs from the oracle's must have a cdf
boundary within ``delta_p`` of one of its proposal uniforms or an acceptance within ``delta_a`` of a tie, and at most 1e-3 of a
case's chains may differ.  float64: ``delta_p = sc.f64_delta(N)`` (the parallel scan's other order of additions), ``delta_a`` =
1e-9 max(1, |l|, |l'|).  float32: 4 x the float32 oracle's own error against the float64 oracle on the case, of the normalised cdf
and of l' - l.  Measured figures: ``profiles/smoothing_mh_parity.txt`` (the ``smoothing-mh-parity:`` lines these tests print)."""
import ctypes as C
import math

import pytest
import torch

from oracle import cpu_ref
from tests import linmat_smoothing_cases as lsc
from tests import smoothing_cases as sc
from tests import smoothing_mh_oracle as mh
from tests.helpers import DT, build_ssm_from_case

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3  # include/pf_amd.h
EDGE_MODELS = ("sine", "rw2d", 4)
EDGE_SHAPE = (600, 2, 3)


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _run(c, tape=True, seed=3):
    """``(out (S, N, B, [D]), idx (S, N, B) int64)`` on the CPU."""
    from pyfilter_amd import ops

    kind, params = c.h.context()
    x_hist, logw, anc, idx_last, u = c.device_inputs()
    out, idx = ops.smooth_mh(kind, params, x_hist, logw, anc, idx_last, u if tape else None, seed, c.k)
    torch.cuda.synchronize()
    return c.h.from_soa(out), idx.permute(0, 2, 1).cpu().to(torch.int64)


def _check(c, out, idx, what):
    """The bars of the module docstring; returns the float64 oracle's teacher-forced steps."""
    h = c.h
    for t in range(h.s):
        assert bool((idx[t] >= 0).all()) and bool((idx[t] < h.n).all()), f"{what}: state {t} names a particle outside the column"
        assert torch.equal(_bits(out[t]), _bits(sc.gather(h.x[t], idx[t]))), f"{what}: out[{t}] is not x_hist[{t}] at idx_out[{t}]"
    forced = lambda t: (out[t], idx[t])  # noqa: E731
    ref = mh.oracle_pass(c, torch.float64, forced=forced)
    low = mh.oracle_pass(c, torch.float32, forced=forced) if h.dtype == torch.float32 else None
    delta_p, delta_a = mh.deltas(c, ref, low)
    bad, total, worst_p, worst_a = mh.compare(c, idx, ref, delta_p, delta_a, what)
    print(f"smoothing-mh-parity: {what} {str(h.dtype)[6:]}: {bad} of {total} chains differ (margins {worst_p:.3e} / {worst_a:.3e}), "
          f"delta_p {delta_p:.3e}, delta_a {'1e-9 rel' if delta_a is None else format(delta_a, '.3e')}")
    return ref


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s,k", mh.DRAW_CASES, ids=mh.DRAW_IDS)
def test_every_chain_against_the_oracle(model, n, b, s, k, dt):
    c = mh.case(model, n, b, s, DT[dt], k)
    out, idx = _run(c)
    _check(c, out, idx, mh.label(model, n, b, s, k))
    if n == 1:
        assert bool((idx == 0).all())
    if s == 1:
        assert torch.equal(idx[0], c.idx_last)


def _live(c, t):
    return cpu_ref.ffbs_sanitize_logw(c.h.logw[t]) != -math.inf


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", EDGE_MODELS, ids=[str(m) for m in EDGE_MODELS])
def test_weight_and_draw_edges(model, dt):
    """``edge_history``'s weights - a NaN, a +inf and the lowest finite value on candidates 0, 1, 2 of column 0 of state 0, all of
    column 1's mass on candidate N - 1, no mass on candidates 256 .. 511 of state 1 - under K = 4: no candidate without mass is
    picked.  Chains 0 .. 9 draw u1 = 0 and u2 = 0 in every round: the first live candidate; chains 10 .. 19 u1 = 1 - eps, u2 = 0:
    the last live one - by the search: (1 - eps) x total is below the total in either dtype.  The fallback itself:
    ``test_the_fallback_is_the_last_candidate_of_positive_mass``."""
    n, b, s = EDGE_SHAPE
    dtype = DT[dt]
    c = mh.edge_case(model, n, b, s, dtype, 4)
    u = c.u.clone()
    u[:, :, :, :20] = 0.0
    u[:, :, 0, 10:20] = 1.0 - torch.finfo(dtype).eps
    c = c.edited(u=u)
    out, idx = _run(c)
    _check(c, out, idx, f"edges {mh.label(model, n, b, s, 4)}")
    for t in range(s - 1):
        live = _live(c, t)
        assert bool(live.gather(0, idx[t]).all()), f"state {t}: a candidate without mass was picked"
        cdf, last_pos = mh.cdf_of(c.h, t, torch.float64)
        first = (cdf > 0).to(torch.int64).argmax(dim=0)  # (B,)
        share = torch.diff(cdf, dim=0, prepend=torch.zeros(1, b, dtype=torch.float64)).gather(0, last_pos[None])[0] / cdf[-1]
        assert bool((share > 4.0 * torch.finfo(dtype).eps).all())  # (input condition: 1 - eps lies inside the last live candidate)
        assert torch.equal(idx[t][:10], first.expand(10, b)), f"state {t}: u1 = 0"
        assert torch.equal(idx[t][10:20], last_pos.expand(10, b)), f"state {t}: u1 = 1 - eps"
    assert bool((idx[0][:, 1] == n - 1).all())  # all of the column's mass on the last candidate
    assert bool((idx[0][:10, 0] >= 3).all())
    assert bool(((idx[1] < 256) | (idx[1] >= 512)).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", EDGE_MODELS, ids=[str(m) for m in EDGE_MODELS])
def test_the_fallback_is_the_last_candidate_of_positive_mass(model, dt):
    """``fallback_case``: the last 100 candidates of every state carry no mass, so the last live one is N - 101, not N - 1.  Chains
    0 .. 9 draw ``u1 = 1`` (and ``u2 = 0``) in every round: no cdf entry lies beyond ``u1 x total``, the oracle takes its fallback -
    asserted - and the kernel's pick is the ``last_pos`` its cdf kernel stored, candidate N - 101.  Chains 10 .. 19 draw
    ``u1 = 1 - eps``: the same candidate, by the search.  No chain picks a trailing candidate."""
    n, b, s = EDGE_SHAPE
    dtype = DT[dt]
    c = mh.fallback_case(model, n, b, s, dtype, 2)
    u = c.u.clone()
    u[:, :, 0, 10:20] = 1.0 - torch.finfo(dtype).eps
    c = c.edited(u=u)
    out, idx = _run(c)
    ref = _check(c, out, idx, f"fallback {mh.label(model, n, b, s, 2)}")
    last = n - 1 - mh.TRAILING_DEAD
    for t in range(s - 1):
        assert torch.equal(mh.cdf_of(c.h, t, torch.float64)[1], torch.full((b,), last))
        assert bool(ref[t]["fallback"][:, :10].all()) and not bool(ref[t]["fallback"][:, 10:].any())
        assert bool((idx[t][:20] == last).all()), f"state {t}: u1 = 1 and u1 = 1 - eps"
        assert bool((idx[t] <= last).all()), f"state {t}: a trailing candidate without mass was picked"


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", EDGE_MODELS, ids=[str(m) for m in EDGE_MODELS])
def test_a_dead_start_loses_and_a_zero_uniform_accepts(model, dt):
    """K = 1.  Every chain of column 0 starts state 0 at candidate 0, which has no mass, and draws u2 = 1 - eps (a live start
    keeps its place against every less likely proposal): the pick is the proposal.  With u2 = 0 everywhere the pick is the proposal
    at every state."""
    n, b, s = EDGE_SHAPE
    dtype = DT[dt]
    c = mh.edge_case(model, n, b, s, dtype, 1)
    anc = c.anc.clone()
    anc[1, :, 0] = 0
    u = c.u.clone()
    u[:, :, 1] = 1.0 - torch.finfo(dtype).eps
    dead = c.edited(anc=anc, u=u)
    out, idx = _run(dead)
    ref = _check(dead, out, idx, f"dead start {mh.label(model, n, b, s, 1)}")
    assert bool((ref[0]["cur"][0][:, 0] == 0).all()) and torch.equal(idx[0][:, 0], ref[0]["prop"][0][:, 0])
    assert bool(_live(dead, 0).gather(0, idx[0]).all())
    kept = (idx[1] == ref[1]["cur"][0]) & (ref[1]["cur"][0] != ref[1]["prop"][0])
    assert int(kept.sum()) > n // 8  # (u2 = 1 - eps: a live start of state 1 stays unless the proposal is at least as likely)
    u0 = c.u.clone()
    u0[:, :, 1] = 0.0
    zero = c.edited(u=u0)
    out, idx = _run(zero)
    ref = _check(zero, out, idx, f"u2 = 0 {mh.label(model, n, b, s, 1)}")
    for t in range(s - 1):
        assert torch.equal(idx[t], ref[t]["prop"][0])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", EDGE_MODELS, ids=[str(m) for m in EDGE_MODELS])
def test_a_single_particle_and_the_launch_trace(model, dt):
    """N = 1: every index is 0, under any draws.  The call leaves one record in the launch trace: SPEC = 22, sizeof(T), D."""
    from pyfilter_amd import ops

    c = mh.case(model, 1, 2, 3, DT[dt], 4)
    out, idx = _run(c)
    rec = ops.debug_launch_trace(1)[-1]
    assert (rec["ENTRY"], rec["SPEC"], rec["tbytes"], rec["D"]) == ("pf_smooth_mh", 22, 4 if dt == "f32" else 8, c.h.d)
    _check(c, out, idx, f"one particle {mh.label(model, 1, 2, 3, 4)}")
    assert bool((idx == 0).all())


def _direct(c, out, idx_out, s=None, n=None, k=None, ws_bytes=None, model=None, nulls=()):
    """``pf_smooth_mh`` itself on ``c``'s device inputs, with arguments replaced; returns the code."""
    from pyfilter_amd import _lib as L, ops

    lib = L.load()
    kind, params = c.h.context()
    x_hist, logw, anc, idx_last, _ = c.device_inputs()
    s, n = c.h.s if s is None else s, c.h.n if n is None else n
    need = C.c_size_t(0)
    assert lib.pf_smooth_mh_workspace_bytes(max(n, 1), c.h.b, max(s, 1), C.byref(need)) == 0
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device="cuda")
    m = ops.make_model_struct(kind, params) if model is None else model
    args = dict(x_hist=x_hist.data_ptr(), logw=logw.data_ptr(), anc=anc.data_ptr(), idx_last=idx_last.data_ptr(), out=out.data_ptr(),
                ws=ws.data_ptr())
    for name in nulls:
        args[name] = None
    rc = lib.pf_smooth_mh(C.byref(m) if m is not False else None, args["x_hist"], args["logw"], args["anc"], args["idx_last"], None, 5,
                          c.k if k is None else k, args["out"], L.ptr(idx_out), s, n, c.h.b, L.dtype_code(c.h.dtype), args["ws"],
                          need.value if ws_bytes is None else ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, (x_hist, logw, anc, idx_last, params, ws)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", EDGE_MODELS, ids=[str(m) for m in EDGE_MODELS])
def test_one_state_and_refused_calls(model, dt):
    """S = 1 writes ``out[0]`` = the last state at ``idx_last`` and ``idx_out[0]`` and nothing else (buffers twice the size, the
    tail a sentinel; no workspace).  ``mcmc_steps < 0``, S < 1, N < 1, a null mandatory pointer, a short workspace: ``PF_EINVAL``;
    a user-defined process, a built-in kind of four components, the matrix kind under a stochastic-volatility observation:
    ``PF_EUNSUPPORTED`` - all before any launch: the outputs are untouched."""
    from pyfilter_amd import _lib as L, ops

    n, b, s = EDGE_SHAPE
    dtype = DT[dt]
    c = mh.case(model, n, b, s, dtype, 4, seed=1)
    x_hist = c.device_inputs()[0]
    out = torch.full((2,) + tuple(x_hist.shape), -77.0, dtype=dtype, device="cuda")
    idx_out = torch.full((2, s, b, n), -5, dtype=torch.int32, device="cuda")
    # (S = 1 over the first state alone: the history's leading slice)
    rc, keep = _direct(c, out, idx_out, s=1, nulls=("ws",), ws_bytes=0)
    assert rc == 0
    idx_last = c.idx_last
    assert torch.equal(_bits(c.h.from_soa(out[0, :1])[0]), _bits(sc.gather(c.h.x[0], idx_last)))
    assert torch.equal(idx_out[0, 0].t().cpu().to(torch.int64), idx_last)
    assert bool((out.view(-1)[x_hist[0].numel():] == -77.0).all()) and bool((idx_out.view(-1)[b * n:] == -5).all())

    out.fill_(-77.0)
    idx_out.fill_(-5)
    kind, params = c.h.context()

    def model_of(**kw):
        m = ops.make_model_struct(kind, params)
        for key, v in kw.items():
            setattr(m, key, v)
        return m

    assert _direct(c, out, idx_out, k=-1)[0] == EINVAL
    assert _direct(c, out, idx_out, s=0)[0] == EINVAL
    assert _direct(c, out, idx_out, n=0)[0] == EINVAL
    for name in ("x_hist", "logw", "anc", "idx_last", "ws"):
        assert _direct(c, out, idx_out, nulls=(name,))[0] == EINVAL, name
    assert _direct(c, out, idx_out, model=False)[0] == EINVAL
    need = C.c_size_t(0)
    assert L.load().pf_smooth_mh_workspace_bytes(n, b, s, C.byref(need)) == 0 and need.value >= 8 * (s - 1) * b * n
    assert _direct(c, out, idx_out, ws_bytes=need.value - 1)[0] == EINVAL
    assert L.load().pf_smooth_mh_workspace_bytes(0, b, s, C.byref(need)) == EINVAL
    assert _direct(c, out, idx_out, model=model_of(hid_kind=L.HID_USER_AFFINE))[0] == EUNSUPPORTED
    assert _direct(c, out, idx_out, model=model_of(hid_kind=L.HID_LINEAR, dim=4, obs_dim=2))[0] == EUNSUPPORTED
    assert _direct(c, out, idx_out, model=model_of(hid_kind=L.HID_LINEAR_MAT, dim=9, obs_dim=2))[0] == EUNSUPPORTED
    assert _direct(c, out, idx_out, model=model_of(hid_kind=L.HID_LINEAR_MAT, dim=4, obs_dim=1, obs_kind=L.OBS_SV))[0] == EUNSUPPORTED
    assert bool((out == -77.0).all()) and bool((idx_out == -5).all())
    # ... and a NULL idx_out is served
    rc, _ = _direct(c, out, None)
    assert rc == 0 and bool((out[0] != -77.0).all()) and bool((out[1] == -77.0).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s", [("sine", 257, 2, 3), ("lorenz", 1000, 1, 4), (5, 1537, 3, 4)])
def test_no_rounds_from_the_identity_is_the_fixed_lag_smoother(model, n, b, s, dt):
    """K = 0 with ``idx_last = arange``: ``ops.smooth_fixed_lag`` bit for bit, and the indices are its ancestor walk."""
    from pyfilter_amd import ops

    c = mh.case(model, n, b, s, DT[dt], 0)
    c = c.edited(idx_last=torch.arange(n).unsqueeze(-1).expand(n, b).contiguous())
    out, idx = _run(c)
    x_hist, _, anc, _, _ = c.device_inputs()
    fl = ops.smooth_fixed_lag(x_hist, anc)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(c.h.from_soa(fl)))
    walk = c.idx_last
    for t in range(s - 2, -1, -1):
        walk = c.anc[t + 1].gather(0, walk)
        assert torch.equal(idx[t], walk)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s", [(m,) + sh for m in ("sine", 4) for sh in sc.EVERY_MODEL_AT],
                         ids=[f"{m}-{n}x{b}x{s}" for m in ("sine", 4) for n, b, s in sc.EVERY_MODEL_AT])
def test_philox_draws_replay_under_the_oracle(model, n, b, s, dt):
    """``u == NULL``: the same seed gives the same bits, another seed other picks, and every chain replays under the oracle fed
    with ``philox_ref``'s uniforms of call ``(b N + j) K + r`` of (seed, stream 10, step t) - under the bars of the tape mode."""
    dtype = DT[dt]
    c = mh.case(model, n, b, s, dtype, 4)
    out, idx = _run(c, tape=False, seed=11)
    again, idx_again = _run(c, tape=False, seed=11)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(idx, idx_again)
    assert not torch.equal(idx[:-1], _run(c, tape=False, seed=12)[1][:-1])
    replay = c.edited(u=mh.philox_uniforms(11, s, 4, n, b, dtype))
    _check(replay, out, idx, f"philox {mh.label(model, n, b, s, 4)}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", ["sine", "rw2d"])
def test_philox_chains_follow_the_backward_categorical(model, dt):
    """The law case of ``tests/test_smoothing_mh_oracle_cpu.py`` on the kernel's own draws: 4 096 chains from one x+, 16 live
    candidates, mostly dead starts, K = 64 - a chi-square below 60 against the categorical of ``cpu_ref.ffbs_backward_step``."""
    c = mh.law_case(model, DT[dt], 64)
    _, idx = _run(c, tape=False, seed=21)
    chi2, bins = mh.law_chi2(c, idx[0][:, 0])
    print(f"smoothing-mh-law: kernel {model} {dt} K=64: chi2 {chi2:.1f} over {bins} bins")
    assert chi2 < mh.CHI2_BAR, chi2


# ---- the public interface ---------------------------------------------------------------------------------------------------
N_PUB, T_PUB, B_PUB = 512, 12, 3


def _sine_filter(dtype, seed=9, **kw):
    from pyfilter_amd.filters.particle import APF, proposals

    filt = APF(build_ssm_from_case(dict(model="sine", B=B_PUB), dtype, "cuda"), N_PUB, proposal=proposals.LinearGaussianObservations(),
               record_states=True, seed=seed, **kw)
    filt.set_batch_shape(torch.Size([B_PUB]))
    y = 0.5 * torch.randn(T_PUB, generator=torch.Generator().manual_seed(4), dtype=torch.float64).cumsum(0)
    return filt, y.to(device="cuda", dtype=dtype)


def _tracker_filter(dtype, seed=17):
    from pyfilter_amd.filters.particle import SISR
    from tests import linmat_forecast_cases as FC

    theta = {"q": torch.linspace(0.3, 0.5, B_PUB, dtype=dtype, device="cuda"), "r": torch.linspace(0.4, 0.6, B_PUB, dtype=dtype, device="cuda")}
    filt = SISR(FC.tracker_builder(dtype, "cuda"), N_PUB, record_states=True, seed=seed)
    filt.set_batch_shape(torch.Size([B_PUB]))
    filt.initialize_model(theta)
    g = torch.Generator().manual_seed(8)
    y = torch.arange(T_PUB, dtype=torch.float64)[:, None] * torch.tensor([1.0, -0.5], dtype=torch.float64) \
        + 0.5 * torch.randn(T_PUB, 2, generator=g, dtype=torch.float64)
    return filt, y.to(device="cuda", dtype=dtype)


def _fix_resampler(filt, u_last):
    from pyfilter_amd import resampling

    filt._resampler = lambda w, normalized=False: resampling.systematic(w, normalized=normalized, u=u_last.cuda())


@pytest.mark.parametrize("which", ["sine", "tracker"])
def test_smooth_through_the_public_interface(which):
    """``smooth(states, "ffbs-mh", mcmc_steps=4)``: ``"ffbs"``'s shape, every row a particle of its state, reproducible from the
    filter's seed, and - under ``set_smoothing_tape`` - the oracle's pass over the recorded history (float64; teacher-forced with the
    picks recovered from the rows).  ``route="torch"`` and a user-lambda model raise ``PfAmdError``."""
    from pyfilter_amd import _lib as L
    from pyfilter_amd import timeseries as ts

    dtype, k = torch.float64, 4
    torch.manual_seed(5)  # (a LinearModel's initial sample is its initial kernel's: torch's generator)
    filt, y = _sine_filter(dtype) if which == "sine" else _tracker_filter(dtype)
    states = list(filt.batch_filter(y, bar=False).states)
    s = len(states)
    assert s == T_PUB + 1
    gen = torch.Generator().manual_seed(23)
    u_last = torch.rand(B_PUB, generator=gen, dtype=torch.float64)
    tape = torch.rand((s - 1, k, 2, N_PUB, B_PUB), generator=gen, dtype=torch.float64)
    _fix_resampler(filt, u_last)
    want_shape = filt.smooth(states, "ffbs").shape
    draws = filt._draws
    free = filt.smooth(states, "ffbs-mh", mcmc_steps=k)
    filt._draws = draws  # (the same draw seed again)
    assert torch.equal(free, filt.smooth(states, "ffbs-mh", mcmc_steps=k, route="kernel"))
    assert not torch.equal(free, filt.smooth(states, "ffbs-mh", mcmc_steps=k))  # (the next seed)
    assert free.shape == want_shape
    filt.set_smoothing_tape(tape)
    out = filt.smooth(states, "ffbs-mh", mcmc_steps=k).cpu()
    filt.set_smoothing_tape(None)
    idx_last = filt._resampler(states[-1].weights).cpu()
    torch.cuda.synchronize()

    xs = [st.timeseries_state.value.cpu() for st in states]
    ws = [st.weights.cpu() for st in states]
    anc = torch.stack([st.previous_indices.cpu().to(torch.int64) for st in states], 0)
    dummy = torch.zeros((s - 1, N_PUB, B_PUB), dtype=dtype)
    if which == "sine":
        h = sc.History("sine", dtype, xs, ws, xs[-1], dummy)
        h.case = dict(model="sine", N=N_PUB, B=B_PUB, proposal="lgo")
    else:
        h = lsc.History(filt._ensure_context().params.cpu().numpy(), 4, dtype, xs, ws, xs[-1], dummy)
    c = mh.Case(h, anc, idx_last, k, tape)
    own_out, own_idx = mh.paths_of(c, mh.oracle_pass(c, torch.float64))
    idx = torch.stack([sc.recover_picks(xs[t], out[t], prefer=own_idx[t]) for t in range(s)], 0)
    assert bool((idx >= 0).all()), "a row is no particle of its state"
    for rows in (free.cpu(),):
        assert all(bool((sc.recover_picks(xs[t], rows[t]) >= 0).all()) for t in range(s))
    _check(c, out, idx, f"smooth() {which} {N_PUB}x{B_PUB}x{s} K={k}")

    with pytest.raises(L.PfAmdError, match="ffbs"):
        filt.smooth(states, "ffbs-mh", route="torch")
    with pytest.raises(ValueError, match="mcmc_steps"):  # (the argument's own error, whatever the route)
        filt.smooth(states, "ffbs-mh", mcmc_steps=-1, route="torch")
    filt.set_smoothing_tape(torch.rand((s - 1, N_PUB, B_PUB), dtype=dtype))  # ("ffbs"'s tape, left behind)
    with pytest.raises(ValueError, match=r"\(S - 1, K, 2, N"):
        filt.smooth(states, "ffbs-mh", mcmc_steps=k)
    filt.set_smoothing_tape(None)
    if which == "sine":
        from torch.distributions import Normal

        from pyfilter_amd.filters.particle import SISR

        t = lambda v: torch.tensor(v, device="cuda", dtype=dtype)  # noqa: E731
        hidden = ts.AffineProcess(lambda x, a, sg: (a * x.value, sg), (t(0.9), t(0.5)), Normal(t(0.0), t(1.0)),
                                  initial_kernel=lambda a, sg: Normal(t(0.0), t(1.0)))
        user = SISR(ts.LinearStateSpaceModel(hidden, (t(1.0), t(0.5))), 64, record_states=True, seed=3)
        user.set_batch_shape(torch.Size([2]))
        user_states = user.batch_filter(y[:4], bar=False).states
        with pytest.raises(L.PfAmdError, match="ffbs"):
            user.smooth(user_states, "ffbs-mh")


def test_gradient_based_proposal_passes_the_method_through():
    """``GradientBasedProposal(method="ffbs-mh", mcmc_steps=4).build(...)``: a finite location that is neither the ``"fl"`` nor the
    ``"ffbs"`` one, and ``smooth`` is called with the method and the rounds."""
    from pyfilter_amd.inference import GradientBasedProposal
    from tests.test_gradient_proposal_gpu import _filtered

    y, theta, filt, state = _filtered(torch.float32)
    seen = []
    smooth = filt.smooth
    filt.smooth = lambda *a, **kw: seen.append((a[1], kw.get("mcmc_steps"))) or smooth(*a, **kw)
    locs = {m: GradientBasedProposal(scale=0.05, method=m, mcmc_steps=4).build(theta, state, filt, y).base_dist.loc for m in ("ffbs-mh", "fl", "ffbs")}
    filt.smooth = smooth
    assert seen[0] == ("ffbs-mh", 4)
    assert bool(torch.isfinite(locs["ffbs-mh"]).all())
    assert not torch.equal(locs["ffbs-mh"], locs["fl"]) and not torch.equal(locs["ffbs-mh"], locs["ffbs"])
